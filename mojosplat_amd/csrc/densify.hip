// The densification step of 3DGS training (adaptive density control), fused: clone, split and prune a scene of N Gaussians
// -- every parameter tensor, both Adam moments of each and the source map -- in three kernels and ONE host read.
// mojosplat_amd/refine.py holds the definition (densify_and_prune_torch); nothing in the reference does this (it is
// forward-only), the CUDA stack has gsplat's DefaultStrategy, a dozen boolean-index gathers and cats per tensor.
//
// OUTPUT ROWS, in this order, each segment in ascending source row (order-preserving compaction, no atomics):
//   [0, K)            originals      flag bit 0:  ~split & ~lowop & ~big
//   [K, K + C)        clones         flag bit 1:   clone & ~lowop & ~big
//   [K + C, K + C + S)  first children   flag bit 2:   split & ~lowop & ~childbig
//   [K + C + S, K + C + 2 S)  second children  (the same rows)
//
// k_densify_classify  one lane per Gaussian, kRows (256) per workgroup: reads the three statistics, the scales row and the
//                     opacity (28 bytes), decides in float32 -- IEEE division, no contraction, no exp: the scale tests are
//                     in log space against thresholds the HOST rounded once -- and writes the flag byte and the workgroup's
//                     counts of the three output kinds (and of the rows that leave nothing): ballots, no atomics.
// k_densify_scan      one workgroup, a wave per count kind: exclusive scan of the per-workgroup counts in place, kScanSpan
//                     (512: 8 per lane) workgroups per pass with a carry; the four totals go to `totals` for the host's read.
// k_densify_move      one workgroup per kRows SOURCE rows.  A lane per row rebuilds the row's destinations from the flags
//                     (ballot prefix + the scanned workgroup offset) into LDS, writes `source`, and -- for a split row --
//                     reads the quaternion, the scales and the two noise vectors and writes both children's means.  Then
//                     the workgroup walks the TABLE (kernel argument, up to MS_DENSIFY_MAX_TENSORS records of src, dst,
//                     width, kind): its kRows x width block of each tensor is read once, contiguously, and every element is
//                     stored to the row's destinations: kind COPY as it is everywhere; MEAN as it is to original and clone
//                     (the children's means were written above); SCALE minus log 1.6 to the children; MOMENT as it is to the
//                     original and ZERO to clone and children (no memset).  16-byte loads and stores when the width is a
//                     multiple of 4 and both pointers are 16-byte aligned (a vector then lies inside one row, on both
//                     sides), dword ones otherwise.  A row without destinations is not read.  As compaction keeps the
//                     order, a wave's stores land in at most four contiguous runs.
//
// BYTES per Gaussian with F floats per row over all parameters (14 with RGB, 59 with SH degree 3) and an optimiser attached:
// classify 28 + 1; move: the flag byte, 12 F read per source row that leaves an output, 24 of noise per split row, 12 F + 8
// (source) written per output row.  With ~5 % cloned, split and pruned each (new N = 1.05 N): ~ 24 F + 40 bytes per
// Gaussian -- 376 bytes (RGB), 1.46 kB (SH 3).
// Element offsets are 32-bit: a tensor of 2^31 elements or more, on either side, is REFUSED (MS_ERR_TOO_LARGE).
#include <math.h>

#include "ms_common.hpp"

namespace {

constexpr int kRows = MS_DENSIFY_ROWS;            // rows of a workgroup = its lanes
constexpr int kScanItems = 8;                     // counts per lane and pass of the scan
constexpr int kScanSpan = MS_DENSIFY_SCAN_SPAN;   // counts per pass of a wave
constexpr int kKinds = 4;                         // originals, clones, children, rows that leave nothing
static_assert(kScanSpan == 64 * kScanItems && kRows == 256, "the scan runs a wave per kind, the move a lane per row");

constexpr float kLog16 = (float)0.47000362924573556;   // float32(log 1.6), as refine.py forms it

struct MoveRec {
    const float *src;
    float *dst;
    uint32_t width;
    uint32_t kind;          // ms_densify_kind | 16 when 16-byte accesses are allowed
};
struct MoveTable {
    MoveRec rec[MS_DENSIFY_MAX_TENSORS];
};
static_assert(sizeof(MoveRec) == 24, "the table is a kernel argument: keep it small");

struct SplitArgs {          // the row path of the move (all null on a later chunk of the table)
    const float *means3d, *scales, *quats, *noise;
    float *out_means3d;
    int64_t *source;
};

// torch's max: a NaN wins
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }

__global__ void __launch_bounds__(kRows)
k_densify_classify(uint32_t N, const float *__restrict__ grad2d, const float *__restrict__ count,
                   const float *__restrict__ max_radii, const float *__restrict__ scales,
                   const float *__restrict__ opacities, const ms_densify_rules r, uint8_t *__restrict__ flags,
                   uint32_t *__restrict__ counts, uint32_t nb) {
#pragma clang fp contract(off)
    __shared__ uint32_t wave_counts[kKinds][kRows / 64];
    const uint32_t row = blockIdx.x * (uint32_t)kRows + threadIdx.x;
    uint32_t f = 0;
    const bool live = row < N;
    if (live) {
        const float c = count[row];
        const float g = grad2d[row] / (c < 1.0f ? 1.0f : c);      // clamp_min(1): a NaN count stays NaN
        const float rad = max_radii[row], op = opacities[row];
        const float smax = max_nan(max_nan(scales[3 * row], scales[3 * row + 1]), scales[3 * row + 2]);
        const bool high = g > r.grow_grad2d, small = smax <= r.log_grow;
        const bool clone = high && small;
        const bool split = (high && !small) || rad > r.grow_radius;
        const bool lowop = op < r.thr_opa;
        const bool rad_big = rad > r.prune_radius;
        const bool big = smax > r.log_big || rad_big;
        const bool childbig = (smax - kLog16) > r.log_big || rad_big;
        f = (uint32_t)(!split && !lowop && !big) | (uint32_t)(clone && !lowop && !big) << 1 |
            (uint32_t)(split && !lowop && !childbig) << 2;
        flags[row] = (uint8_t)f;
    }
    const int wave = threadIdx.x >> 6;
    const uint64_t b0 = __ballot(f & 1u), b1 = __ballot(f & 2u), b2 = __ballot(f & 4u), b3 = __ballot(live && f == 0u);
    if ((threadIdx.x & 63) == 0) {
        wave_counts[0][wave] = __popcll(b0);
        wave_counts[1][wave] = __popcll(b1);
        wave_counts[2][wave] = __popcll(b2);
        wave_counts[3][wave] = __popcll(b3);
    }
    __syncthreads();
    if (threadIdx.x < kKinds) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < kRows / 64; ++w) s += wave_counts[threadIdx.x][w];
        counts[threadIdx.x * nb + blockIdx.x] = s;
    }
}

// wave `k` scans counts[k * nb .. (k + 1) * nb) in place (exclusive) and writes its total
__global__ void __launch_bounds__(64 * kKinds)
k_densify_scan(uint32_t *__restrict__ counts, uint32_t nb, int64_t *__restrict__ totals) {
    const int lane = threadIdx.x & 63, kind = threadIdx.x >> 6;
    uint32_t *c = counts + (size_t)kind * nb;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += kScanSpan) {
        const uint32_t first = base + lane * kScanItems;
        uint32_t v[kScanItems], sum = 0;
#pragma unroll
        for (int j = 0; j < kScanItems; ++j) {
            v[j] = first + j < nb ? c[first + j] : 0u;
            sum += v[j];
        }
        uint32_t incl = sum;                        // inclusive scan of the lanes' sums
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        uint32_t run = carry + incl - sum;
#pragma unroll
        for (int j = 0; j < kScanItems; ++j) {
            if (first + j < nb) c[first + j] = run;
            run += v[j];
        }
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) totals[kind] = (int64_t)carry;
}

// both children of one split row: mean + R(q / |q|) (exp(scales) * noise[c])
__device__ __forceinline__ void child_means(const float *__restrict__ means3d, const float *__restrict__ scales,
                                            const float *__restrict__ quats, const float *__restrict__ noise,
                                            float *__restrict__ out_means3d, uint32_t N, uint32_t row, uint32_t d2, uint32_t d3) {
#pragma clang fp contract(off)
    const float qw = quats[4 * row], qx = quats[4 * row + 1], qy = quats[4 * row + 2], qz = quats[4 * row + 3];
    const float norm = sqrtf(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    const float w = qw / norm, x = qx / norm, y = qy / norm, z = qz / norm;
    const float r00 = 1.f - 2.f * (y * y + z * z), r01 = 2.f * (x * y - w * z), r02 = 2.f * (x * z + w * y);
    const float r10 = 2.f * (x * y + w * z), r11 = 1.f - 2.f * (x * x + z * z), r12 = 2.f * (y * z - w * x);
    const float r20 = 2.f * (x * z - w * y), r21 = 2.f * (y * z + w * x), r22 = 1.f - 2.f * (x * x + y * y);
    const float sx = expf(scales[3 * row]), sy = expf(scales[3 * row + 1]), sz = expf(scales[3 * row + 2]);
    const float mx = means3d[3 * row], my = means3d[3 * row + 1], mz = means3d[3 * row + 2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float *n = noise + ((size_t)c * N + row) * 3;
        const float vx = sx * n[0], vy = sy * n[1], vz = sz * n[2];
        float *o = out_means3d + (size_t)(c ? d3 : d2) * 3;
        o[0] = mx + ((r00 * vx + r01 * vy) + r02 * vz);
        o[1] = my + ((r10 * vx + r11 * vy) + r12 * vz);
        o[2] = mz + ((r20 * vx + r21 * vy) + r22 * vz);
    }
}

__global__ void __launch_bounds__(kRows)
k_densify_move(const MoveTable tab, int n_tensors, uint32_t N, const uint8_t *__restrict__ flags,
               const uint32_t *__restrict__ offsets, uint32_t nb, uint32_t n_kept, uint32_t n_cloned, uint32_t n_split,
               const SplitArgs sa) {
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    __shared__ uint32_t wave_counts[3][kRows / 64];
    __shared__ uint32_t dest[3][kRows];          // the row's original, clone and first child (kNone: it has none)
    const uint32_t row0 = blockIdx.x * (uint32_t)kRows, row = row0 + threadIdx.x;
    const uint32_t f = row < N ? flags[row] : 0u;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t pre[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint64_t b = __ballot((f >> k) & 1u);
        pre[k] = __popcll(b & below);
        if (lane == 0) wave_counts[k][wave] = __popcll(b);
    }
    __syncthreads();
    const uint32_t seg[3] = {0u, n_kept, n_kept + n_cloned}, len[3] = {n_kept, n_cloned, n_split};
    uint32_t d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint32_t in_seg = offsets[k * nb + blockIdx.x] + pre[k];
#pragma unroll
        for (int w = 0; w < kRows / 64 - 1; ++w) in_seg += w < wave ? wave_counts[k][w] : 0u;
        // (in_seg < len: the totals are the scan's own; a caller's mismatch must not become a store out of bounds)
        d[k] = ((f >> k) & 1u) && in_seg < len[k] ? seg[k] + in_seg : kNone;
        dest[k][threadIdx.x] = d[k];
    }
    if (sa.source) {
        if (d[0] != kNone) sa.source[d[0]] = row;
        if (d[1] != kNone) sa.source[d[1]] = row;
        if (d[2] != kNone) {
            sa.source[d[2]] = row;
            sa.source[d[2] + n_split] = row;
            child_means(sa.means3d, sa.scales, sa.quats, sa.noise, sa.out_means3d, N, row, d[2], d[2] + n_split);
        }
    }
    __syncthreads();

    const uint32_t rows_here = N - row0 < (uint32_t)kRows ? N - row0 : (uint32_t)kRows;
    for (int t = 0; t < n_tensors; ++t) {
        const MoveRec r = tab.rec[t];
        const uint32_t kind = r.kind & 15u;
        const bool to_children = kind != MS_DENSIFY_MEAN;
        if (r.kind & 16u) {
            const uint32_t w4 = r.width >> 2, total = rows_here * w4;
            const float4 *src = reinterpret_cast<const float4 *>(r.src) + (size_t)row0 * w4;
            float4 *dst = reinterpret_cast<float4 *>(r.dst);
            for (uint32_t i = threadIdx.x; i < total; i += kRows) {
                const uint32_t lr = i / w4, col = i - lr * w4;
                const uint32_t d0 = dest[0][lr], d1 = dest[1][lr], d2 = dest[2][lr];
                if ((d0 & d1 & d2) == kNone) continue;
                const float4 v = src[i];
                const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
                if (d0 != kNone) dst[(size_t)d0 * w4 + col] = v;
                if (d1 != kNone) dst[(size_t)d1 * w4 + col] = kind == MS_DENSIFY_MOMENT ? zero : v;
                if (d2 != kNone) {               // (width 3 never comes here: this is a copy or a moment)
                    const float4 cv = kind == MS_DENSIFY_MOMENT ? zero : v;
                    dst[(size_t)d2 * w4 + col] = cv;
                    dst[(size_t)(d2 + n_split) * w4 + col] = cv;
                }
            }
        } else {
            const uint32_t width = r.width, total = rows_here * width;
            const float *src = r.src + (size_t)row0 * width;
            for (uint32_t i = threadIdx.x; i < total; i += kRows) {
                const uint32_t lr = i / width, col = i - lr * width;
                const uint32_t d0 = dest[0][lr], d1 = dest[1][lr], d2 = dest[2][lr];
                if ((d0 & d1 & d2) == kNone) continue;
                const float v = src[i];
                if (d0 != kNone) r.dst[(size_t)d0 * width + col] = v;
                if (d1 != kNone) r.dst[(size_t)d1 * width + col] = kind == MS_DENSIFY_MOMENT ? 0.f : v;
                if (d2 != kNone && to_children) {
                    const float cv = kind == MS_DENSIFY_MOMENT ? 0.f : kind == MS_DENSIFY_SCALE ? v - kLog16 : v;
                    r.dst[(size_t)d2 * width + col] = cv;
                    r.dst[(size_t)(d2 + n_split) * width + col] = cv;
                }
            }
        }
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

constexpr int64_t kMaxElements = (int64_t)1 << 31;

size_t flags_bytes(int64_t N) { return ms::align_up((size_t)N, 16); }
int64_t blocks_of(int64_t N) { return ms::ceil_div(N, kRows); }

}  // namespace

extern "C" size_t ms_densify_workspace_bytes(int64_t N) {
    if (N <= 0) return 0;
    return flags_bytes(N) + (size_t)blocks_of(N) * kKinds * sizeof(uint32_t);
}

extern "C" int ms_densify_classify(int64_t N, const float *grad2d, const float *count, const float *max_radii,
                                   const float *scales, const float *opacities, const ms_densify_rules *rules,
                                   void *workspace, size_t workspace_bytes, int64_t *totals, void *stream_) {
    MS_REQUIRE(N >= 0, MS_ERR_INVALID_ARG, "densify_classify: negative size (N = %lld)", (long long)N);
    MS_REQUIRE(rules, MS_ERR_INVALID_ARG, "densify_classify: null pointer (rules)");
    MS_REQUIRE(!isnan(rules->grow_grad2d) && !isnan(rules->log_grow) && !isnan(rules->grow_radius) && !isnan(rules->thr_opa) &&
                   !isnan(rules->log_big) && !isnan(rules->prune_radius),
               MS_ERR_INVALID_ARG, "densify_classify: a threshold is NaN (a rule that is off is +inf)");
    if (N == 0) return MS_OK;
    MS_REQUIRE(grad2d && count && max_radii && scales && opacities && workspace && totals, MS_ERR_INVALID_ARG,
               "densify_classify: null pointer (grad2d, count, max_radii, scales, opacities, workspace or totals)");
    MS_REQUIRE(3 * N < kMaxElements, MS_ERR_TOO_LARGE, "densify_classify: %lld x 3 elements, 2^31 or more (32-bit offsets)",
               (long long)N);
    MS_REQUIRE(workspace_bytes >= ms_densify_workspace_bytes(N), MS_ERR_WORKSPACE,
               "densify_classify: workspace of %zu bytes, %zu needed", workspace_bytes, ms_densify_workspace_bytes(N));
    uint8_t *flags = (uint8_t *)workspace;
    uint32_t *counts = (uint32_t *)(flags + flags_bytes(N));
    const uint32_t nb = (uint32_t)blocks_of(N);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_densify_classify, dim3(nb), dim3(kRows), 0, stream, (uint32_t)N, grad2d, count, max_radii, scales,
                       opacities, *rules, flags, counts, nb);
    MS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_densify_scan, dim3(1), dim3(64 * kKinds), 0, stream, counts, nb, totals);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

extern "C" int ms_densify_move(int64_t N, int64_t n_kept, int64_t n_cloned, int64_t n_split, const void *workspace,
                               size_t workspace_bytes, int n_tensors, const ms_densify_tensor *tensors,
                               const float *means3d, const float *scales, const float *quats, const float *noise,
                               float *out_means3d, int64_t *source, void *stream_) {
    MS_REQUIRE(N >= 0 && n_kept >= 0 && n_cloned >= 0 && n_split >= 0, MS_ERR_INVALID_ARG,
               "densify_move: negative size (N %lld, kept %lld, cloned %lld, split %lld)", (long long)N, (long long)n_kept,
               (long long)n_cloned, (long long)n_split);
    MS_REQUIRE(n_kept <= N && n_cloned <= N && n_split <= N, MS_ERR_INVALID_ARG,
               "densify_move: more kept (%lld), cloned (%lld) or split (%lld) rows than the %lld there are", (long long)n_kept,
               (long long)n_cloned, (long long)n_split, (long long)N);
    MS_REQUIRE(n_tensors >= 0 && n_tensors <= MS_DENSIFY_MAX_TENSORS, MS_ERR_INVALID_ARG,
               "densify_move: n_tensors = %d, not in [0, %d]", n_tensors, MS_DENSIFY_MAX_TENSORS);
    const int64_t n_out = n_kept + n_cloned + 2 * n_split;
    if (N == 0 || n_out == 0) return MS_OK;
    const int row_ptrs = (means3d != nullptr) + (scales != nullptr) + (quats != nullptr) + (noise != nullptr) +
                         (out_means3d != nullptr) + (source != nullptr);
    MS_REQUIRE(row_ptrs == 0 || row_ptrs == 6, MS_ERR_INVALID_ARG,
               "densify_move: null pointer (means3d, scales, quats, noise, out_means3d and source go together: all or none)");
    MS_REQUIRE(workspace, MS_ERR_INVALID_ARG, "densify_move: null pointer (workspace)");
    MS_REQUIRE(n_tensors == 0 || tensors, MS_ERR_INVALID_ARG, "densify_move: null pointer (tensors)");
    MS_REQUIRE(n_tensors > 0 || row_ptrs, MS_ERR_INVALID_ARG, "densify_move: nothing to move (no tensor and no row outputs)");
    MS_REQUIRE(3 * N < kMaxElements && 3 * n_out < kMaxElements, MS_ERR_TOO_LARGE,
               "densify_move: %lld -> %lld rows of 3 elements, 2^31 or more (32-bit offsets)", (long long)N, (long long)n_out);
    MoveTable tab = {};
    for (int i = 0; i < n_tensors; ++i) {
        const ms_densify_tensor &t = tensors[i];
        MS_REQUIRE(t.src && t.dst, MS_ERR_INVALID_ARG, "densify_move: null pointer (tensor %d: src or dst)", i);
        MS_REQUIRE(t.width > 0, MS_ERR_INVALID_ARG, "densify_move: tensor %d: non-positive size (width %lld)", i, (long long)t.width);
        MS_REQUIRE(t.kind >= MS_DENSIFY_COPY && t.kind <= MS_DENSIFY_MOMENT, MS_ERR_INVALID_ARG,
                   "densify_move: tensor %d: kind %d is none of copy, mean, scale, moment", i, t.kind);
        MS_REQUIRE(t.width < kMaxElements && N * t.width < kMaxElements && n_out * t.width < kMaxElements, MS_ERR_TOO_LARGE,
                   "densify_move: tensor %d: %lld -> %lld rows x %lld elements, 2^31 or more (32-bit offsets)", i, (long long)N,
                   (long long)n_out, (long long)t.width);
        MS_REQUIRE((t.kind != MS_DENSIFY_MEAN && t.kind != MS_DENSIFY_SCALE) || t.width == 3, MS_ERR_INVALID_ARG,
                   "densify_move: tensor %d: a mean or scale tensor of width %lld, not 3", i, (long long)t.width);
        MoveRec &r = tab.rec[i];
        r.src = t.src;
        r.dst = t.dst;
        r.width = (uint32_t)t.width;
        r.kind = (uint32_t)t.kind | ((t.width % 4 == 0 && aligned16(t.src) && aligned16(t.dst)) ? 16u : 0u);
    }
    MS_REQUIRE(workspace_bytes >= ms_densify_workspace_bytes(N), MS_ERR_WORKSPACE,
               "densify_move: workspace of %zu bytes, %zu needed", workspace_bytes, ms_densify_workspace_bytes(N));
    const uint8_t *flags = (const uint8_t *)workspace;
    const uint32_t *offsets = (const uint32_t *)(flags + flags_bytes(N));
    const uint32_t nb = (uint32_t)blocks_of(N);
    const SplitArgs sa = {means3d, scales, quats, noise, out_means3d, source};
    hipLaunchKernelGGL(k_densify_move, dim3(nb), dim3(kRows), 0, (hipStream_t)stream_, tab, n_tensors, (uint32_t)N, flags,
                       offsets, nb, (uint32_t)n_kept, (uint32_t)n_cloned, (uint32_t)n_split, sa);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
