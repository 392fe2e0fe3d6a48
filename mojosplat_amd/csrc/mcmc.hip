// The 3DGS-MCMC strategy (Kheradmand et al. 2024; gsplat's MCMCStrategy) on a scene of N Gaussians: relocate dead
// Gaussians onto live ones sampled by opacity, grow the scene the same way, and perturb the means with covariance-shaped
// noise.  mojosplat_amd/mcmc.py holds the definition (relocate_dead_torch, grow_torch, inject_noise_torch); nothing in the
// reference does this (it is forward-only).  No host wait anywhere: the number of dead rows stays on the device.
//
// SAMPLE (ms_mcmc_sample), four launches:
// k_mcmc_classify  one lane per Gaussian, kRows (256) per workgroup: dead = !(opacity > thr) on the stored value, the
//                  integer weight w = dead ? 0 : round(o 2^24) (exact in float32), the workgroup's sum of weights and its
//                  number of dead rows; zeroes the row's draw count.
// k_mcmc_scan      one workgroup, a wave per kind (weights, dead rows): exclusive int64 scan of the per-workgroup sums,
//                  kScanSpan (512) per pass with a carry; leaves total, n_dead and n (the draws that will be applied).
// k_mcmc_cumsum    the inclusive int64 scan of the weights inside each workgroup on top of its offset (`cum`), and the dead
//                  rows' ranks by ballot prefix: targets[rank] = row, ascending (order-preserving, no atomics).
// k_mcmc_draw      one lane per draw: t = min(floor(u total), total - 1) in double, a binary search for the first row with
//                  cum > t (a zero-weight row is never that), an INTEGER atomic on the source's count (order-independent,
//                  so the counts are bitwise reproducible).  A caller's own `sampled` bypasses the search.
// APPLY (ms_mcmc_apply), two phases so that no thread copies a row another one is rewriting:
// k_mcmc_values    one lane per Gaussian: the row's NEW stored opacity and scales from its OLD ones and its count, in double
//                  (a few hundred rows every hundred steps; the alternating binomial sum cancels), into the workspace.  A
//                  row nobody drew keeps its values.
// k_mcmc_apply     one workgroup per kRows draws walks the TABLE (kernel argument, up to MS_MCMC_MAX_TENSORS records of
//                  base, width, kind), in place: kind COPY: row target <- row source (sources are alive, targets dead or
//                  appended: nobody writes a row that is read); OPACITY / SCALE: source and target <- the workspace's new
//                  values (never the tensor's: idempotent, so many draws of one source store the same bits); MOMENT:
//                  source and target <- 0.  16-byte accesses when the width is a multiple of 4 and the base 16-byte aligned.
// NOISE (ms_mcmc_noise), one launch, one Gaussian per lane, no scratch:
// k_mcmc_noise     means += R (exp(2 s) * (R^T v)), v = noise * gate * step: 56 bytes read and 12 written per Gaussian.
//
// BYTES with F floats per row over all parameters (14 with RGB, 59 with SH degree 3) and an optimiser attached: noise 68 per
// Gaussian; sample and values 17 (classify) + 17 (cumsum) + 36 (values) = 70 per Gaussian; per draw 184 of sampling (the
// uniform, ~20 probes, source and target) and 24 F + 16 of moving (the source's copied rows read, the target's written, both
// moments of both zeroed, the new values stored twice).  1 M Gaussians, 5 % dead: 96.8 MB (RGB), 150.8 MB (SH 3).
// Element offsets are 32-bit: a tensor of 2^31 elements or more is REFUSED (MS_ERR_TOO_LARGE).
#include <math.h>

#include "ms_common.hpp"

namespace {

constexpr int kRows = MS_MCMC_ROWS;               // rows (or draws) of a workgroup = its lanes
constexpr int kWaves = kRows / 64;
constexpr int kScanItems = 8;                     // sums per lane and pass of the scan
constexpr int kScanSpan = 64 * kScanItems;        // sums per pass of a wave
constexpr int kMaxRatio = MS_MCMC_MAX_RATIO;      // 51: the binomial table's side
constexpr int64_t kMaxElements = (int64_t)1 << 31;
constexpr uint32_t kNone = 0xFFFFFFFFu;
static_assert(kRows == 256, "a lane per row, four waves");

// the workspace: everything 16-byte aligned
struct Workspace {
    int64_t *cum;          // [N]      weights, then their inclusive scan
    int64_t *block;        // [2][nb]  per-workgroup sums of the weights / numbers of dead rows, then their exclusive scans
    int64_t *info;         // [4]      total weight, dead rows, draws applied
    float4 *values;        // [N]      new stored opacity, new scales
    uint32_t *counts;      // [N]      draws of each source
    uint8_t *flags;        // [N]      1: dead
};

int64_t blocks_of(int64_t N) { return ms::ceil_div(N, kRows); }

size_t carve(int64_t N, void *base, Workspace *w) {
    const size_t nb = (size_t)blocks_of(N);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += ms::align_up(bytes, 16);
        return (char *)base + at;
    };
    char *cum = take((size_t)N * 8), *block = take(2 * nb * 8), *info = take(4 * 8), *values = take((size_t)N * 16),
         *counts = take((size_t)N * 4), *flags = take((size_t)N);
    if (w) *w = {(int64_t *)cum, (int64_t *)block, (int64_t *)info, (float4 *)values, (uint32_t *)counts, (uint8_t *)flags};
    return off;
}

__device__ __forceinline__ int64_t wave_inclusive(int64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

__device__ __forceinline__ float opacity_of(float stored, int logit) {
    return logit ? 1.0f / (1.0f + expf(-stored)) : stored;
}

__global__ void __launch_bounds__(kRows)
k_mcmc_classify(uint32_t N, const float *__restrict__ opacities, int logit, float thr, int64_t *__restrict__ cum,
                uint32_t *__restrict__ counts, uint8_t *__restrict__ flags, int64_t *__restrict__ block, uint32_t nb) {
    __shared__ int64_t wave_w[kWaves];
    __shared__ uint32_t wave_dead[kWaves];
    const uint32_t row = blockIdx.x * (uint32_t)kRows + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t w = 0;
    bool dead = false;
    if (row < N) {
        const float x = opacities[row];
        dead = !(x > thr);                                       // a NaN is dead
        w = dead ? 0 : (int64_t)rintf(opacity_of(x, logit) * 16777216.0f);
        cum[row] = w;
        counts[row] = 0u;
        flags[row] = (uint8_t)dead;
    }
    const int64_t incl = wave_inclusive(w, lane);
    const uint64_t b = __ballot(dead);
    if (lane == 63) wave_w[wave] = incl;
    if (lane == 0) wave_dead[wave] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t sw = 0, sd = 0;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) {
            sw += wave_w[i];
            sd += wave_dead[i];
        }
        block[blockIdx.x] = sw;
        block[nb + blockIdx.x] = sd;
    }
}

// wave `k` scans block[k * nb .. (k + 1) * nb) in place (exclusive); then info = {total, n_dead, n}
__global__ void __launch_bounds__(128)
k_mcmc_scan(int64_t *__restrict__ block, uint32_t nb, int64_t *__restrict__ info, int64_t n_draws, int grow,
            int64_t *__restrict__ n_out) {
    __shared__ int64_t totals[2];
    const int lane = threadIdx.x & 63, kind = threadIdx.x >> 6;
    int64_t *c = block + (size_t)kind * nb;
    int64_t carry = 0;
    for (uint32_t base = 0; base < nb; base += kScanSpan) {
        const uint32_t first = base + lane * kScanItems;
        int64_t v[kScanItems], sum = 0;
#pragma unroll
        for (int j = 0; j < kScanItems; ++j) {
            v[j] = first + j < nb ? c[first + j] : 0;
            sum += v[j];
        }
        const int64_t incl = wave_inclusive(sum, lane);
        int64_t run = carry + incl - sum;
#pragma unroll
        for (int j = 0; j < kScanItems; ++j) {
            if (first + j < nb) c[first + j] = run;
            run += v[j];
        }
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) totals[kind] = carry;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t total = totals[0], n_dead = totals[1];
        const int64_t n = grow ? n_draws : (total > 0 ? (n_dead < n_draws ? n_dead : n_draws) : 0);
        info[0] = total;
        info[1] = n_dead;
        info[2] = n;
        info[3] = 0;
        if (n_out) *n_out = n;
    }
}

__global__ void __launch_bounds__(kRows)
k_mcmc_cumsum(uint32_t N, int64_t *__restrict__ cum, const uint8_t *__restrict__ flags, const int64_t *__restrict__ block,
              uint32_t nb, const int64_t *__restrict__ info, int64_t *__restrict__ targets) {
    __shared__ int64_t wave_w[kWaves];
    __shared__ uint32_t wave_dead[kWaves];
    const uint32_t row = blockIdx.x * (uint32_t)kRows + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool live = row < N;
    const int64_t w = live ? cum[row] : 0;
    const bool dead = live && flags[row];
    const int64_t incl = wave_inclusive(w, lane);
    const uint64_t b = __ballot(dead);
    if (lane == 63) wave_w[wave] = incl;
    if (lane == 0) wave_dead[wave] = __popcll(b);
    __syncthreads();
    int64_t before_w = block[blockIdx.x];
    int64_t rank = block[nb + blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
#pragma unroll
    for (int i = 0; i < kWaves - 1; ++i) {
        before_w += i < wave ? wave_w[i] : 0;
        rank += i < wave ? wave_dead[i] : 0u;
    }
    if (live) cum[row] = before_w + incl;
    if (targets) {                      // relocation: the first n entries are the dead rows, ascending; the rest is -1
        const int64_t n = info[2];
        if (dead && rank < n) targets[rank] = row;
        if (live && row >= n) targets[row] = -1;
    }
}

__global__ void __launch_bounds__(kRows)
k_mcmc_draw(int64_t N, int64_t n_draws, int grow, const int64_t *__restrict__ cum, const uint8_t *__restrict__ flags,
            const int64_t *__restrict__ info, const double *__restrict__ draws, const int64_t *__restrict__ sampled_in,
            int64_t *__restrict__ sampled, int64_t *__restrict__ targets, uint32_t *__restrict__ counts) {
    const int64_t j = (int64_t)blockIdx.x * kRows + threadIdx.x;
    if (j >= n_draws) return;
    const int64_t total = info[0], n = info[2];
    if (grow) targets[j] = N + j;
    int64_t s = -1;
    if (j < n) {
        if (sampled_in) {
            s = sampled_in[j];
            if (s < 0 || s >= N) s = -1;
        } else if (total > 0) {
            int64_t t = (int64_t)floor(draws[j] * (double)total);
            t = t < total - 1 ? t : total - 1;
            int64_t lo = 0, hi = N - 1;             // the first row with cum > t: cum[N - 1] = total > t, so there is one
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (cum[mid] > t) hi = mid; else lo = mid + 1;
            }
            s = lo;
        }
        if (s >= 0 && flags[s]) s = -1;             // a source that is not alive: the draw is not applied
        if (s >= 0) atomicAdd(&counts[s], 1u);
    }
    sampled[j] = s;
}

__global__ void __launch_bounds__(kRows)
k_mcmc_values(uint32_t N, const float *__restrict__ opacities, const float *__restrict__ scales,
              const uint32_t *__restrict__ counts, const float *__restrict__ binom, int logit, double min_opacity,
              float4 *__restrict__ values) {
    const uint32_t row = blockIdx.x * (uint32_t)kRows + threadIdx.x;
    if (row >= N) return;
    const float x = opacities[row];
    float4 out = make_float4(x, scales[3 * row], scales[3 * row + 1], scales[3 * row + 2]);
    const uint32_t c = counts[row];
    if (c > 0u) {
        const int n = c + 1u < (uint32_t)kMaxRatio ? (int)(c + 1u) : kMaxRatio;
        const double o = logit ? 1.0 / (1.0 + exp(-(double)x)) : (double)x;
        const double op = -expm1(log1p(-o) / (double)n);
        const float *k = binom + (size_t)(n - 1) * kMaxRatio;
        double acc = 0.0;
        for (int b = n - 1; b >= 0; --b) acc = acc * op + (double)k[b];
        const double dlog = log(o / (acc * op));
        double oc = op < min_opacity ? min_opacity : op;        // (a NaN stays one, as torch.clamp leaves it)
        oc = oc > 1.0 - 1e-7 ? 1.0 - 1e-7 : oc;
        out = make_float4((float)(logit ? log(oc / (1.0 - oc)) : oc), (float)((double)out.y + dlog),
                          (float)((double)out.z + dlog), (float)((double)out.w + dlog));
    }
    values[row] = out;
}

struct ApplyRec {
    float *base;
    uint32_t width;
    uint32_t kind;          // ms_mcmc_kind | 16 when 16-byte accesses are allowed
};
struct ApplyTable {
    ApplyRec rec[MS_MCMC_MAX_TENSORS];
};
static_assert(sizeof(ApplyRec) == 16, "the table is a kernel argument: keep it small");

__global__ void __launch_bounds__(kRows)
k_mcmc_apply(const ApplyTable tab, int n_tensors, int64_t N, int64_t n_draws, int64_t n_rows, int grow,
             const int64_t *__restrict__ sampled, const int64_t *__restrict__ targets, const float4 *__restrict__ values) {
    __shared__ uint32_t src[kRows], dst[kRows];     // kNone: nothing to do for this draw
    __shared__ uint8_t rewrite[kRows];              // the source takes its new values and loses its moments
    __shared__ int any;
    const int64_t j0 = (int64_t)blockIdx.x * kRows, j = j0 + threadIdx.x;
    if (threadIdx.x == 0) any = 0;
    __syncthreads();
    uint32_t s = kNone, t = kNone;
    bool rw = false;
    if (j < n_draws) {
        const int64_t sj = sampled[j], tj = targets[j];
        if (tj >= 0 && tj < n_rows && sj < N) {
            if (sj >= 0) {
                s = (uint32_t)sj, t = (uint32_t)tj, rw = true;
            } else if (grow) {                       // an appended row nobody was drawn for: a copy of row 0
                s = 0u, t = (uint32_t)tj;
            }
        }
    }
    src[threadIdx.x] = s;
    dst[threadIdx.x] = t;
    rewrite[threadIdx.x] = rw;
    if (t != kNone) any = 1;
    __syncthreads();
    if (!any) return;

    const uint32_t here = n_draws - j0 < (int64_t)kRows ? (uint32_t)(n_draws - j0) : (uint32_t)kRows;
    for (int r = 0; r < n_tensors; ++r) {
        const ApplyRec rec = tab.rec[r];
        const uint32_t kind = rec.kind & 15u;
        if (rec.kind & 16u) {                        // COPY or MOMENT, a vector lies inside one row
            const uint32_t w4 = rec.width >> 2, total = here * w4;
            float4 *base = reinterpret_cast<float4 *>(rec.base);
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            for (uint32_t i = threadIdx.x; i < total; i += kRows) {
                const uint32_t d = i / w4, col = i - d * w4, si = src[d], ti = dst[d];
                if (ti == kNone) continue;
                if (kind == MS_MCMC_MOMENT) {
                    base[(size_t)ti * w4 + col] = zero;
                    if (rewrite[d]) base[(size_t)si * w4 + col] = zero;
                } else {
                    base[(size_t)ti * w4 + col] = base[(size_t)si * w4 + col];
                }
            }
        } else {
            const uint32_t width = rec.width, total = here * width;
            float *base = rec.base;
            for (uint32_t i = threadIdx.x; i < total; i += kRows) {
                const uint32_t d = i / width, col = i - d * width, si = src[d], ti = dst[d];
                if (ti == kNone) continue;
                if (kind == MS_MCMC_COPY) {
                    base[(size_t)ti * width + col] = base[(size_t)si * width + col];
                    continue;
                }
                float v = 0.f;
                if (kind != MS_MCMC_MOMENT) {
                    const float4 nv = values[si];
                    v = kind == MS_MCMC_OPACITY ? nv.x : col == 0 ? nv.y : col == 1 ? nv.z : nv.w;
                }
                base[(size_t)ti * width + col] = v;
                if (rewrite[d]) base[(size_t)si * width + col] = v;
            }
        }
    }
}

__global__ void __launch_bounds__(kRows)
k_mcmc_noise(uint32_t N, float *__restrict__ means3d, const float *__restrict__ scales, const float *__restrict__ quats,
             const float *__restrict__ opacities, const float *__restrict__ noise, int logit, float step, float k, float x0,
             int quats_aligned) {
#pragma clang fp contract(off)
    const uint32_t row = blockIdx.x * (uint32_t)kRows + threadIdx.x;
    if (row >= N) return;
    float qw, qx, qy, qz;
    if (quats_aligned) {
        const float4 q = reinterpret_cast<const float4 *>(quats)[row];
        qw = q.x, qx = q.y, qy = q.z, qz = q.w;
    } else {
        qw = quats[4 * row], qx = quats[4 * row + 1], qy = quats[4 * row + 2], qz = quats[4 * row + 3];
    }
    const float norm = sqrtf(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    const float w = qw / norm, x = qx / norm, y = qy / norm, z = qz / norm;
    const float r00 = 1.f - 2.f * (y * y + z * z), r01 = 2.f * (x * y - w * z), r02 = 2.f * (x * z + w * y);
    const float r10 = 2.f * (x * y + w * z), r11 = 1.f - 2.f * (x * x + z * z), r12 = 2.f * (y * z - w * x);
    const float r20 = 2.f * (x * z - w * y), r21 = 2.f * (y * z + w * x), r22 = 1.f - 2.f * (x * x + y * y);
    const float o = opacity_of(opacities[row], logit);
    const float gate = 1.0f / (1.0f + expf(-k * ((1.0f - o) - x0)));
    const float v0 = (noise[3 * row] * gate) * step, v1 = (noise[3 * row + 1] * gate) * step,
                v2 = (noise[3 * row + 2] * gate) * step;
    // Sigma v = R (exp(2 s) * (R^T v)): no 3x3 covariance is formed, nothing cancels
    const float l0 = expf(2.f * scales[3 * row]) * ((r00 * v0 + r10 * v1) + r20 * v2);
    const float l1 = expf(2.f * scales[3 * row + 1]) * ((r01 * v0 + r11 * v1) + r21 * v2);
    const float l2 = expf(2.f * scales[3 * row + 2]) * ((r02 * v0 + r12 * v1) + r22 * v2);
    means3d[3 * row] += (r00 * l0 + r01 * l1) + r02 * l2;
    means3d[3 * row + 1] += (r10 * l0 + r11 * l1) + r12 * l2;
    means3d[3 * row + 2] += (r20 * l0 + r21 * l1) + r22 * l2;
}

bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" size_t ms_mcmc_workspace_bytes(int64_t N) {
    if (N <= 0) return 0;
    return carve(N, nullptr, nullptr);
}

extern "C" int ms_mcmc_sample(int64_t N, const float *opacities, int logit, float thr, int64_t n_draws, int grow,
                              const double *draws, const int64_t *sampled_in, void *workspace, size_t workspace_bytes,
                              int64_t *sampled, int64_t *targets, int64_t *n_out, void *stream_) {
    MS_REQUIRE(N >= 0 && n_draws >= 0, MS_ERR_INVALID_ARG, "mcmc_sample: negative size (N = %lld, n_draws = %lld)",
               (long long)N, (long long)n_draws);
    MS_REQUIRE(!isnan(thr), MS_ERR_INVALID_ARG, "mcmc_sample: the opacity threshold is NaN");
    MS_REQUIRE(grow || n_draws == N, MS_ERR_INVALID_ARG,
               "mcmc_sample: %lld draws to relocate the dead rows of %lld Gaussians (a relocation takes N)", (long long)n_draws,
               (long long)N);
    if (N == 0 || n_draws == 0) return MS_OK;
    MS_REQUIRE(opacities && workspace && sampled && targets, MS_ERR_INVALID_ARG,
               "mcmc_sample: null pointer (opacities, workspace, sampled or targets)");
    MS_REQUIRE(draws || sampled_in, MS_ERR_INVALID_ARG, "mcmc_sample: null pointer (draws and sampled_in: one is needed)");
    MS_REQUIRE(aligned(opacities, 4) && aligned(draws, 8) && aligned(sampled_in, 8) && aligned(sampled, 8) &&
                   aligned(targets, 8) && aligned(n_out, 8) && aligned(workspace, 16),
               MS_ERR_INVALID_ARG, "mcmc_sample: misaligned pointer (float 4, double and int64 8, workspace 16 bytes)");
    MS_REQUIRE(3 * N < kMaxElements && n_draws < kMaxElements, MS_ERR_TOO_LARGE,
               "mcmc_sample: %lld rows of 3 elements or %lld draws, 2^31 or more (32-bit offsets)", (long long)N,
               (long long)n_draws);
    MS_REQUIRE(workspace_bytes >= ms_mcmc_workspace_bytes(N), MS_ERR_WORKSPACE,
               "mcmc_sample: workspace of %zu bytes, %zu needed", workspace_bytes, ms_mcmc_workspace_bytes(N));
    Workspace w;
    carve(N, workspace, &w);
    const uint32_t nb = (uint32_t)blocks_of(N);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_mcmc_classify, dim3(nb), dim3(kRows), 0, stream, (uint32_t)N, opacities, logit, thr, w.cum,
                       w.counts, w.flags, w.block, nb);
    MS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mcmc_scan, dim3(1), dim3(128), 0, stream, w.block, nb, w.info, n_draws, grow, n_out);
    MS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mcmc_cumsum, dim3(nb), dim3(kRows), 0, stream, (uint32_t)N, w.cum, w.flags, w.block, nb, w.info,
                       grow ? nullptr : targets);
    MS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mcmc_draw, dim3((uint32_t)blocks_of(n_draws)), dim3(kRows), 0, stream, N, n_draws, grow, w.cum,
                       w.flags, w.info, draws, sampled_in, sampled, targets, w.counts);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

extern "C" int ms_mcmc_apply(int64_t N, int64_t n_draws, int64_t n_rows, int grow, void *workspace, size_t workspace_bytes,
                             const int64_t *sampled, const int64_t *targets, int n_tensors, const ms_mcmc_tensor *tensors,
                             const float *opacities, const float *scales, const float *binom, int logit,
                             double min_opacity, void *stream_) {
    MS_REQUIRE(N >= 0 && n_draws >= 0 && n_rows >= 0, MS_ERR_INVALID_ARG,
               "mcmc_apply: negative size (N = %lld, n_draws = %lld, n_rows = %lld)", (long long)N, (long long)n_draws,
               (long long)n_rows);
    MS_REQUIRE(n_rows >= N, MS_ERR_INVALID_ARG, "mcmc_apply: tensors of %lld rows for %lld Gaussians", (long long)n_rows,
               (long long)N);
    MS_REQUIRE(n_tensors >= 0 && n_tensors <= MS_MCMC_MAX_TENSORS, MS_ERR_INVALID_ARG,
               "mcmc_apply: n_tensors = %d, not in [0, %d]", n_tensors, MS_MCMC_MAX_TENSORS);
    if (N == 0 || n_draws == 0) return MS_OK;
    const int value_ptrs = (opacities != nullptr) + (scales != nullptr) + (binom != nullptr);
    MS_REQUIRE(value_ptrs == 0 || value_ptrs == 3, MS_ERR_INVALID_ARG,
               "mcmc_apply: null pointer (opacities, scales and binom go together: all or none)");
    MS_REQUIRE(workspace && sampled && targets, MS_ERR_INVALID_ARG, "mcmc_apply: null pointer (workspace, sampled or targets)");
    MS_REQUIRE(n_tensors == 0 || tensors, MS_ERR_INVALID_ARG, "mcmc_apply: null pointer (tensors)");
    MS_REQUIRE(n_tensors > 0 || value_ptrs, MS_ERR_INVALID_ARG, "mcmc_apply: nothing to do (no tensor and no values to compute)");
    MS_REQUIRE(!value_ptrs || (min_opacity > 0.0 && min_opacity < 1.0), MS_ERR_INVALID_ARG,
               "mcmc_apply: min_opacity = %g, not in (0, 1)", min_opacity);
    MS_REQUIRE(aligned(opacities, 4) && aligned(scales, 4) && aligned(binom, 4) && aligned(sampled, 8) && aligned(targets, 8) &&
                   aligned(workspace, 16),
               MS_ERR_INVALID_ARG, "mcmc_apply: misaligned pointer (float 4, int64 8, workspace 16 bytes)");
    MS_REQUIRE(3 * n_rows < kMaxElements && n_draws < kMaxElements, MS_ERR_TOO_LARGE,
               "mcmc_apply: %lld rows of 3 elements or %lld draws, 2^31 or more (32-bit offsets)", (long long)n_rows,
               (long long)n_draws);
    ApplyTable tab = {};
    for (int i = 0; i < n_tensors; ++i) {
        const ms_mcmc_tensor &t = tensors[i];
        MS_REQUIRE(t.base, MS_ERR_INVALID_ARG, "mcmc_apply: null pointer (tensor %d: base)", i);
        MS_REQUIRE(aligned(t.base, 4), MS_ERR_INVALID_ARG, "mcmc_apply: tensor %d: misaligned pointer (float: 4 bytes)", i);
        MS_REQUIRE(t.width > 0, MS_ERR_INVALID_ARG, "mcmc_apply: tensor %d: non-positive size (width %lld)", i, (long long)t.width);
        MS_REQUIRE(t.kind >= MS_MCMC_COPY && t.kind <= MS_MCMC_MOMENT, MS_ERR_INVALID_ARG,
                   "mcmc_apply: tensor %d: kind %d is none of copy, opacity, scale, moment", i, t.kind);
        MS_REQUIRE(t.width < kMaxElements && n_rows * t.width < kMaxElements, MS_ERR_TOO_LARGE,
                   "mcmc_apply: tensor %d: %lld rows x %lld elements, 2^31 or more (32-bit offsets)", i, (long long)n_rows,
                   (long long)t.width);
        MS_REQUIRE(t.kind != MS_MCMC_OPACITY || t.width == 1, MS_ERR_INVALID_ARG,
                   "mcmc_apply: tensor %d: an opacity tensor of width %lld, not 1", i, (long long)t.width);
        MS_REQUIRE(t.kind != MS_MCMC_SCALE || t.width == 3, MS_ERR_INVALID_ARG,
                   "mcmc_apply: tensor %d: a scale tensor of width %lld, not 3", i, (long long)t.width);
        ApplyRec &r = tab.rec[i];
        r.base = t.base;
        r.width = (uint32_t)t.width;
        r.kind = (uint32_t)t.kind | ((t.width % 4 == 0 && aligned(t.base, 16)) ? 16u : 0u);
    }
    MS_REQUIRE(workspace_bytes >= ms_mcmc_workspace_bytes(N), MS_ERR_WORKSPACE,
               "mcmc_apply: workspace of %zu bytes, %zu needed", workspace_bytes, ms_mcmc_workspace_bytes(N));
    Workspace w;
    carve(N, workspace, &w);
    hipStream_t stream = (hipStream_t)stream_;
    if (value_ptrs) {
        hipLaunchKernelGGL(k_mcmc_values, dim3((uint32_t)blocks_of(N)), dim3(kRows), 0, stream, (uint32_t)N, opacities, scales,
                           w.counts, binom, logit, min_opacity, w.values);
        MS_LAUNCH_CHECK();
    }
    if (n_tensors) {
        hipLaunchKernelGGL(k_mcmc_apply, dim3((uint32_t)blocks_of(n_draws)), dim3(kRows), 0, stream, tab, n_tensors, N, n_draws,
                           n_rows, grow, sampled, targets, w.values);
        MS_LAUNCH_CHECK();
    }
    return MS_OK;
}

extern "C" int ms_mcmc_noise(int64_t N, float *means3d, const float *scales, const float *quats, const float *opacities,
                             const float *noise, int logit, float step, float k, float x0, void *stream_) {
    MS_REQUIRE(N >= 0, MS_ERR_INVALID_ARG, "mcmc_noise: negative size (N = %lld)", (long long)N);
    MS_REQUIRE(!isnan(step) && !isnan(k) && !isnan(x0), MS_ERR_INVALID_ARG, "mcmc_noise: step, k or x0 is NaN");
    if (N == 0) return MS_OK;
    MS_REQUIRE(means3d && scales && quats && opacities && noise, MS_ERR_INVALID_ARG,
               "mcmc_noise: null pointer (means3d, scales, quats, opacities or noise)");
    MS_REQUIRE(aligned(means3d, 4) && aligned(scales, 4) && aligned(quats, 4) && aligned(opacities, 4) && aligned(noise, 4),
               MS_ERR_INVALID_ARG, "mcmc_noise: misaligned pointer (float: 4 bytes)");
    MS_REQUIRE(4 * N < kMaxElements, MS_ERR_TOO_LARGE, "mcmc_noise: %lld x 4 elements, 2^31 or more (32-bit offsets)", (long long)N);
    hipLaunchKernelGGL(k_mcmc_noise, dim3((uint32_t)blocks_of(N)), dim3(kRows), 0, (hipStream_t)stream_, (uint32_t)N, means3d,
                       scales, quats, opacities, noise, logit, step, k, x0, (int)aligned(quats, 16));
    MS_LAUNCH_CHECK();
    return MS_OK;
}
