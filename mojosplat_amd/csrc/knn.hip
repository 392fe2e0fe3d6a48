// Exact k nearest neighbours of every point of a cloud (k <= 8, three dimensions): the squared distances that set a scene's
// initial scales (3DGS create_from_pcd; the CUDA stack's simple-knn, distCUDA2), restated for 64-wide waves.
// mojosplat_amd/knn.py holds the definition (knn_torch); nothing in the reference does this (it has no training).
//
// The caller hands a permutation `order` that makes the points spatially coherent (a Morton order; any permutation gives the
// same bits, a coherent one is fast).  Two launches, no atomics, no host wait:
// k_knn_gather   a wave per block of kBlock (64) consecutive points of the sorted order: sorted[pos] = (x, y, z, original row)
//                and the block's min/max box by a butterfly of exact min / max.
// k_knn_search   a wave per block, a query per lane, the k best so far in registers as (d, original row), ascending in (d, row).
//                SEED: the wave's own block and the two next to it in sorted order, every point of them (they hold the +-k
//                neighbours of every query of the block, and at least k other points whenever N > k).
//                WALK: the other blocks, 64 at a time (a lane per box), outward from the wave's own position.  A box is first
//                tested against the wave's box and the largest k-th best of its lanes, then by every lane against its own
//                query and k-th best; it is visited when one lane cannot skip it.  A visited block's points are loaded once
//                by the wave (one coalesced 16-byte load per lane) and handed round by v_readlane.  Every block is visited
//                at most once by a wave and seed and walk visit disjoint blocks: no candidate is offered twice.
//
// THE BOUND.  d(p, q) = ((dx dx) + (dy dy)) + (dz dz), every operation rounded to float32 on its own.  The distance to a box is
// the same expression over the per-axis gaps max(lo - p, p - hi, 0): for a point q inside the box |p - q| >= gap holds per axis
// in the reals, rounding is monotone, and so are the square of a non-negative number and the sums: box <= d(p, q) IN FLOAT32 for
// every q of the box.  The gap between two boxes bounds the gap of a point of the first to the second from below the same way.
// A box is skipped only when box > k-th best, STRICTLY: at equality a candidate with a smaller row still displaces the k-th.
// Self is the candidate with the query's own original row; equal points are neighbours at distance 0.
#include <math.h>

#include "ms_common.hpp"

namespace {

constexpr int kBlock = MS_KNN_BLOCK;              // points of a block = queries of a wave
constexpr int kWaves = 4;                         // waves (independent of each other) of a workgroup
constexpr uint32_t kNoRow = 0xFFFFFFFFu;
static_assert(kBlock == 64, "a block is a wave: a query per lane, a box per lane of the walk");

struct Workspace {
    float4 *sorted;        // [N]      x, y, z, the original row's bits
    float4 *boxes;         // [2 nb]   lo, hi of every block (w unused)
};

int64_t blocks_of(int64_t N) { return ms::ceil_div(N, kBlock); }

size_t carve(int64_t N, void *base, Workspace *w) {
    const size_t sorted_bytes = ms::align_up((size_t)N * 16, 16), box_bytes = (size_t)blocks_of(N) * 32;
    if (w) *w = {(float4 *)base, (float4 *)((char *)base + sorted_bytes)};
    return sorted_bytes + box_bytes;
}

__device__ __forceinline__ float dist2_of(float px, float py, float pz, float qx, float qy, float qz) {
#pragma clang fp contract(off)
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// a point against a box: a lower bound, in float32, of dist2_of(p, q) for every q inside the box
__device__ __forceinline__ float box_dist2(float px, float py, float pz, const float4 lo, const float4 hi) {
#pragma clang fp contract(off)
    const float ax = fmaxf(fmaxf(lo.x - px, px - hi.x), 0.f);
    const float ay = fmaxf(fmaxf(lo.y - py, py - hi.y), 0.f);
    const float az = fmaxf(fmaxf(lo.z - pz, pz - hi.z), 0.f);
    return ((ax * ax) + (ay * ay)) + (az * az);
}

// box a against box b: a lower bound of box_dist2(p, b) for every p inside a
__device__ __forceinline__ float box_box_dist2(const float4 alo, const float4 ahi, const float4 blo, const float4 bhi) {
#pragma clang fp contract(off)
    const float ax = fmaxf(fmaxf(blo.x - ahi.x, alo.x - bhi.x), 0.f);
    const float ay = fmaxf(fmaxf(blo.y - ahi.y, alo.y - bhi.y), 0.f);
    const float az = fmaxf(fmaxf(blo.z - ahi.z, alo.z - bhi.z), 0.f);
    return ((ax * ax) + (ay * ay)) + (az * az);
}

__device__ __forceinline__ float lane_value(float v, int lane) {      // `lane` is the same in every lane
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

__global__ void __launch_bounds__(kWaves * 64)
k_knn_gather(uint32_t N, uint32_t nb, const float *__restrict__ points, const int32_t *__restrict__ order,
             float4 *__restrict__ sorted, float4 *__restrict__ boxes) {
    const int lane = threadIdx.x & 63;
    const uint32_t b = blockIdx.x * (uint32_t)kWaves + (threadIdx.x >> 6);
    if (b >= nb) return;                                     // (the whole wave: nothing below crosses waves)
    const uint32_t pos = b * (uint32_t)kBlock + lane;
    const float inf = __builtin_huge_valf();
    float lx = inf, ly = inf, lz = inf, hx = -inf, hy = -inf, hz = -inf;
    if (pos < N) {
        uint32_t row = order ? (uint32_t)order[pos] : pos;
        if (row >= N) row = pos;                             // not a permutation: wrong results, but no access out of bounds
        const float x = points[3 * (size_t)row], y = points[3 * (size_t)row + 1], z = points[3 * (size_t)row + 2];
        sorted[pos] = make_float4(x, y, z, __uint_as_float(row));
        lx = hx = x, ly = hy = y, lz = hz = z;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        lx = fminf(lx, __shfl_xor(lx, d, 64)), ly = fminf(ly, __shfl_xor(ly, d, 64)), lz = fminf(lz, __shfl_xor(lz, d, 64));
        hx = fmaxf(hx, __shfl_xor(hx, d, 64)), hy = fmaxf(hy, __shfl_xor(hy, d, 64)), hz = fmaxf(hz, __shfl_xor(hz, d, 64));
    }
    if (lane == 0) {
        boxes[2 * (size_t)b] = make_float4(lx, ly, lz, 0.f);
        boxes[2 * (size_t)b + 1] = make_float4(hx, hy, hz, 0.f);
    }
}

// the k best of a query, ascending in (d, row)
template <int K>
struct Best {
    float d[K];
    uint32_t r[K];
};

template <int K>
__device__ __forceinline__ void offer(Best<K> &best, float d, uint32_t r) {
    if (d < best.d[K - 1] || (d == best.d[K - 1] && r < best.r[K - 1])) {
        best.d[K - 1] = d;
        best.r[K - 1] = r;
#pragma unroll
        for (int i = K - 1; i > 0; --i) {
            const float da = best.d[i - 1], db = best.d[i];
            const uint32_t ra = best.r[i - 1], rb = best.r[i];
            const bool up = db < da || (db == da && rb < ra);
            best.d[i - 1] = up ? db : da, best.d[i] = up ? da : db;
            best.r[i - 1] = up ? rb : ra, best.r[i] = up ? ra : rb;
        }
    }
}

// every point of block `bb` is offered to every query of the wave (a point that a lane could have skipped is a candidate
// like any other)
template <int K>
__device__ __forceinline__ void visit(Best<K> &best, bool active, float px, float py, float pz, uint32_t my_row,
                                      const float4 *__restrict__ sorted, uint32_t N, uint32_t bb, int lane) {
    const uint32_t first = bb * (uint32_t)kBlock, left = N - first, count = left < (uint32_t)kBlock ? left : (uint32_t)kBlock;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((uint32_t)lane < count) c = sorted[first + lane];
    for (uint32_t t = 0; t < count; ++t) {
        const float qx = lane_value(c.x, (int)t), qy = lane_value(c.y, (int)t), qz = lane_value(c.z, (int)t);
        const uint32_t r = __float_as_uint(lane_value(c.w, (int)t));
        const float d = dist2_of(px, py, pz, qx, qy, qz);
        if (active && r != my_row) offer(best, d, r);
    }
}

// the largest k-th best of the wave's queries (a lane without a query: below every distance)
template <int K>
__device__ __forceinline__ float wave_kth(const Best<K> &best, bool active) {
    float v = active ? best.d[K - 1] : -1.f;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}

template <int K>
__global__ void __launch_bounds__(kWaves * 64)
k_knn_search(uint32_t N, uint32_t nb, const float4 *__restrict__ sorted, const float4 *__restrict__ boxes,
             float *__restrict__ dist2, int64_t *__restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const uint32_t w = blockIdx.x * (uint32_t)kWaves + (threadIdx.x >> 6);
    if (w >= nb) return;                                     // (the whole wave)
    const uint32_t pos = w * (uint32_t)kBlock + lane;
    const bool active = pos < N;
    float px = 0.f, py = 0.f, pz = 0.f;
    uint32_t my_row = kNoRow;
    if (active) {
        const float4 me = sorted[pos];
        px = me.x, py = me.y, pz = me.z, my_row = __float_as_uint(me.w);
    }
    Best<K> best;
#pragma unroll
    for (int i = 0; i < K; ++i) best.d[i] = __builtin_huge_valf(), best.r[i] = kNoRow;

    // seed: the own block and its neighbours in sorted order
    const uint32_t seed_lo = w > 0u ? w - 1u : 0u, seed_hi = w + 1u < nb ? w + 1u : nb - 1u;
    for (uint32_t bb = seed_lo; bb <= seed_hi; ++bb) visit<K>(best, active, px, py, pz, my_row, sorted, N, bb, lane);
    float wmax = wave_kth<K>(best, active);

    // walk: the chunks of 64 boxes, c0, c0 + 1, c0 - 1, c0 + 2, ...
    const float4 wlo = boxes[2 * (size_t)w], whi = boxes[2 * (size_t)w + 1];
    const uint32_t n_chunks = (nb + 63u) >> 6, c0 = w >> 6;
    for (uint32_t step = 0; step < 2u * n_chunks; ++step) {
        const uint32_t off = (step + 1u) >> 1;
        if (step & 1u ? c0 + off >= n_chunks : off > c0) continue;
        const uint32_t c = step & 1u ? c0 + off : c0 - off;
        const uint32_t b = (c << 6) + lane;
        bool open = b < nb && (b + 1u < w || b > w + 1u);    // (the seed's blocks are done)
        if (open) open = !(box_box_dist2(wlo, whi, boxes[2 * (size_t)b], boxes[2 * (size_t)b + 1]) > wmax);
        uint64_t mask = __ballot(open);
        while (mask) {
            const uint32_t bb = (c << 6) + (uint32_t)__builtin_ctzll(mask);
            mask &= mask - 1ull;
            const bool need = active && !(box_dist2(px, py, pz, boxes[2 * (size_t)bb], boxes[2 * (size_t)bb + 1]) > best.d[K - 1]);
            if (__ballot(need) == 0ull) continue;
            visit<K>(best, active, px, py, pz, my_row, sorted, N, bb, lane);
            wmax = wave_kth<K>(best, active);
        }
    }

    if (active) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            dist2[(size_t)my_row * K + i] = best.d[i];
            if (idx) idx[(size_t)my_row * K + i] = (int64_t)best.r[i];
        }
    }
}

template <int K>
void launch_search(uint32_t N, uint32_t nb, const Workspace &w, float *dist2, int64_t *idx, hipStream_t stream) {
    hipLaunchKernelGGL(k_knn_search<K>, dim3((nb + kWaves - 1) / kWaves), dim3(kWaves * 64), 0, stream, N, nb, w.sorted, w.boxes,
                       dist2, idx);
}

bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" size_t ms_knn_workspace_bytes(int64_t N, int k) {
    if (N <= 0 || N >= ((int64_t)1 << 31) || k < 1 || k > MS_KNN_MAX_K) return 0;
    return carve(N, nullptr, nullptr);
}

extern "C" int ms_knn(int64_t N, const float *points, const int32_t *order, int k, float *dist2, int64_t *idx, void *workspace,
                      void *stream_) {
    MS_REQUIRE(k >= 1 && k <= MS_KNN_MAX_K, MS_ERR_INVALID_ARG, "knn: k = %d, not in [1, %d]", k, MS_KNN_MAX_K);
    MS_REQUIRE(N > k, MS_ERR_INVALID_ARG, "knn: %lld points have no %d neighbours each (N >= k + 1)", (long long)N, k);
    MS_REQUIRE(N < ((int64_t)1 << 31), MS_ERR_TOO_LARGE, "knn: %lld points, 2^31 or more (32-bit rows)", (long long)N);
    MS_REQUIRE(points && dist2 && workspace, MS_ERR_INVALID_ARG, "knn: null pointer (points, dist2 or workspace)");
    MS_REQUIRE(aligned(points, 4) && aligned(order, 4) && aligned(dist2, 4) && aligned(idx, 8) && aligned(workspace, 16),
               MS_ERR_INVALID_ARG, "knn: misaligned pointer (float and int32 4, int64 8, workspace 16 bytes)");
    Workspace w;
    carve(N, workspace, &w);
    const uint32_t nb = (uint32_t)blocks_of(N);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_knn_gather, dim3((nb + kWaves - 1) / kWaves), dim3(kWaves * 64), 0, stream, (uint32_t)N, nb, points, order,
                       w.sorted, w.boxes);
    MS_LAUNCH_CHECK();
    switch (k) {
        case 1: launch_search<1>((uint32_t)N, nb, w, dist2, idx, stream); break;
        case 2: launch_search<2>((uint32_t)N, nb, w, dist2, idx, stream); break;
        case 3: launch_search<3>((uint32_t)N, nb, w, dist2, idx, stream); break;
        case 4: launch_search<4>((uint32_t)N, nb, w, dist2, idx, stream); break;
        case 5: launch_search<5>((uint32_t)N, nb, w, dist2, idx, stream); break;
        case 6: launch_search<6>((uint32_t)N, nb, w, dist2, idx, stream); break;
        case 7: launch_search<7>((uint32_t)N, nb, w, dist2, idx, stream); break;
        default: launch_search<8>((uint32_t)N, nb, w, dist2, idx, stream); break;
    }
    MS_LAUNCH_CHECK();
    return MS_OK;
}
