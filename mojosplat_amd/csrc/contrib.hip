// Per-Gaussian contribution statistics of one view (the definition: mojosplat_amd/contrib.py, contributions_from_lists_torch).
// A rasteriser-shaped kernel beside the frame path: every pixel walks its tile's sorted list front to back with the
// compositor's own rules (ms_common.hpp: kAlphaThreshold, kMaxAlpha, kTransmittanceStop), and instead of blending colours
// the kernel reduces, per list entry, the blend weights w = alpha T of the pixels that blended it: their number, their
// maximum, their sum and their sum under a per-pixel weight map.
//
// Shape: one workgroup of four waves per 16x16 pixel block (a 32-px tile is four blocks that walk the same list), a wave
// per four pixel rows.  List entries are staged 64 at a time (id, mean, conic, opacity); every wave ballots which of them can
// reach its pixel rows at all (can_reach) and walks only those.  The reduction over a wave's 64
// pixels goes through a wave-private LDS image, 32 entries at a time: lane p stores its w of entry r at [r][p] (one
// conflict-free ds_write_b32 per entry), then lane l sums row l & 31 over the pixels 32 (l >> 5) .. + 31 in pixel order with
// eight ds_read_b128 (row stride 68 floats: the sixteen lanes of a ds_read_b128 group sit on sixteen different slots), and
// one cross-lane move per quantity adds the upper half to the lower.  Per (entry, wave) that is about 4 vector
// instructions, half a ds_read_b128 and one ds_write_b32, against 18 DPP additions plus a ballot for a shuffle tree over
// three float quantities.  The four waves' partials meet in LDS, are added in wave order, rounded to
// fixed point and leave as integer atomics, one quantity per wave: everything is summed in a fixed order, so a run is
// bitwise reproducible.  No float atomics; nothing is written for a (block, entry) that blended no pixel.
#include "ms_common.hpp"

namespace {

constexpr int kBlock = 16;                  // pixels per side of a workgroup's block
constexpr int kThreads = kBlock * kBlock;   // 256: four waves
constexpr int kWaves = kThreads / 64;
constexpr int kBatch = 64;                  // list entries staged at a time
constexpr int kSub = 32;                    // ... reduced at a time
constexpr int kStride = 68;                 // floats per row of a wave's image: 64 pixels + one 16-byte slot
constexpr float kFixedOne = 0x1p30f;        // MS_CONTRIB_FIXED_ONE

struct ContribArgs {
    int64_t N, M;
    const float2 *means2d;
    const float *conics;
    const float *opacities;
    const int2 *tile_ranges;
    const int32_t *ids;
    const float *weights;
    int W, H, per_side, tw;                 // per_side: blocks per side of a tile (1 or 2)
    unsigned long long *pixels;
    unsigned int *max_weight;
    unsigned long long *sum_q, *wsum_q;
};

// (the LDS executes one wave's instructions in order; the compiler must keep a lane's load below another lane's store)
__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// Can the entry blend any pixel centre of the rectangle [xl, xl + 15] x [yl, yl + 3]?  alpha >= 1/255 needs
// sigma <= log(255 o).  With a, c > 0 and the mean outside the rectangle, the least sigma over it lies on one of its four
// edges, where sigma is a parabola of positive curvature in one variable: the form itself is evaluated at each edge's clamped
// minimiser, with the walk's own expression -- no determinant, whose float32 value cancels for long thin rotated Gaussians.
// The walk's float32 sigma at a pixel, and the value here, each differ from the exact one by a few 2^-24 S, with
// S <= 0.5 (a DX^2 + c DY^2) + |b| DX DY the sum of the magnitudes of the form's terms (DX, DY: the largest |dx|, |dy| over the
// rectangle); the margin is 2e-6 S (over thirty 2^-24 S) plus 1e-2 + 1e-3 |log(255 o)| for the exponential and the logarithm.
// So an entry that is left out is one the walk skips at every pixel; anything undecidable (a or c <= 0, b^2 clearly above a c, a NaN) is walked.
__device__ __forceinline__ bool can_reach(const float4 a, const float2 b, const float xl, const float yl) {
    const float ca = a.z, cb = a.w, cc = b.x;
    const float dx0 = a.x - (xl + 15.0f), dx1 = a.x - xl, dy0 = a.y - (yl + 3.0f), dy1 = a.y - yl;   // dx = mean - pixel
    if (!(ca > 0.0f && cc > 0.0f && cb * cb <= 1.001f * (ca * cc))) return true;   // (not a positive form: no bound)
    if (dx0 <= 0.0f && dx1 >= 0.0f && dy0 <= 0.0f && dy1 >= 0.0f) return true;                       // the mean is inside
    auto sigma = [&](float dx, float dy) { return 0.5f * (ca * dx * dx + cc * dy * dy) + cb * dx * dy; };
    auto along_y = [&](float dx) { return sigma(dx, fminf(fmaxf(-cb * dx / cc, dy0), dy1)); };
    auto along_x = [&](float dy) { return sigma(fminf(fmaxf(-cb * dy / ca, dx0), dx1), dy); };
    const float least = fminf(fminf(along_y(dx0), along_y(dx1)), fminf(along_x(dy0), along_x(dy1)));
    const float DX = fmaxf(fabsf(dx0), fabsf(dx1)), DY = fmaxf(fabsf(dy0), fabsf(dy1));
    const float S = 0.5f * (ca * DX * DX + cc * DY * DY) + fabsf(cb) * DX * DY;
    const float lim = __logf(255.0f * b.y);
    return !(least > lim + 1e-3f * fabsf(lim) + 1e-2f + 2e-6f * S);
}

template <bool HAS_W>
__global__ void __launch_bounds__(kThreads) k_contrib(const ContribArgs A) {
    __shared__ __attribute__((aligned(16))) float s_img[kWaves][kSub * kStride];
    __shared__ float s_part[2][4][kWaves][kBatch];     // [batch parity][count, max, sum, weighted sum][wave][entry]
    __shared__ float4 s_a[kBatch];                     // mean.x, mean.y, conic a, conic b
    __shared__ float2 s_b[kBatch];                     // conic c, opacity
    __shared__ int32_t s_id[2][kBatch];
    __shared__ __attribute__((aligned(16))) float s_w[kThreads];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int per_tile = A.per_side * A.per_side;
    const int tile = blockIdx.x / per_tile, quad = blockIdx.x - tile * per_tile;
    const int ty = tile / A.tw, tx = tile - ty * A.tw;
    const int x0 = (tx * A.per_side + quad % A.per_side) * kBlock, y0 = (ty * A.per_side + quad / A.per_side) * kBlock;
    if (x0 >= A.W || y0 >= A.H) return;
    const int2 range = A.tile_ranges[tile];
    const int64_t begin = range.x > 0 ? range.x : 0, end = range.y < A.M ? range.y : A.M;
    if (end <= begin) return;

    const int x = x0 + (lane & 15), y = y0 + wave * 4 + (lane >> 4);
    const bool inside = x < A.W && y < A.H;
    if (HAS_W) {
        const float v = inside ? A.weights[(int64_t)y * A.W + x] : 0.0f;
        s_w[tid] = v > 0.0f ? fminf(v, 1.0f) : 0.0f;   // clamped to [0, 1]; NaN counts as 0
    }
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    float T = 1.0f;
    bool done = !inside;
    float *img = s_img[wave];

    for (int it = 0;; ++it) {
        const int64_t base = begin + (int64_t)it * kBatch;
        const int n = (int)(end - base < kBatch ? end - base : kBatch);
        const int par = it & 1;
        if (tid < kBatch) {
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float2 b = make_float2(0.0f, 0.0f);
            int32_t g = -1;
            if (tid < n) {
                g = A.ids[base + tid];
                if ((int64_t)(uint32_t)g < A.N) {
                    const float2 m = A.means2d[g];
                    const float *c = A.conics + (int64_t)g * 3;
                    a = make_float4(m.x, m.y, c[0], c[1]);
                    b = make_float2(c[2], A.opacities[g]);
                } else {
                    g = -1;                            // not a row of the scene: blends nothing
                }
            }
            s_a[tid] = a;
            s_b[tid] = b;
            s_id[par][tid] = g;
        }
        __syncthreads();
        // lane j: can staged entry j reach this wave's 16 x 4 pixels at all?  Only those are walked.
        const unsigned long long reach =
            __ballot(s_id[par][lane] >= 0 && can_reach(s_a[lane], s_b[lane], (float)x0 + 0.5f, (float)(y0 + 4 * wave) + 0.5f));

        for (int sub = 0; sub < kBatch / kSub; ++sub) {
            const int first = sub * kSub;
            uint32_t todo = __builtin_amdgcn_readfirstlane((uint32_t)(reach >> first));
            uint32_t walked = 0;                                    // bit r: row r of the image was written
            if (todo && __ballot(!done) != 0ull) {
                int e = __builtin_ctz(todo);
                float4 a = s_a[first + e];
                float2 b = s_b[first + e];
                for (;;) {
                    todo &= todo - 1;
                    const int en = todo ? __builtin_ctz(todo) : e;
                    const float4 an = s_a[first + en];              // the next entry's record, while this one is evaluated
                    const float2 bn = s_b[first + en];
                    const float dx = a.x - px, dy = a.y - py;
                    const float sigma = 0.5f * (a.z * dx * dx + b.x * dy * dy) + a.w * dx * dy;
                    const float alpha = fminf(ms::kMaxAlpha, b.y * __expf(-sigma));
                    const bool valid = !done && sigma >= 0.0f && alpha >= ms::kAlphaThreshold;
                    const float next = T * (1.0f - alpha);
                    const bool stop = valid && next <= ms::kTransmittanceStop;   // stops BEFORE adding the entry
                    const bool blend = valid && !stop;
                    img[e * kStride + lane] = blend ? alpha * T : 0.0f;
                    T = blend ? next : T;
                    done = done || stop;
                    walked |= 1u << e;
                    if (!todo || __ballot(!done) == 0ull) break;
                    e = en;
                    a = an;
                    b = bn;
                }
            }
            wave_lds_sync();
            // lane l: entry first + (l & 31), pixels 32 (l >> 5) .. + 31 of this wave, in pixel order
            const int r = lane & 31, half = lane >> 5;
            float cnt = 0.0f, mx = 0.0f, sum = 0.0f, wsum = 0.0f;
            if ((walked >> r) & 1u) {
                const float4 *row = reinterpret_cast<const float4 *>(img + r * kStride + half * 32);
                const float4 *wt = reinterpret_cast<const float4 *>(s_w + wave * 64 + half * 32);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float4 v = row[k];
                    cnt += (v.x > 0.0f ? 1.0f : 0.0f) + (v.y > 0.0f ? 1.0f : 0.0f) + (v.z > 0.0f ? 1.0f : 0.0f) +
                           (v.w > 0.0f ? 1.0f : 0.0f);
                    mx = fmaxf(fmaxf(fmaxf(mx, v.x), fmaxf(v.y, v.z)), v.w);
                    sum = (((sum + v.x) + v.y) + v.z) + v.w;
                    if (HAS_W) {
                        const float4 u = wt[k];
                        wsum = (((wsum + v.x * u.x) + v.y * u.y) + v.z * u.z) + v.w * u.w;
                    }
                }
            }
            // the upper half's partial behind the lower half's; the lower lanes hold the wave's values
            cnt += __shfl_xor(cnt, 32);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float sum_o = __shfl_xor(sum, 32);
            sum = half ? sum_o + sum : sum + sum_o;
            if (HAS_W) {
                const float wsum_o = __shfl_xor(wsum, 32);
                wsum = half ? wsum_o + wsum : wsum + wsum_o;
            }
            if (half == 0) {
                s_part[par][0][wave][first + r] = cnt;
                s_part[par][1][wave][first + r] = mx;
                s_part[par][2][wave][first + r] = sum;
                if (HAS_W) s_part[par][3][wave][first + r] = wsum;
            }
            wave_lds_sync();                            // the image is rewritten by the next 32 entries
        }
        const int all_done = __syncthreads_and(__ballot(!done) == 0ull);

        // wave q sends quantity q of entry `lane`: the four waves' partials in wave order
        if (lane < n) {
            const int32_t g = s_id[par][lane];
            float cnt = 0.0f;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) cnt += s_part[par][0][w][lane];
            if (cnt > 0.0f && g >= 0) {
                const float *p = &s_part[par][wave][0][lane];
                if (wave == 0) {
                    atomicAdd(A.pixels + g, (unsigned long long)cnt);
                } else if (wave == 1) {
                    float m = 0.0f;
#pragma unroll
                    for (int w = 0; w < kWaves; ++w) m = fmaxf(m, p[w * kBatch]);
                    atomicMax(A.max_weight + g, __float_as_uint(m));
                } else if (wave == 2 || HAS_W) {
                    float s = 0.0f;
#pragma unroll
                    for (int w = 0; w < kWaves; ++w) s += p[w * kBatch];
                    atomicAdd((wave == 2 ? A.sum_q : A.wsum_q) + g, (unsigned long long)__float2ll_rn(s * kFixedOne));
                }
            }
        }
        if (all_done || base + kBatch >= end) break;
    }
}

}  // namespace

extern "C" int ms_contrib_accumulate(int64_t N, int64_t M, const float *means2d, const float *conics, const float *opacities,
                                     const int32_t *tile_ranges, const int32_t *flatten_ids, const float *weights, int W, int H,
                                     int tile_size, int64_t *pixels, float *max_weight, int64_t *sum_q, int64_t *wsum_q,
                                     void *stream) {
    MS_REQUIRE(N >= 0 && M >= 0, MS_ERR_INVALID_ARG, "contrib_accumulate: N = %lld, M = %lld", (long long)N, (long long)M);
    MS_REQUIRE(W > 0 && H > 0, MS_ERR_INVALID_ARG, "contrib_accumulate: image %d x %d", W, H);
    MS_REQUIRE(tile_size == 16 || tile_size == 32, MS_ERR_INVALID_ARG, "contrib_accumulate: tile_size = %d, not 16 or 32",
               tile_size);
    MS_REQUIRE(N <= 0x7FFFFFFFll && M <= 0x7FFFFFFFll, MS_ERR_TOO_LARGE,
               "contrib_accumulate: N = %lld, M = %lld do not fit int32 indices", (long long)N, (long long)M);
    if (N == 0 || M == 0) return MS_OK;
    MS_REQUIRE(means2d && conics && opacities && tile_ranges && flatten_ids && pixels && max_weight && sum_q,
               MS_ERR_INVALID_ARG, "contrib_accumulate: null pointer");
    MS_REQUIRE(!weights || wsum_q, MS_ERR_INVALID_ARG, "contrib_accumulate: weights without wsum_q");
    MS_REQUIRE(((uintptr_t)means2d & 7) == 0 && ((uintptr_t)tile_ranges & 7) == 0 && ((uintptr_t)pixels & 7) == 0 &&
                   ((uintptr_t)sum_q & 7) == 0 && ((uintptr_t)wsum_q & 7) == 0,
               MS_ERR_INVALID_ARG, "contrib_accumulate: misaligned pointer (means2d, tile_ranges, int64 buffers: 8 bytes)");
    const int64_t tw = ms::ceil_div(W, tile_size), th = ms::ceil_div(H, tile_size);
    const int per_side = tile_size / kBlock;
    const int64_t blocks = tw * th * per_side * per_side;
    MS_REQUIRE(blocks <= 0x7FFFFFFFll, MS_ERR_TOO_LARGE, "contrib_accumulate: %lld pixel blocks, more than a launch has workgroups for",
               (long long)blocks);
    ContribArgs A;
    A.N = N;
    A.M = M;
    A.means2d = reinterpret_cast<const float2 *>(means2d);
    A.conics = conics;
    A.opacities = opacities;
    A.tile_ranges = reinterpret_cast<const int2 *>(tile_ranges);
    A.ids = flatten_ids;
    A.weights = weights;
    A.W = W;
    A.H = H;
    A.per_side = per_side;
    A.tw = (int)tw;
    A.pixels = reinterpret_cast<unsigned long long *>(pixels);
    A.max_weight = reinterpret_cast<unsigned int *>(max_weight);
    A.sum_q = reinterpret_cast<unsigned long long *>(sum_q);
    A.wsum_q = reinterpret_cast<unsigned long long *>(wsum_q);
    hipStream_t s = (hipStream_t)stream;
    if (weights)
        hipLaunchKernelGGL(k_contrib<true>, dim3((uint32_t)blocks), dim3(kThreads), 0, s, A);
    else
        hipLaunchKernelGGL(k_contrib<false>, dim3((uint32_t)blocks), dim3(kThreads), 0, s, A);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
