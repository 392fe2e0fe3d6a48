// Scene editing: the similarity transform x' = s R x + t of a whole scene (mojosplat_amd/edit.py holds the derivation of the
// constants and the definition, transform_scene with backend="torch"; nothing in the reference does this: it edits no scene).
// One kernel, k_scene_transform<K>, one launch, no atomics, no workspace, no host wait.
//
// What is here is a separately rounded float32 multiply or add per operation of the definition, in its order, with contraction
// off (the assembly holds no fused multiply-add), nothing skipped for a zero matrix entry, denormals kept: the bits are the
// definition's.  The only operations are multiply and add -- the quaternion product's a - b c is a + (-b) c with the negated
// constants handed in beside the transform, so the compiler cannot turn the pair into a subtraction whose NaN might differ in
// sign from the definition's.
//
// K > 1: a workgroup owns kRows (64) consecutive Gaussians.  Their feature rows are one contiguous span of 64 * 3 K floats that
// starts on a multiple of 256 bytes from the array's base, so it is moved by coalesced 16-byte accesses whenever the base is
// 16-byte aligned (dwords otherwise, and for the last < 4 floats of the last workgroup).
//   STAGE   the span goes to LDS, row r at r * S: S = 3 K | 1 is odd, so the 64 lanes of a wave that read or write one
//           coefficient of 64 consecutive rows touch 64 different addresses modulo any power of two -- no bank conflict.
//   ROTATE  wave c < 3 takes channel c, lane g Gaussian g: the lane reads band l's 2 l + 1 coefficients of its (Gaussian,
//           channel), forms the 2 l + 1 products with M_l from the by-value transform (scalar registers), and writes them back
//           over the ones it read -- nobody else touches those words.  Band 0 stays as staged.
//           Wave 3 meanwhile moves the 64 Gaussians' means, log-scales and quaternions from global to global.
//   EMIT    the span goes back out as it came in.
// K = 1 (and (N, 3) RGB): nothing to rotate.  A workgroup owns 256 Gaussians, a lane moves one Gaussian's geometry, and the
// features' span is copied 16 bytes a lane.
// Every global element index is 64-bit (size_t).  Within a workgroup an index is below 64 * 76 and stays 32-bit.
#include "ms_common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kRows = MS_TRANSFORM_ROWS;
constexpr int kRowsK1 = MS_TRANSFORM_ROWS_K1;
constexpr int kThreads = 256;
static_assert(kRows == 64 && kThreads == 4 * kRows, "three waves rotate a channel each, the fourth moves the geometry");
static_assert(kRowsK1 == kThreads, "K = 1: a lane per Gaussian");
static_assert(kRows % 4 == 0 && kRowsK1 % 4 == 0, "a workgroup's span of rows of any width starts on a multiple of 16 bytes");

struct Geometry {
    const float *means, *scales, *quats;
    float *out_means, *out_scales, *out_quats;
};
struct NegQuat {                                   // -r.x, -r.y, -r.z of the transform's quaternion (the host negates: exact)
    float x, y, z;
};

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ void move_geometry(const ms_transform &xf, const NegQuat &nr, const Geometry &g, size_t row) {
    const float x = g.means[3 * row], y = g.means[3 * row + 1], z = g.means[3 * row + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        g.out_means[3 * row + i] = ((xf.A[3 * i] * x + xf.A[3 * i + 1] * y) + xf.A[3 * i + 2] * z) + xf.t[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) g.out_scales[3 * row + i] = g.scales[3 * row + i] + xf.l;
    float4 q;
    if (aligned16(g.quats)) {
        q = ((const float4 *)g.quats)[row];
    } else {
        q = make_float4(g.quats[4 * row], g.quats[4 * row + 1], g.quats[4 * row + 2], g.quats[4 * row + 3]);
    }
    const float rw = xf.r[0], rx = xf.r[1], ry = xf.r[2], rz = xf.r[3];
    const float qw = q.x, qx = q.y, qy = q.z, qz = q.w;
    float4 o;
    o.x = ((rw * qw + nr.x * qx) + nr.y * qy) + nr.z * qz;
    o.y = ((rw * qx + rx * qw) + ry * qz) + nr.z * qy;
    o.z = ((rw * qy + nr.x * qz) + ry * qw) + rz * qx;
    o.w = ((rw * qz + rx * qy) + nr.y * qx) + rz * qw;
    if (aligned16(g.out_quats)) {
        ((float4 *)g.out_quats)[row] = o;
    } else {
        g.out_quats[4 * row] = o.x, g.out_quats[4 * row + 1] = o.y, g.out_quats[4 * row + 2] = o.z, g.out_quats[4 * row + 3] = o.w;
    }
}

// band L of one (Gaussian, channel): v = the band's first coefficient in LDS, the next ones 3 words apart; M: row-major
template <int L>
__device__ __forceinline__ void rotate_band(const float *__restrict__ M, float *v) {
    constexpr int W = 2 * L + 1;
    float c[W], o[W];
#pragma unroll
    for (int j = 0; j < W; ++j) c[j] = v[3 * j];
#pragma unroll
    for (int m = 0; m < W; ++m) {
        float acc = M[m * W] * c[0];
#pragma unroll
        for (int j = 1; j < W; ++j) acc = acc + M[m * W + j] * c[j];
        o[m] = acc;
    }
#pragma unroll
    for (int m = 0; m < W; ++m) v[3 * m] = o[m];
}

// global span of rows W floats wide, `count` floats -> LDS rows S words apart
template <int W, int S>
__device__ __forceinline__ void stage(const float *__restrict__ src, uint32_t count, float *lds) {
    const uint32_t tid = threadIdx.x;
    uint32_t done = 0;
    if (aligned16(src)) {
        const uint32_t n4 = count >> 2;
        for (uint32_t i = tid; i < n4; i += kThreads) {
            const float4 f = ((const float4 *)src)[i];
            const float v[4] = {f.x, f.y, f.z, f.w};
            uint32_t r = (i << 2) / W, o = (i << 2) - r * W;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lds[r * S + o] = v[j];
                if (++o == W) o = 0, ++r;
            }
        }
        done = n4 << 2;
    }
    for (uint32_t e = done + tid; e < count; e += kThreads) {
        const uint32_t r = e / W;
        lds[r * S + (e - r * W)] = src[e];
    }
}

template <int W, int S>
__device__ __forceinline__ void emit(float *__restrict__ dst, uint32_t count, const float *lds) {
    const uint32_t tid = threadIdx.x;
    uint32_t done = 0;
    if (aligned16(dst)) {
        const uint32_t n4 = count >> 2;
        for (uint32_t i = tid; i < n4; i += kThreads) {
            uint32_t r = (i << 2) / W, o = (i << 2) - r * W;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = lds[r * S + o];
                if (++o == W) o = 0, ++r;
            }
            ((float4 *)dst)[i] = make_float4(v[0], v[1], v[2], v[3]);
        }
        done = n4 << 2;
    }
    for (uint32_t e = done + tid; e < count; e += kThreads) {
        const uint32_t r = e / W;
        dst[e] = lds[r * S + (e - r * W)];
    }
}

template <int K>
__global__ void __launch_bounds__(kThreads)
k_scene_transform(const ms_transform xf, const NegQuat nr, int64_t N, const Geometry g, const float *__restrict__ features,
                  float *__restrict__ out_features) {
    constexpr int W = 3 * K, S = W | 1;
    __shared__ float lds[kRows * S];
    const uint32_t tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kRows;
    const uint32_t n = (uint32_t)(N - row0 < kRows ? N - row0 : kRows);
    stage<W, S>(features + (size_t)row0 * W, n * W, lds);
    __syncthreads();
    const uint32_t wave = tid >> 6, lane = tid & 63;
    if (lane < n) {
        if (wave < 3) {
            float *v = lds + lane * S + wave;                        // coefficient k of this channel: v[3 k]
            rotate_band<1>(xf.M1, v + 3 * 1);
            if (K >= 9) rotate_band<2>(xf.M2, v + 3 * 4);
            if (K >= 16) rotate_band<3>(xf.M3, v + 3 * 9);
            if (K >= 25) rotate_band<4>(xf.M4, v + 3 * 16);
        } else {
            move_geometry(xf, nr, g, (size_t)row0 + lane);
        }
    }
    __syncthreads();
    emit<W, S>(out_features + (size_t)row0 * W, n * W, lds);
}

__global__ void __launch_bounds__(kThreads)
k_scene_transform_k1(const ms_transform xf, const NegQuat nr, int64_t N, const Geometry g, const float *__restrict__ features,
                     float *__restrict__ out_features) {
    const uint32_t tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kRowsK1;
    const uint32_t n = (uint32_t)(N - row0 < kRowsK1 ? N - row0 : kRowsK1);
    if (tid < n) move_geometry(xf, nr, g, (size_t)row0 + tid);
    const float *__restrict__ src = features + (size_t)row0 * 3;
    float *__restrict__ dst = out_features + (size_t)row0 * 3;
    const uint32_t count = n * 3;
    uint32_t done = 0;
    if (aligned16(src) && aligned16(dst)) {
        const uint32_t n4 = count >> 2;
        for (uint32_t i = tid; i < n4; i += kThreads) ((float4 *)dst)[i] = ((const float4 *)src)[i];
        done = n4 << 2;
    }
    for (uint32_t e = done + tid; e < count; e += kThreads) dst[e] = src[e];
}

template <int K>
void launch(uint32_t grid, hipStream_t stream, const ms_transform &xf, const NegQuat &nr, int64_t N, const Geometry &g,
            const float *features, float *out_features) {
    hipLaunchKernelGGL(k_scene_transform<K>, dim3(grid), dim3(kThreads), 0, stream, xf, nr, N, g, features, out_features);
}

}  // namespace

extern "C" int ms_scene_transform(int64_t N, int K, const float *means, const float *scales, const float *quats,
                                  const float *features, const ms_transform *xf, float *out_means, float *out_scales,
                                  float *out_quats, float *out_features, void *stream) {
    MS_REQUIRE(N >= 0, MS_ERR_INVALID_ARG, "scene_transform: N < 0");
    if (N == 0) return MS_OK;
    MS_REQUIRE(K == 1 || K == 4 || K == 9 || K == 16 || K == 25, MS_ERR_INVALID_ARG,
               "scene_transform: K = %d, not one of 1, 4, 9, 16, 25", K);
    const void *p[] = {means, scales, quats, features, out_means, out_scales, out_quats, out_features};
    for (const void *q : p) {
        MS_REQUIRE(q, MS_ERR_INVALID_ARG, "scene_transform: null pointer");
        MS_REQUIRE(((uintptr_t)q & 3) == 0, MS_ERR_INVALID_ARG, "scene_transform: misaligned pointer (float: 4 bytes)");
    }
    MS_REQUIRE(xf, MS_ERR_INVALID_ARG, "scene_transform: null pointer (xf)");
    const int64_t groups = ms::ceil_div(N, K == 1 ? kRowsK1 : kRows);
    MS_REQUIRE(groups <= 0x7FFFFFFF, MS_ERR_TOO_LARGE, "scene_transform: %lld rows, more than a launch has workgroups for",
               (long long)N);
    const Geometry g = {means, scales, quats, out_means, out_scales, out_quats};
    const NegQuat nr = {-xf->r[1], -xf->r[2], -xf->r[3]};
    const uint32_t grid = (uint32_t)groups;
    hipStream_t s = (hipStream_t)stream;
    switch (K) {
    case 1:
        hipLaunchKernelGGL(k_scene_transform_k1, dim3(grid), dim3(kThreads), 0, s, *xf, nr, N, g, features, out_features);
        break;
    case 4: launch<4>(grid, s, *xf, nr, N, g, features, out_features); break;
    case 9: launch<9>(grid, s, *xf, nr, N, g, features, out_features); break;
    case 16: launch<16>(grid, s, *xf, nr, N, g, features, out_features); break;
    default: launch<25>(grid, s, *xf, nr, N, g, features, out_features); break;
    }
    MS_LAUNCH_CHECK();
    return MS_OK;
}
