// Viewer formats: the bit packing of the PlayCanvas / SuperSplat compressed PLY (16 bytes per Gaussian, a byte per higher-order
// SH coefficient, 18 floats per chunk of 256 Gaussians) and of the 32-byte .splat row (mojosplat_amd/splatio.py holds both
// formats and the definition, backend="torch"; nothing in the reference does this: it reads and writes no scene).  Four
// kernels, one launch each, no atomics, no workspace, no host wait.
//
// The transcendental and normalising conversions (sigmoid, exp, log, the quaternion's norm) are torch ops outside these
// kernels, the same for both backends.  What is here is EXACT in IEEE float32 -- compare, subtract, divide, multiply, add,
// floor, trunc, sqrt, convert -- and written in the definition's operation order with contraction off (the assembly holds no
// fused multiply-add), division and square root correctly rounded, denormals kept: the bits are the definition's.
//
// COMPRESS    a workgroup is a chunk, a lane a row.  The lane loads its 13 floats; the nine (min, max) pairs are reduced over
//             each row of 16 lanes by four DPP steps on the vector pipe (no LDS traffic), then across the chunk's 16 such
//             rows through 16 x 18 LDS words (min and max of finite floats do not depend on the reduction tree); lanes
//             0..17 write the chunk row and leave it in LDS for everybody; every lane packs its four words and stores them
//             as 16 bytes.  Rows past N carry the neutral element through the reduction and write nothing.
//             The SH bytes are an element-wise map of the chunk's contiguous span of shr (byte i of the span comes from float
//             i): a lane converts a float4 into one packed dword, 256 contiguous bytes per wave store, with no LDS round
//             trip; only the last chunk can end in a tail of fewer than four bytes.
// DECOMPRESS  the same shape without the reduction: the chunk row is uniform in the workgroup (scalar loads).
// SPLAT32     a lane is a 32-byte row, moved as two 16-byte accesses.
// Every global row index is 64-bit.  Within a chunk an index is below 256 * 3 (K - 1) and stays 32-bit.
#include "ms_common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kChunk = MS_SPLAT_CHUNK;             // rows of a workgroup = Gaussians of a chunk
constexpr int kParts = kChunk / 16;                // DPP rows of 16 lanes: a partial (min, max) set each
static_assert(kChunk % 64 == 0, "a chunk is whole waves");
constexpr int kChunkFloats = 18;
constexpr float kInf = __builtin_huge_valf();

__device__ __forceinline__ bool aligned_to(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// ---- the format's helpers (splatio.py, "Helpers") ------------------------------------------------------------------------
__device__ __forceinline__ float norm01(float v, float lo, float hi) {
    if (v <= lo) return 0.f;
    if (v >= hi) return 1.f;
    const float d = hi - lo;
    if (d < 1e-5f) return 0.f;
    return (v - lo) / d;
}
template <int BITS>
__device__ __forceinline__ uint32_t pack_bits(float v) {
    constexpr float t = (float)((1u << BITS) - 1u);
    return (uint32_t)fminf(t, fmaxf(0.f, floorf(v * t + 0.5f)));
}
template <int BITS>
__device__ __forceinline__ float unit(uint32_t x) {
    constexpr uint32_t mask = (1u << BITS) - 1u;
    return (float)(x & mask) / (float)mask;
}
__device__ __forceinline__ float mix(float lo, float hi, float u) { return lo * (1.f - u) + hi * u; }
__device__ __forceinline__ uint32_t byte_of(float x) { return (uint32_t)fminf(255.f, fmaxf(0.f, truncf(x))); }
__device__ __forceinline__ uint32_t sh_byte(float v) { return byte_of((v / 8.f + 0.5f) * 256.f); }
__device__ __forceinline__ float sh_value(uint32_t b) { return (float)b * (8.0f / 255.0f) - 4.0f; }

__device__ __forceinline__ uint32_t pack_11_10_11(float x, float y, float z) {
    return pack_bits<11>(x) << 21 | pack_bits<10>(y) << 11 | pack_bits<11>(z);
}

// the largest |component| first (the first of equals), its sign made positive, then the other three in order
__device__ __forceinline__ uint32_t pack_rotation(float4 q) {
    float a0 = q.x, a1 = q.y, a2 = q.z, a3 = q.w;
    uint32_t L = 0;
    float best = fabsf(a0);
    if (fabsf(a1) > best) L = 1, best = fabsf(a1);
    if (fabsf(a2) > best) L = 2, best = fabsf(a2);
    if (fabsf(a3) > best) L = 3, best = fabsf(a3);
    const float top = L == 0 ? a0 : L == 1 ? a1 : L == 2 ? a2 : a3;
    if (top < 0.f) a0 = -a0, a1 = -a1, a2 = -a2, a3 = -a3;
    const uint32_t p0 = pack_bits<10>(a0 * 0.70710678f + 0.5f), p1 = pack_bits<10>(a1 * 0.70710678f + 0.5f);
    const uint32_t p2 = pack_bits<10>(a2 * 0.70710678f + 0.5f), p3 = pack_bits<10>(a3 * 0.70710678f + 0.5f);
    uint32_t word = L;
    if (L != 0) word = word << 10 | p0;
    if (L != 1) word = word << 10 | p1;
    if (L != 2) word = word << 10 | p2;
    if (L != 3) word = word << 10 | p3;
    return word;
}

__device__ __forceinline__ float4 unpack_rotation(uint32_t word) {
    const uint32_t L = word >> 30;
    const float a = (unit<10>(word >> 20) - 0.5f) * 1.41421356f;
    const float b = (unit<10>(word >> 10) - 0.5f) * 1.41421356f;
    const float c = (unit<10>(word) - 0.5f) * 1.41421356f;
    const float m = sqrtf(fmaxf(0.f, ((1.f - a * a) - b * b) - c * c));
    return make_float4(L == 0 ? m : a, L == 1 ? m : L == 0 ? a : b, L == 2 ? m : L < 2 ? b : c, L == 3 ? m : c);
}

// min / max over the lane's DPP row of 16 lanes, in every lane of the row: the quad's other three lanes (quad_perm [1,0,3,2],
// then [2,3,0,1]), then the row rotated by 4 and by 8.  min and max are commutative and idempotent, so the overlapping rotations
// are exact, and the result does not depend on the order (finite values).  Every lane of the wave must be active.
template <int CTRL>
__device__ __forceinline__ float dpp_move(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float row_min(float x) {
    x = fminf(x, dpp_move<0xB1>(x));
    x = fminf(x, dpp_move<0x4E>(x));
    x = fminf(x, dpp_move<0x124>(x));   // row_ror:4
    return fminf(x, dpp_move<0x128>(x));   // row_ror:8
}
__device__ __forceinline__ float row_max(float x) {
    x = fmaxf(x, dpp_move<0xB1>(x));
    x = fmaxf(x, dpp_move<0x4E>(x));
    x = fmaxf(x, dpp_move<0x124>(x));
    return fmaxf(x, dpp_move<0x128>(x));
}

// the element-wise maps between a chunk's span of shr (count floats) and of sh (count bytes)
__device__ __forceinline__ void sh_to_bytes(const float *__restrict__ src, uint8_t *__restrict__ dst, uint32_t count) {
    const uint32_t tid = threadIdx.x;
    uint32_t done = 0;
    if (aligned_to(src, 16) && aligned_to(dst, 4)) {
        const uint32_t n4 = count >> 2;
        for (uint32_t i = tid; i < n4; i += kChunk) {
            const float4 f = ((const float4 *)src)[i];
            ((uint32_t *)dst)[i] = sh_byte(f.x) | sh_byte(f.y) << 8 | sh_byte(f.z) << 16 | sh_byte(f.w) << 24;
        }
        done = n4 << 2;
    }
    for (uint32_t i = done + tid; i < count; i += kChunk) dst[i] = (uint8_t)sh_byte(src[i]);
}
__device__ __forceinline__ void bytes_to_sh(const uint8_t *__restrict__ src, float *__restrict__ dst, uint32_t count) {
    const uint32_t tid = threadIdx.x;
    uint32_t done = 0;
    if (aligned_to(src, 4) && aligned_to(dst, 16)) {
        const uint32_t n4 = count >> 2;
        for (uint32_t i = tid; i < n4; i += kChunk) {
            const uint32_t w = ((const uint32_t *)src)[i];
            ((float4 *)dst)[i] = make_float4(sh_value(w & 255u), sh_value(w >> 8 & 255u), sh_value(w >> 16 & 255u), sh_value(w >> 24));
        }
        done = n4 << 2;
    }
    for (uint32_t i = done + tid; i < count; i += kChunk) dst[i] = sh_value(src[i]);
}

// ---- compressed PLY ------------------------------------------------------------------------------------------------------
// R = 3 (K - 1) SH bytes per row (0: no sh); rot, rgba and vertices are 16-byte aligned (checked by the entry point)
__global__ void __launch_bounds__(kChunk)
k_splat_compress(int64_t N, uint32_t R, const float *__restrict__ pos, const float4 *__restrict__ rot,
                 const float *__restrict__ lsc, const float4 *__restrict__ rgba, const float *__restrict__ shr,
                 float *__restrict__ chunks, uint4 *__restrict__ vertices, uint8_t *__restrict__ sh) {
    __shared__ float s_part[kParts][kChunkFloats];
    __shared__ float s_chunk[kChunkFloats];
    const uint32_t tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kChunk;
    const uint32_t n = (uint32_t)(N - row0 < kChunk ? N - row0 : kChunk);
    const bool live = tid < n;
    const size_t row = (size_t)row0 + tid;
    float v[9];                                                       // pos, lsc, rgb
    float4 q = make_float4(1.f, 0.f, 0.f, 0.f);
    float alpha = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = 0.f;
    if (live) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = pos[3 * row + k], v[3 + k] = lsc[3 * row + k];
        const float4 c = rgba[row];
        v[6] = c.x, v[7] = c.y, v[8] = c.z, alpha = c.w;
        q = rot[row];
    }
    // every lane runs the reduction (a row past N carries the neutral element): the DPP steps need their whole row.
    // s_part[r] is laid out as the chunk row: (min, max) x (pos, lsc, rgb), three floats each
    float mn[9], mx[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) mn[k] = row_min(live ? v[k] : kInf), mx[k] = row_max(live ? v[k] : -kInf);
    if ((tid & 15) == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            s_part[tid >> 4][(k / 3) * 6 + k % 3] = mn[k];
            s_part[tid >> 4][(k / 3) * 6 + 3 + k % 3] = mx[k];
        }
    }
    __syncthreads();
    if (tid < kChunkFloats) {
        const bool is_max = (tid / 3) & 1;
        float r = s_part[0][tid];
#pragma unroll
        for (int w = 1; w < kParts; ++w) r = is_max ? fmaxf(r, s_part[w][tid]) : fminf(r, s_part[w][tid]);
        s_chunk[tid] = r;
        chunks[(size_t)blockIdx.x * kChunkFloats + tid] = r;
    }
    __syncthreads();
    if (live) {
        float u[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) u[k] = norm01(v[k], s_chunk[(k / 3) * 6 + k % 3], s_chunk[(k / 3) * 6 + 3 + k % 3]);
        uint4 w;
        w.x = pack_11_10_11(u[0], u[1], u[2]);
        w.y = pack_rotation(q);
        w.z = pack_11_10_11(u[3], u[4], u[5]);
        w.w = pack_bits<8>(u[6]) << 24 | pack_bits<8>(u[7]) << 16 | pack_bits<8>(u[8]) << 8 | pack_bits<8>(alpha);
        vertices[row] = w;
    }
    if (R) sh_to_bytes(shr + (size_t)row0 * R, sh + (size_t)row0 * R, n * R);
}

// chunk_floats: 18, or 12 (no colour bounds: 0 and 1)
__global__ void __launch_bounds__(kChunk)
k_splat_decompress(int64_t N, uint32_t R, uint32_t chunk_floats, const float *__restrict__ chunks,
                   const uint4 *__restrict__ vertices, const uint8_t *__restrict__ sh, float *__restrict__ pos,
                   float4 *__restrict__ rot, float *__restrict__ lsc, float4 *__restrict__ rgba, float *__restrict__ shr) {
    const uint32_t tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kChunk;
    const uint32_t n = (uint32_t)(N - row0 < kChunk ? N - row0 : kChunk);
    if (tid < n) {
        const size_t row = (size_t)row0 + tid;
        const float *__restrict__ ch = chunks + (size_t)blockIdx.x * chunk_floats;      // (uniform)
        float lo[9], hi[9];
#pragma unroll
        for (int k = 0; k < 6; ++k) lo[k] = ch[(k / 3) * 6 + k % 3], hi[k] = ch[(k / 3) * 6 + 3 + k % 3];
#pragma unroll
        for (int k = 6; k < 9; ++k) {
            lo[k] = chunk_floats == kChunkFloats ? ch[6 + k] : 0.f;
            hi[k] = chunk_floats == kChunkFloats ? ch[9 + k] : 1.f;
        }
        const uint4 w = vertices[row];
        pos[3 * row + 0] = mix(lo[0], hi[0], unit<11>(w.x >> 21));
        pos[3 * row + 1] = mix(lo[1], hi[1], unit<10>(w.x >> 11));
        pos[3 * row + 2] = mix(lo[2], hi[2], unit<11>(w.x));
        lsc[3 * row + 0] = mix(lo[3], hi[3], unit<11>(w.z >> 21));
        lsc[3 * row + 1] = mix(lo[4], hi[4], unit<10>(w.z >> 11));
        lsc[3 * row + 2] = mix(lo[5], hi[5], unit<11>(w.z));
        rgba[row] = make_float4(mix(lo[6], hi[6], unit<8>(w.w >> 24)), mix(lo[7], hi[7], unit<8>(w.w >> 16)),
                                mix(lo[8], hi[8], unit<8>(w.w >> 8)), unit<8>(w.w));
        rot[row] = unpack_rotation(w.y);
    }
    if (R) bytes_to_sh(sh + (size_t)row0 * R, shr + (size_t)row0 * R, n * R);
}

// ---- .splat --------------------------------------------------------------------------------------------------------------
// a row: pos 3 x f32 | scale 3 x f32 | r g b a bytes | w x y z bytes; rows, rgba and rot are 16-byte aligned
__global__ void __launch_bounds__(kChunk)
k_splat32_pack(int64_t N, const float *__restrict__ pos, const float *__restrict__ scale, const float4 *__restrict__ rgba,
               const float4 *__restrict__ rot, uint4 *__restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    if (i >= N) return;
    const size_t row = (size_t)i;
    const float4 c = rgba[row], q = rot[row];
    uint4 a, b;
    a.x = __float_as_uint(pos[3 * row]), a.y = __float_as_uint(pos[3 * row + 1]), a.z = __float_as_uint(pos[3 * row + 2]);
    a.w = __float_as_uint(scale[3 * row]);
    b.x = __float_as_uint(scale[3 * row + 1]), b.y = __float_as_uint(scale[3 * row + 2]);
    b.z = byte_of(c.x * 255.f) | byte_of(c.y * 255.f) << 8 | byte_of(c.z * 255.f) << 16 | byte_of(c.w * 255.f) << 24;
    b.w = byte_of(q.x * 128.f + 128.f) | byte_of(q.y * 128.f + 128.f) << 8 | byte_of(q.z * 128.f + 128.f) << 16 |
          byte_of(q.w * 128.f + 128.f) << 24;
    rows[2 * row] = a;
    rows[2 * row + 1] = b;
}

__global__ void __launch_bounds__(kChunk)
k_splat32_unpack(int64_t N, const uint4 *__restrict__ rows, float *__restrict__ pos, float *__restrict__ scale,
                 float4 *__restrict__ rgba, float4 *__restrict__ rot) {
    const int64_t i = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    if (i >= N) return;
    const size_t row = (size_t)i;
    const uint4 a = rows[2 * row], b = rows[2 * row + 1];
    pos[3 * row] = __uint_as_float(a.x), pos[3 * row + 1] = __uint_as_float(a.y), pos[3 * row + 2] = __uint_as_float(a.z);
    scale[3 * row] = __uint_as_float(a.w), scale[3 * row + 1] = __uint_as_float(b.x), scale[3 * row + 2] = __uint_as_float(b.y);
    rgba[row] = make_float4((float)(b.z & 255u) / 255.f, (float)(b.z >> 8 & 255u) / 255.f, (float)(b.z >> 16 & 255u) / 255.f,
                            (float)(b.z >> 24) / 255.f);
    rot[row] = make_float4(((float)(b.w & 255u) - 128.f) / 128.f, ((float)(b.w >> 8 & 255u) - 128.f) / 128.f,
                           ((float)(b.w >> 16 & 255u) - 128.f) / 128.f, ((float)(b.w >> 24) - 128.f) / 128.f);
}

int check_rows(const char *who, int64_t N) {
    MS_REQUIRE(N >= 0, MS_ERR_INVALID_ARG, "%s: N < 0", who);
    MS_REQUIRE(ms::ceil_div(N, kChunk) <= 0x7FFFFFFF, MS_ERR_TOO_LARGE, "%s: %lld rows, more than a launch has workgroups for", who,
               (long long)N);
    return MS_OK;
}

// the arrays every entry point has: floats (4-byte aligned) and float4 / uint4 rows (16-byte aligned)
int check_pointers(const char *who, const void *const *f4, int n4, const void *const *f16, int n16) {
    for (int k = 0; k < n4; ++k) {
        MS_REQUIRE(f4[k], MS_ERR_INVALID_ARG, "%s: null pointer", who);
        MS_REQUIRE(((uintptr_t)f4[k] & 3) == 0, MS_ERR_INVALID_ARG, "%s: misaligned pointer (float: 4 bytes)", who);
    }
    for (int k = 0; k < n16; ++k) {
        MS_REQUIRE(f16[k], MS_ERR_INVALID_ARG, "%s: null pointer", who);
        MS_REQUIRE(((uintptr_t)f16[k] & 15) == 0, MS_ERR_INVALID_ARG, "%s: misaligned pointer (rows of four words: 16 bytes)", who);
    }
    return MS_OK;
}

}  // namespace

extern "C" int ms_splat_compress(int64_t N, int K, const float *pos, const float *rot, const float *lsc, const float *rgba,
                                 const float *shr, float *chunks, uint32_t *vertices, uint8_t *sh, void *stream) {
    if (int rc = check_rows("splat_compress", N)) return rc;
    if (N == 0) return MS_OK;
    MS_REQUIRE(K >= 1 && K <= MS_SPLAT_MAX_K, MS_ERR_INVALID_ARG, "splat_compress: K = %d, not in [1, %d]", K, MS_SPLAT_MAX_K);
    const void *f4[] = {pos, lsc, chunks}, *f16[] = {rot, rgba, vertices};
    if (int rc = check_pointers("splat_compress", f4, 3, f16, 3)) return rc;
    MS_REQUIRE(K == 1 || (shr && sh), MS_ERR_INVALID_ARG, "splat_compress: null pointer (shr or sh with K > 1)");
    MS_REQUIRE(((uintptr_t)shr & 3) == 0, MS_ERR_INVALID_ARG, "splat_compress: misaligned pointer (shr: float, 4 bytes)");
    hipLaunchKernelGGL(k_splat_compress, dim3((uint32_t)ms::ceil_div(N, kChunk)), dim3(kChunk), 0, (hipStream_t)stream, N,
                       (uint32_t)(3 * (K - 1)), pos, (const float4 *)rot, lsc, (const float4 *)rgba, shr, chunks, (uint4 *)vertices,
                       sh);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

extern "C" int ms_splat_decompress(int64_t N, int K, int chunk_floats, const float *chunks, const uint32_t *vertices,
                                   const uint8_t *sh, float *pos, float *rot, float *lsc, float *rgba, float *shr, void *stream) {
    if (int rc = check_rows("splat_decompress", N)) return rc;
    if (N == 0) return MS_OK;
    MS_REQUIRE(K >= 1 && K <= MS_SPLAT_MAX_K, MS_ERR_INVALID_ARG, "splat_decompress: K = %d, not in [1, %d]", K, MS_SPLAT_MAX_K);
    MS_REQUIRE(chunk_floats == 12 || chunk_floats == kChunkFloats, MS_ERR_INVALID_ARG,
               "splat_decompress: chunk_floats = %d, neither 12 nor 18", chunk_floats);
    const void *f4[] = {pos, lsc, chunks}, *f16[] = {rot, rgba, vertices};
    if (int rc = check_pointers("splat_decompress", f4, 3, f16, 3)) return rc;
    MS_REQUIRE(K == 1 || (shr && sh), MS_ERR_INVALID_ARG, "splat_decompress: null pointer (shr or sh with K > 1)");
    MS_REQUIRE(((uintptr_t)shr & 3) == 0, MS_ERR_INVALID_ARG, "splat_decompress: misaligned pointer (shr: float, 4 bytes)");
    hipLaunchKernelGGL(k_splat_decompress, dim3((uint32_t)ms::ceil_div(N, kChunk)), dim3(kChunk), 0, (hipStream_t)stream, N,
                       (uint32_t)(3 * (K - 1)), (uint32_t)chunk_floats, chunks, (const uint4 *)vertices, sh, pos, (float4 *)rot, lsc,
                       (float4 *)rgba, shr);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

extern "C" int ms_splat32_pack(int64_t N, const float *pos, const float *scale_lin, const float *rgba, const float *rot,
                               uint8_t *rows, void *stream) {
    if (int rc = check_rows("splat32_pack", N)) return rc;
    if (N == 0) return MS_OK;
    const void *f4[] = {pos, scale_lin}, *f16[] = {rgba, rot, rows};
    if (int rc = check_pointers("splat32_pack", f4, 2, f16, 3)) return rc;
    hipLaunchKernelGGL(k_splat32_pack, dim3((uint32_t)ms::ceil_div(N, kChunk)), dim3(kChunk), 0, (hipStream_t)stream, N, pos,
                       scale_lin, (const float4 *)rgba, (const float4 *)rot, (uint4 *)rows);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

extern "C" int ms_splat32_unpack(int64_t N, const uint8_t *rows, float *pos, float *scale_lin, float *rgba, float *rot,
                                 void *stream) {
    if (int rc = check_rows("splat32_unpack", N)) return rc;
    if (N == 0) return MS_OK;
    const void *f4[] = {pos, scale_lin}, *f16[] = {rgba, rot, rows};
    if (int rc = check_pointers("splat32_unpack", f4, 2, f16, 3)) return rc;
    hipLaunchKernelGGL(k_splat32_unpack, dim3((uint32_t)ms::ceil_div(N, kChunk)), dim3(kChunk), 0, (hipStream_t)stream, N,
                       (const uint4 *)rows, pos, scale_lin, (float4 *)rgba, (float4 *)rot);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
