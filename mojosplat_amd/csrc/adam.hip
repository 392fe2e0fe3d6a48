// The parameter update of 3DGS training, fused: one Adam step of up to MS_ADAM_MAX_TENSORS parameter tensors in ONE launch,
// optionally masked by the view's visibility.  mojosplat_amd/optim.py holds the definition (GaussianAdam, backend="torch");
// nothing in the reference updates a parameter (it is forward-only), the CUDA stack has torch.optim.Adam(fused=True) and
// gsplat's SelectiveAdam for this.  Per element, in float32:
//   m' = beta1 m + (1 - beta1) g,   v' = beta2 v + (1 - beta2) g g,   p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)
// i.e. torch.optim.Adam without amsgrad, weight decay or maximize.  bc1 = 1 - beta1^t and sqrt(bc2) come from the HOST's step
// count (ms_adam_tensor); nothing on the device counts steps, no launch precedes this one and nothing waits for it.
//
// THE TABLE.  The kernel takes AdamTable by value (kernel arguments: 8 records of 80 bytes): per tensor its four pointers,
// its element count and row width, the rounded-once constants beta1, 1 - beta1, beta2, 1 - beta2, lr / bc1 (formed in
// double), sqrt(bc2), eps, and the END of its run of chunks.  A chunk is 1024 consecutive elements of one tensor -- a float4
// per lane of a 256-lane workgroup.  The tensors' chunks are numbered through (tensor 0's, then tensor 1's ...), and the
// grid (at most 2048 workgroups: 8 per CU, the residency of a 256-lane workgroup at this register count) strides over that
// one numbering: every tensor gets workgroup-iterations in proportion to its size, an (N,) tensor of opacities is 1/59 of
// an SH scene's iterations rather than a launch of its own.  Which tensor a chunk belongs to is a scan of at most 8
// wave-uniform words.
//
// ACCESS.  A lane's four elements are one 16-byte load each of p, g, m, v and one 16-byte store each of p, m, v when the
// four pointers are 16-byte aligned (checked on the host, per tensor), the elements exist (not the tensor's last, partial
// vector) and every row they touch is visible.  Rows: with a mask, row = element / width; a width that is a multiple of 4
// keeps a vector inside one row (one mask byte), any other width (3: means, scales; 1: opacities) lets a vector straddle up
// to four rows and the mask is read per element.  A vector whose rows are all masked loads and stores NOTHING; one with
// visible and masked elements mixed -- and the partial vector at a tensor's end, and a tensor with a misaligned pointer --
// goes element by element, dword loads and stores of the visible elements only.  Both forms call the same adam_element,
// compiled without contraction, with IEEE sqrtf and division: a visible element gets the same bits whichever form carried
// it, whatever the mask, and an all-visible mask gives the bits of no mask.  Masked rows of p, m, v are never written.
// No atomics, no LDS, no cross-lane traffic: elementwise, bitwise reproducible.
//
// BYTES.  Dense: p, g, m, v in and p, m, v out, 28 bytes per element (59 floats per Gaussian with SH degree 3: 1.65 GB per
// million Gaussians, 263 us at the 6.29 TB/s copy rate; 14 floats with RGB: 392 MB, 62 us).  Masked: 28 bytes per VISIBLE
// element + 1 byte per row per tensor of mask, at the granularity the memory system fetches (a 12-byte row of a scattered
// mask shares its 128-byte line with ten neighbours: see DESIGN.md 4c for what was measured).
// Tensors of 2^31 elements or more are REFUSED (MS_ERR_TOO_LARGE): element offsets are 32-bit.
#include <math.h>

#include "ms_common.hpp"

namespace {

constexpr int kAdamThreads = 256;
constexpr int kChunk = kAdamThreads * 4;      // elements of a workgroup-iteration
constexpr unsigned kAdamMaxGrid = 2048;       // 256 CUs x 8 resident workgroups

struct AdamRec {
    float *p;
    const float *g;
    float *m, *v;
    uint32_t n, width;          // elements (rows * width), elements per row
    uint32_t chunk_end;         // this tensor owns the chunks [previous record's chunk_end, chunk_end)
    uint32_t vec_ok;            // all four pointers 16-byte aligned
    float beta1, omb1, beta2, omb2, step, bc2s, eps;
    float pad_;
};
struct AdamTable {
    AdamRec rec[MS_ADAM_MAX_TENSORS];
};
static_assert(sizeof(AdamRec) == 80, "the table is a kernel argument: keep it small");

struct AdamOut {
    float p, m, v;
};

// One element.  No contraction: every product and sum is rounded on its own, so the result does not depend on what the
// compiler could fuse around the call site (the vector and the element-by-element forms must agree bit for bit).
__device__ __forceinline__ AdamOut adam_element(float p, float g, float m, float v, const AdamRec &r) {
#pragma clang fp contract(off)
    AdamOut o;
    o.m = r.beta1 * m + r.omb1 * g;
    o.v = r.beta2 * v + (r.omb2 * g) * g;
    const float denom = sqrtf(o.v) / r.bc2s + r.eps;
    o.p = p - (r.step * o.m) / denom;
    return o;
}

__global__ void __launch_bounds__(kAdamThreads)
k_adam_step(const AdamTable tab, int n_tensors, uint32_t total_chunks, const uint8_t *__restrict__ visible) {
    for (uint32_t chunk = blockIdx.x; chunk < total_chunks; chunk += gridDim.x) {
        int t = 0;
        uint32_t first = 0;
        while (t + 1 < n_tensors && chunk >= tab.rec[t].chunk_end) first = tab.rec[t++].chunk_end;
        const AdamRec r = tab.rec[t];
        const uint32_t e = (chunk - first) * (uint32_t)kChunk + threadIdx.x * 4u;   // < n + kChunk <= 2^31 + 1023
        if (e >= r.n) continue;
        const bool whole = e + 4u <= r.n;

        // which of the lane's (up to) four elements are visible
        bool vis[4] = {true, true, true, true};
        if (visible) {
            uint32_t row = e / r.width;
            if ((r.width & 3u) == 0u) {
                vis[0] = vis[1] = vis[2] = vis[3] = visible[row] != 0;
            } else {
                uint32_t col = e - row * r.width;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    vis[k] = e + k < r.n && visible[row] != 0;   // (row < rows as long as the element exists)
                    if (++col == r.width) {
                        col = 0;
                        ++row;
                    }
                }
            }
        }
        const bool all = vis[0] && vis[1] && vis[2] && vis[3], any = vis[0] || vis[1] || vis[2] || vis[3];
        if (!any) continue;

        if (all && whole && r.vec_ok) {
            const float4 p4 = *reinterpret_cast<const float4 *>(r.p + e), g4 = *reinterpret_cast<const float4 *>(r.g + e);
            const float4 m4 = *reinterpret_cast<const float4 *>(r.m + e), v4 = *reinterpret_cast<const float4 *>(r.v + e);
            const AdamOut a = adam_element(p4.x, g4.x, m4.x, v4.x, r), b = adam_element(p4.y, g4.y, m4.y, v4.y, r);
            const AdamOut c = adam_element(p4.z, g4.z, m4.z, v4.z, r), d = adam_element(p4.w, g4.w, m4.w, v4.w, r);
            *reinterpret_cast<float4 *>(r.p + e) = make_float4(a.p, b.p, c.p, d.p);
            *reinterpret_cast<float4 *>(r.m + e) = make_float4(a.m, b.m, c.m, d.m);
            *reinterpret_cast<float4 *>(r.v + e) = make_float4(a.v, b.v, c.v, d.v);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t i = e + k;
                if (i < r.n && vis[k]) {
                    const AdamOut o = adam_element(r.p[i], r.g[i], r.m[i], r.v[i], r);
                    r.p[i] = o.p;
                    r.m[i] = o.m;
                    r.v[i] = o.v;
                }
            }
        }
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int ms_adam_step(int n_tensors, const ms_adam_tensor *tensors, const uint8_t *visible, int64_t visible_rows,
                            void *stream_) {
    MS_REQUIRE(n_tensors >= 1 && n_tensors <= MS_ADAM_MAX_TENSORS, MS_ERR_INVALID_ARG,
               "adam_step: n_tensors = %d, not in [1, %d]", n_tensors, MS_ADAM_MAX_TENSORS);
    MS_REQUIRE(tensors, MS_ERR_INVALID_ARG, "adam_step: null pointer (tensors)");
    MS_REQUIRE(!visible || visible_rows > 0, MS_ERR_INVALID_ARG, "adam_step: a mask of %lld rows", (long long)visible_rows);
    AdamTable tab = {};
    uint64_t chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const ms_adam_tensor &t = tensors[i];
        MS_REQUIRE(t.param && t.grad && t.exp_avg && t.exp_avg_sq, MS_ERR_INVALID_ARG,
                   "adam_step: null pointer (tensor %d: param, grad, exp_avg or exp_avg_sq)", i);
        MS_REQUIRE(t.rows > 0 && t.width > 0, MS_ERR_INVALID_ARG, "adam_step: tensor %d: non-positive size (rows %lld, width %lld)",
                   i, (long long)t.rows, (long long)t.width);
        MS_REQUIRE(t.rows < ((int64_t)1 << 31) && t.width < ((int64_t)1 << 31) && t.rows * t.width < ((int64_t)1 << 31),
                   MS_ERR_TOO_LARGE, "adam_step: tensor %d: %lld x %lld elements, 2^31 or more (32-bit offsets)", i,
                   (long long)t.rows, (long long)t.width);
        MS_REQUIRE(isfinite(t.lr) && t.lr >= 0.0, MS_ERR_INVALID_ARG, "adam_step: tensor %d: lr %g is negative or not finite", i, t.lr);
        MS_REQUIRE(t.beta1 >= 0.0 && t.beta1 < 1.0 && t.beta2 >= 0.0 && t.beta2 < 1.0, MS_ERR_INVALID_ARG,
                   "adam_step: tensor %d: beta (%g, %g) outside [0, 1)", i, t.beta1, t.beta2);
        MS_REQUIRE(t.eps > 0.0, MS_ERR_INVALID_ARG, "adam_step: tensor %d: eps %g is not positive", i, t.eps);
        MS_REQUIRE(t.bias_correction1 > 0.0 && t.bias_correction1 <= 1.0 && t.bias_correction2_sqrt > 0.0 &&
                       t.bias_correction2_sqrt <= 1.0,
                   MS_ERR_INVALID_ARG, "adam_step: tensor %d: bias correction (%g, sqrt %g) outside (0, 1]", i,
                   t.bias_correction1, t.bias_correction2_sqrt);
        MS_REQUIRE(!visible || t.rows == visible_rows, MS_ERR_INVALID_ARG,
                   "adam_step: tensor %d has %lld rows, the visibility mask %lld", i, (long long)t.rows, (long long)visible_rows);
        AdamRec &r = tab.rec[i];
        r.p = t.param;
        r.g = t.grad;
        r.m = t.exp_avg;
        r.v = t.exp_avg_sq;
        r.n = (uint32_t)(t.rows * t.width);
        r.width = (uint32_t)t.width;
        chunks += (uint64_t)ms::ceil_div((int64_t)r.n, kChunk);
        r.chunk_end = (uint32_t)chunks;     // <= 8 * 2^21
        r.vec_ok = aligned16(t.param) && aligned16(t.grad) && aligned16(t.exp_avg) && aligned16(t.exp_avg_sq);
        r.beta1 = (float)t.beta1;
        r.omb1 = (float)(1.0 - t.beta1);
        r.beta2 = (float)t.beta2;
        r.omb2 = (float)(1.0 - t.beta2);
        r.step = (float)(t.lr / t.bias_correction1);
        r.bc2s = (float)t.bias_correction2_sqrt;
        r.eps = (float)t.eps;
        MS_REQUIRE(isfinite(r.step) && r.eps > 0.f && r.bc2s > 0.f, MS_ERR_INVALID_ARG,
                   "adam_step: tensor %d: lr / bias_correction1, eps or sqrt(bias_correction2) leaves float32's range", i);
    }
    const uint32_t total = (uint32_t)chunks;
    const unsigned grid = total < kAdamMaxGrid ? total : kAdamMaxGrid;
    hipLaunchKernelGGL(k_adam_step, dim3(grid), dim3(kAdamThreads), 0, (hipStream_t)stream_, tab, n_tensors, total, visible);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
