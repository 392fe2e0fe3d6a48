// The photometric loss of 3DGS training, fused: loss = (1 - lambda) * mean|x - y| + lambda * (1 - mean SSIM(x, y)),
// SSIM under the 11x11 Gaussian window (sigma 1.5) with zero padding, on the (B, H, W, C) float32 image the rasteriser
// writes (channel innermost) -- no permuted copy of x, y or the gradient anywhere.  mojosplat_amd/loss.py holds the
// definition (photometric_loss_torch); nothing in the reference computes a loss (it is forward-only), the CUDA stack has
// its fused-ssim extension for this.
//
// FORWARD, k_loss_fwd: a workgroup of 256 lanes owns 32 x 16 pixels (all C channels) of one image.
//   1. it stages x and y of its 42 x 26 halo rectangle into LDS with coalesced loads (a row of the rectangle is one run of
//      42 C floats in memory); pixels outside the image are zeros (the definition's padding);
//   2. per channel, a horizontal 11-tap pass over the staged rows leaves the five windowed row sums (x, y, x^2, y^2, x y) of
//      26 rows x 32 columns in LDS -- a lane owns 4 neighbouring columns of a row, so its 14 staged values serve 4 outputs;
//   3. a vertical 11-tap pass gives each lane the five sums of two pixels; the lane forms the SSIM of each and (training)
//      the three partial derivatives the backward needs, d ssim / d mu_x (at fixed w*x^2, w*xy), d ssim / d s_xx and
//      d ssim / d s_xy, and stores them as PLANES ([map][b][c][H][W]: the workspace's layout is the kernel's own, so these
//      stores and the backward's loads are coalesced);
//   4. |x - y| and the SSIM are summed over the workgroup (butterfly across a wave, the 4 waves in wave order) and stored
//      as the workgroup's row of partial sums.
// k_loss_finalize (one workgroup) adds the rows in a fixed order, in double, and writes [loss, l1, ssim].
// BACKWARD, k_loss_bwd: the same two passes over the three derivative planes a, b, c (zero outside the image: with zero
// padding the symmetric window is its own adjoint), then
//   v_x = v_loss * ((1 - lambda) / n * sign(x - y) - lambda / n * (w*a + 2 x (w*b) + y (w*c))),      n = B H W C,
// with v_loss read from device memory; the tile's x and y come in and its gradient goes out through LDS, coalesced.
// No float atomics anywhere: every sum has an order fixed by the shapes alone, so the three numbers and the gradient are
// bitwise the same from run to run.
//
// Bytes per training step (I = 4 B H W C, the size of one image): the forward reads 2 I and writes 3 I of planes, the
// backward reads 3 I + 2 I and writes I: 11 I (274 MB at 1920 x 1080 x 3) against 5 I for a backward that would stage a
// 10-pixel halo of x and y and redo the forward's passes on 2.6 times the pixels.  Evaluation (no planes) moves 2 I.
//
// LDS and residency (160 KiB per CU): forward, C = 3: 2 x 26 x 127 staged floats + 5 x 26 x 33 row sums = 43.6 KB -> 3
// workgroups (12 waves) per CU, one staging while others compute; 4 would need a 16 x 16 tile whose halo rectangle is 2.6
// times its pixels.  Backward: 3 x 26 x 43 + 3 x 26 x 33 + 2 x 16 x 96 floats = 36.0 KB -> 4 workgroups per CU.
// __launch_bounds__ states both.  Row strides are odd (127, 43, 33 floats) so that lanes that walk down a column of rows
// fall on different banks.
//
// The windowed sums are float32, accumulated tap by tap; s_xx = w*x^2 - mu_x^2 is formed last, from rounded products (no
// contraction in ssim_point: for x == y numerator and denominator are then the same bits, the SSIM is exactly 1 and
// the gradient exactly 0).
// Images whose B H W C exceeds 2^31 - 1 are REFUSED (MS_ERR_TOO_LARGE): element offsets are 32-bit.
#include "ms_common.hpp"

namespace {

constexpr int kR = 5;                     // window radius: 11 taps
constexpr int kTX = 32, kTY = 16;         // the pixels of a workgroup
constexpr int kHX = kTX + 2 * kR;         // 42: columns of its halo rectangle
constexpr int kHY = kTY + 2 * kR;         // 26: rows
constexpr int kLossThreads = 256;
constexpr int kHS = kTX + 1;              // row stride of the horizontal pass's sums
constexpr int kMS = kHX + 1;              // row stride of a staged derivative plane (backward)
constexpr int kGroups = kTX / 4;          // 4-column groups of the horizontal pass
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;
static_assert(kHY * kGroups <= kLossThreads, "one lane per (row, 4-column group) of the horizontal pass");
static_assert(kTX * kTY == 2 * kLossThreads, "the vertical pass gives every lane two pixels");

// g[i] = exp(-(i - 5)^2 / 4.5) / sum, computed in double, rounded to float (loss.py, gaussian_window)
#define MS_GAUSS11                                                                                                   \
    {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f, 0x1.b43c4p-3f, \
     0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f}

template <int C>
struct LossCfg {
    static constexpr int S = (kHX * C) | 1;     // floats between staged rows of x / y (odd)
    static constexpr int RW = kHX * C;          // floats of a staged row
    static constexpr int TW = kTX * C;          // floats of a row of the tile itself
};

struct SsimPoint {
    float ssim, a, b, c;   // a = d ssim / d mu_x at fixed w*x^2 and w*xy, b = d ssim / d s_xx, c = d ssim / d s_xy
};

__device__ __forceinline__ SsimPoint ssim_point(float mx, float my, float exx, float eyy, float exy) {
#pragma clang fp contract(off)
    const float p = mx * my, q = mx * mx, r = my * my;
    const float sxx = exx - q, syy = eyy - r, sxy = exy - p;
    const float A1 = 2.f * p + kC1, A2 = 2.f * sxy + kC2, B1 = (q + r) + kC1, B2 = (sxx + syy) + kC2;
    SsimPoint o;
    o.ssim = (A1 * A2) / (B1 * B2);
    // The derivatives through the two ratios: for x == y (A1 == B1, A2 == B2 bit for bit) r1 = r2 = 1, so c = -2 b and
    // a = 0 EXACTLY, and the backward's sum cancels to an exactly zero gradient at the optimum.
    const float r1 = A1 / B1, r2 = A2 / B2, t = r1 / B2;
    o.b = -(t * r2);
    o.c = 2.f * t;
    const float at_fixed_s = 2.f * r2 * (my - mx * r1) / B1;
    o.a = at_fixed_s - (2.f * mx * o.b + my * o.c);
    return o;
}

// w*a + 2 x (w*b) + y (w*c), each product rounded on its own (see ssim_point: exact cancellation for x == y)
__device__ __forceinline__ float ssim_grad_sum(float wa, float wb, float wc, float xv, float yv) {
#pragma clang fp contract(off)
    return wa + (2.f * xv * wb + yv * wc);
}

// Sum of v over the workgroup's 256 lanes in a fixed order; the total is returned to thread 0 (other lanes: unspecified).
__device__ __forceinline__ float block_sum(float v, float *s_red4) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_red4[0] + s_red4[1]) + s_red4[2]) + s_red4[3];
}

template <int C, bool KEEP>
__global__ void __launch_bounds__(kLossThreads, 3)
k_loss_fwd(int B, int H, int W, const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ partials,
           float *__restrict__ maps) {
    using Cfg = LossCfg<C>;
    __shared__ float s_x[kHY * Cfg::S], s_y[kHY * Cfg::S];
    __shared__ float s_h[5 * kHY * kHS];
    __shared__ float s_red[2][4];
    const float g[11] = MS_GAUSS11;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY, b = blockIdx.z;
    const int rowf = W * C;

    for (int i = tid; i < kHY * Cfg::RW; i += kLossThreads) {
        const int r = i / Cfg::RW, j = i - r * Cfg::RW;
        const int gy = y0 - kR + r, gj = (x0 - kR) * C + j;
        float vx = 0.f, vy = 0.f;
        if (gy >= 0 && gy < H && gj >= 0 && gj < rowf) {
            const int o = (b * H + gy) * rowf + gj;
            vx = x[o];
            vy = y[o];
        }
        s_x[r * Cfg::S + j] = vx;
        s_y[r * Cfg::S + j] = vy;
    }
    __syncthreads();

    float sum_l1 = 0.f, sum_ssim = 0.f;
    const int col = tid & (kTX - 1), ry0 = (tid >> 5) * 2;
    const size_t plane = (size_t)H * W;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (c) __syncthreads();   // the previous channel's vertical pass has read s_h
        if (tid < kHY * kGroups) {
            const int r = tid % kHY, gq = tid / kHY;
            const float *px = s_x + r * Cfg::S + gq * 4 * C + c, *py = s_y + r * Cfg::S + gq * 4 * C + c;
            float vx[14], vy[14], vxx[14], vyy[14], vxy[14];
#pragma unroll
            for (int k = 0; k < 14; ++k) {
                vx[k] = px[k * C];
                vy[k] = py[k * C];
                vxx[k] = vx[k] * vx[k];
                vyy[k] = vy[k] * vy[k];
                vxy[k] = vx[k] * vy[k];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float mx = 0.f, my = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
                for (int t = 0; t < 11; ++t) {
                    mx = fmaf(g[t], vx[j + t], mx);
                    my = fmaf(g[t], vy[j + t], my);
                    exx = fmaf(g[t], vxx[j + t], exx);
                    eyy = fmaf(g[t], vyy[j + t], eyy);
                    exy = fmaf(g[t], vxy[j + t], exy);
                }
                float *h = s_h + r * kHS + gq * 4 + j;
                h[0 * kHY * kHS] = mx;
                h[1 * kHY * kHS] = my;
                h[2 * kHY * kHS] = exx;
                h[3 * kHY * kHS] = eyy;
                h[4 * kHY * kHS] = exy;
            }
        }
        __syncthreads();
        float acc[2][5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            float h[12];
#pragma unroll
            for (int t = 0; t < 12; ++t) h[t] = s_h[(k * kHY + ry0 + t) * kHS + col];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float a = 0.f;
#pragma unroll
                for (int t = 0; t < 11; ++t) a = fmaf(g[t], h[j + t], a);
                acc[j][k] = a;
            }
        }
        const int gx = x0 + col;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gy = y0 + ry0 + j;
            if (gx < W && gy < H) {
                const SsimPoint sp = ssim_point(acc[j][0], acc[j][1], acc[j][2], acc[j][3], acc[j][4]);
                const int e = (ry0 + j + kR) * Cfg::S + (col + kR) * C + c;
                sum_l1 += fabsf(s_x[e] - s_y[e]);
                sum_ssim += sp.ssim;
                if (KEEP) {
                    const size_t o = ((size_t)b * C + c) * plane + (size_t)gy * W + gx;
                    const size_t mstride = (size_t)B * C * plane;
                    maps[o] = sp.a;
                    maps[o + mstride] = sp.b;
                    maps[o + 2 * mstride] = sp.c;
                }
            }
        }
    }
    const float t_l1 = block_sum(sum_l1, s_red[0]);
    const float t_ssim = block_sum(sum_ssim, s_red[1]);
    if (tid == 0) {
        const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partials[2 * blk] = t_l1;
        partials[2 * blk + 1] = t_ssim;
    }
}

// One workgroup: lane t adds rows t, t + 256, ... in that order, then the 256 lane totals are added as a fixed tree.
__global__ void __launch_bounds__(kLossThreads)
k_loss_finalize(const float *__restrict__ partials, int64_t rows, double n, double lambda, float *__restrict__ out3) {
    __shared__ double s_a[kLossThreads], s_b[kLossThreads];
    const int tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int64_t i = tid; i < rows; i += kLossThreads) {
        a += (double)partials[2 * i];
        b += (double)partials[2 * i + 1];
    }
    s_a[tid] = a;
    s_b[tid] = b;
    __syncthreads();
    for (int half = kLossThreads / 2; half >= 1; half >>= 1) {
        if (tid < half) {
            s_a[tid] += s_a[tid + half];
            s_b[tid] += s_b[tid + half];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double l1 = s_a[0] / n, ssim = s_b[0] / n;   // (a division: identical images give exactly 1)
        out3[0] = (float)((1.0 - lambda) * l1 + lambda * (1.0 - ssim));
        out3[1] = (float)l1;
        out3[2] = (float)ssim;
    }
}

template <int C>
__global__ void __launch_bounds__(kLossThreads, 4)
k_loss_bwd(int B, int H, int W, const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ maps,
           const float *__restrict__ v_loss, float coef_l1, float coef_ssim, float *__restrict__ v_img) {
    using Cfg = LossCfg<C>;
    __shared__ float s_m[3 * kHY * kMS];
    __shared__ float s_h[3 * kHY * kHS];
    __shared__ float s_xt[kTY * Cfg::TW], s_yt[kTY * Cfg::TW];   // the tile's x (then its gradient) and y
    const float g[11] = MS_GAUSS11;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY, b = blockIdx.z;
    const int rowf = W * C;

    for (int i = tid; i < kTY * Cfg::TW; i += kLossThreads) {
        const int r = i / Cfg::TW, j = i - r * Cfg::TW;
        const int gy = y0 + r, gj = x0 * C + j;
        float vx = 0.f, vy = 0.f;
        if (gy < H && gj < rowf) {
            const int o = (b * H + gy) * rowf + gj;
            vx = x[o];
            vy = y[o];
        }
        s_xt[i] = vx;
        s_yt[i] = vy;
    }
    const int col = tid & (kTX - 1), ry0 = (tid >> 5) * 2;
    const size_t plane = (size_t)H * W, mstride = (size_t)B * C * plane;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        // (the horizontal pass of the previous channel ended before its second barrier: s_m is free)
        const float *mp = maps + ((size_t)b * C + c) * plane;
        for (int i = tid; i < kHY * kHX; i += kLossThreads) {
            const int r = i / kHX, j = i - r * kHX;
            const int gy = y0 - kR + r, gx = x0 - kR + j;
            const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
            const size_t o = in ? (size_t)gy * W + gx : 0;
#pragma unroll
            for (int m = 0; m < 3; ++m) s_m[(m * kHY + r) * kMS + j] = in ? mp[o + m * mstride] : 0.f;
        }
        __syncthreads();   // also: every lane has left the previous channel's vertical pass (s_h) and staged s_xt / s_yt
        if (tid < kHY * kGroups) {
            const int r = tid % kHY, gq = tid / kHY;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const float *pm = s_m + (m * kHY + r) * kMS + gq * 4;
                float v[14];
#pragma unroll
                for (int k = 0; k < 14; ++k) v[k] = pm[k];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float a = 0.f;
#pragma unroll
                    for (int t = 0; t < 11; ++t) a = fmaf(g[t], v[j + t], a);
                    s_h[(m * kHY + r) * kHS + gq * 4 + j] = a;
                }
            }
        }
        __syncthreads();
        float acc[2][3];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            float h[12];
#pragma unroll
            for (int t = 0; t < 12; ++t) h[t] = s_h[(m * kHY + ry0 + t) * kHS + col];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float a = 0.f;
#pragma unroll
                for (int t = 0; t < 11; ++t) a = fmaf(g[t], h[j + t], a);
                acc[j][m] = a;
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int e = (ry0 + j) * Cfg::TW + col * C + c;   // this lane alone reads and writes element e
            const float xv = s_xt[e], yv = s_yt[e];
            const float d = xv - yv;
            const float sgn = (float)((d > 0.f) - (d < 0.f));
            s_xt[e] = coef_l1 * sgn - coef_ssim * ssim_grad_sum(acc[j][0], acc[j][1], acc[j][2], xv, yv);
        }
    }
    __syncthreads();
    const float vl = *v_loss;
    for (int i = tid; i < kTY * Cfg::TW; i += kLossThreads) {
        const int r = i / Cfg::TW, j = i - r * Cfg::TW;
        const int gy = y0 + r, gj = x0 * C + j;
        if (gy < H && gj < rowf) v_img[(b * H + gy) * rowf + gj] = vl * s_xt[i];
    }
}

struct LossDims {
    int64_t n, rows;        // elements; workgroups of the forward = rows of partial sums
    dim3 grid;
    size_t partial_bytes;   // the planes start here
};

int check_loss(int B, int H, int W, int C, float lambda_dssim, const char *who, LossDims *d) {
    MS_REQUIRE(B > 0 && H > 0 && W > 0, MS_ERR_INVALID_ARG, "%s: non-positive size (B %d, H %d, W %d)", who, B, H, W);
    MS_REQUIRE(C >= 1 && C <= 4, MS_ERR_INVALID_ARG, "%s: C = %d channels, not in [1, 4]", who, C);
    MS_REQUIRE(lambda_dssim >= 0.f && lambda_dssim <= 1.f, MS_ERR_INVALID_ARG, "%s: lambda_dssim %g outside [0, 1]", who,
               (double)lambda_dssim);
    const int64_t hw = (int64_t)H * W;
    MS_REQUIRE(hw <= 0x7fffffff && hw * C <= 0x7fffffff && hw * C * B <= 0x7fffffff, MS_ERR_TOO_LARGE,
               "%s: B H W C exceeds 2^31 - 1 elements (32-bit offsets)", who);
    const int64_t gx = ms::ceil_div(W, kTX), gy = ms::ceil_div(H, kTY);
    MS_REQUIRE(gy <= 65535 && B <= 65535, MS_ERR_TOO_LARGE, "%s: more than 65535 tile rows or images", who);
    d->n = hw * C * B;
    d->rows = gx * gy * B;
    d->grid = dim3((unsigned)gx, (unsigned)gy, (unsigned)B);
    d->partial_bytes = ms::align_up((size_t)d->rows * 2 * sizeof(float), 256);
    return MS_OK;
}

template <int C>
int launch_fwd(const LossDims &d, int B, int H, int W, const float *x, const float *y, float *partials, float *maps,
               hipStream_t stream) {
    if (maps)
        hipLaunchKernelGGL((k_loss_fwd<C, true>), d.grid, dim3(kLossThreads), 0, stream, B, H, W, x, y, partials, maps);
    else
        hipLaunchKernelGGL((k_loss_fwd<C, false>), d.grid, dim3(kLossThreads), 0, stream, B, H, W, x, y, partials, maps);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

}  // namespace

extern "C" size_t ms_photometric_loss_workspace_bytes(int B, int H, int W, int C, int keep_for_backward) {
    LossDims d;
    if (check_loss(B, H, W, C, 0.f, "photometric_loss_workspace_bytes", &d)) return 0;
    return d.partial_bytes + (keep_for_backward ? (size_t)d.n * 3 * sizeof(float) : 0);
}

extern "C" int ms_photometric_loss_fwd(int B, int H, int W, int C, const float *img, const float *target,
                                       float lambda_dssim, void *workspace, size_t workspace_bytes, int keep_for_backward,
                                       float *out3, void *stream_) {
    LossDims d;
    if (int rc = check_loss(B, H, W, C, lambda_dssim, "photometric_loss_fwd", &d)) return rc;
    MS_REQUIRE(img && target && workspace && out3, MS_ERR_INVALID_ARG, "photometric_loss_fwd: null pointer");
    const size_t need = d.partial_bytes + (keep_for_backward ? (size_t)d.n * 3 * sizeof(float) : 0);
    MS_REQUIRE(workspace_bytes >= need, MS_ERR_WORKSPACE, "photometric_loss_fwd: workspace of %zu bytes, needs %zu",
               workspace_bytes, need);
    hipStream_t stream = (hipStream_t)stream_;
    float *partials = (float *)workspace;
    float *maps = keep_for_backward ? (float *)((char *)workspace + d.partial_bytes) : nullptr;
    int rc;
    switch (C) {
        case 1: rc = launch_fwd<1>(d, B, H, W, img, target, partials, maps, stream); break;
        case 2: rc = launch_fwd<2>(d, B, H, W, img, target, partials, maps, stream); break;
        case 3: rc = launch_fwd<3>(d, B, H, W, img, target, partials, maps, stream); break;
        default: rc = launch_fwd<4>(d, B, H, W, img, target, partials, maps, stream); break;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(k_loss_finalize, dim3(1), dim3(kLossThreads), 0, stream, (const float *)partials, d.rows,
                       (double)d.n, (double)lambda_dssim, out3);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

extern "C" int ms_photometric_loss_bwd(int B, int H, int W, int C, const float *img, const float *target,
                                       float lambda_dssim, const void *workspace, size_t workspace_bytes,
                                       const float *v_loss, float *v_img, void *stream_) {
    LossDims d;
    if (int rc = check_loss(B, H, W, C, lambda_dssim, "photometric_loss_bwd", &d)) return rc;
    MS_REQUIRE(img && target && workspace && v_loss && v_img, MS_ERR_INVALID_ARG, "photometric_loss_bwd: null pointer");
    const size_t need = d.partial_bytes + (size_t)d.n * 3 * sizeof(float);
    MS_REQUIRE(workspace_bytes >= need, MS_ERR_WORKSPACE,
               "photometric_loss_bwd: workspace of %zu bytes, needs %zu (a forward with keep_for_backward)", workspace_bytes,
               need);
    hipStream_t stream = (hipStream_t)stream_;
    const float *maps = (const float *)((const char *)workspace + d.partial_bytes);
    const float coef_l1 = (float)((1.0 - (double)lambda_dssim) / (double)d.n);
    const float coef_ssim = (float)((double)lambda_dssim / (double)d.n);
    switch (C) {
        case 1: hipLaunchKernelGGL((k_loss_bwd<1>), d.grid, dim3(kLossThreads), 0, stream, B, H, W, img, target, maps, v_loss, coef_l1, coef_ssim, v_img); break;
        case 2: hipLaunchKernelGGL((k_loss_bwd<2>), d.grid, dim3(kLossThreads), 0, stream, B, H, W, img, target, maps, v_loss, coef_l1, coef_ssim, v_img); break;
        case 3: hipLaunchKernelGGL((k_loss_bwd<3>), d.grid, dim3(kLossThreads), 0, stream, B, H, W, img, target, maps, v_loss, coef_l1, coef_ssim, v_img); break;
        default: hipLaunchKernelGGL((k_loss_bwd<4>), d.grid, dim3(kLossThreads), 0, stream, B, H, W, img, target, maps, v_loss, coef_l1, coef_ssim, v_img); break;
    }
    MS_LAUNCH_CHECK();
    return MS_OK;
}
