// Bilateral-grid colour correction (gsplat's `use_bilateral_grid`; with a 1 x 1 x 1 grid: 3DGS's per-image exposure matrix),
// fused: out = A(y, x, gray) * (r, g, b, 1), A the 3 x 4 matrix interpolated trilinearly from a (12, L, Gh, Gw) grid at
// (z, v, u) = (gray (L - 1), (y + 0.5) / H (Gh - 1), (x + 0.5) / W (Gw - 1)), and the total-variation loss of the grids.
// mojosplat_amd/bilagrid.py holds the definitions (bilagrid_slice_torch, bilagrid_tv_loss_torch); nothing in the reference
// corrects colours.
//
// SLICE FORWARD, k_slice_tile<false>: a workgroup of 256 lanes owns 32 x 16 pixels of one image, a lane two pixels of one
// column.  The tile's colours come in and the result goes out through LDS, as whole runs of 96 floats of an (H, W, 3) row
// (16 bytes a lane where W % 4 == 0 and the bases are 16-byte aligned, dwords otherwise).
// The vertices its pixels can touch -- the u / v vertex range of its first and last column and row, times L levels, times
// 12 coefficients -- are staged in LDS, transposed so that the 12 coefficients of a vertex are three 16-byte reads; at
// 1920 x 1080 under 16 x 16 x 8 that is 2 x 2 x 8 x 12 = 384 floats (at most 3 x 3 x 8 x 12).  A tile whose footprint
// exceeds kFootMax floats (a small image under a dense grid: the tile spans many cells) reads its vertices from global
// memory instead; the choice is per workgroup, from the footprint's own size.
// SLICE BACKWARD, image: k_slice_tile<true>, the same pass with v_out staged next to the colours:
//   v_img_j = sum_i A[4 i + j] v_out_i + [0 < z < L - 1] (L - 1) (sum_c dA_c/df_z g_c) * (0.299, 0.587, 0.114)_j,
//   g_{4 i + j} = v_out_i rgb_j, g_{4 i + 3} = v_out_i        (nothing flows into u and v: pixel positions are constants).
// SLICE BACKWARD, grids: a vertex-centred gather, no float atomics.  k_slice_gather: workgroup (b, vertex (gy, gx), chunk s
// of 32 pixel rows, 8 levels) walks the pixels of the vertex's up to four adjacent cells -- a rectangle that follows from the
// geometry, taken two pixels too wide: a pixel's weight on the vertex is evaluated by the definition itself and is an exact
// zero outside the cells -- as 16 x 16 lanes: a lane owns two rows, walks the columns 16 at a time and keeps 8 x 12 sums
// over its own pixels, in pixel order, as 48 register pairs (packed multiply-adds); the lanes' sums are added by a halving
// butterfly across a wave (wave_reduce) and the four waves in wave order, into the workspace slab
// [b][vertex][chunk][level][12].  The kernel is VALU-bound: a pixel is visited by its four vertices, for 8 levels each.
// k_slice_sum adds a grid element's chunks in ascending order and writes EVERY element of v_grids (exact zeros where no pixel
// reaches).  Every sum's order is fixed by the shapes alone: the same inputs give the same bits.
// TV LOSS: k_tv_fwd gives per-workgroup sums of the squared neighbour differences along x, y and z (one lane: four elements
// along Gw, 16-byte loads, where Gw is a multiple of 4 and the base is aligned), k_tv_finalize adds them in a fixed order in
// double (the pattern of k_loss_fwd / k_loss_finalize); k_tv_bwd writes v_loss * d tv / d grids from the grids in one launch.
//
// Bytes (I = 12 B H W, one image): forward 2 I + the grids; backward, image: 3 I; backward, grids: every pixel is read by
// its four neighbouring vertices (times ceil(L / 8)): 4 x 2 I out of L2, plus the slab.
// Pixel offsets are 64-bit.  gray = (0.299 r + 0.587 g) + 0.114 b with separately rounded products and sums (no contraction).
#include "ms_common.hpp"

namespace {

constexpr int kTX = 32, kTY = 16;         // the pixels of a workgroup of the tile kernel
constexpr int kThreads = 256;
constexpr int kTW = kTX * 3;              // floats of a tile row
constexpr int kFootMax = 2048;            // floats of LDS for a tile's vertex footprint (8 KiB)
constexpr int kGatherRows = 32;           // pixel rows per chunk of the gather
constexpr int kMaxExtent = 1 << 23;       // (x + 0.5f) is exact below this
static_assert(kTX * kTY == 2 * kThreads, "a lane owns two pixels of a column");

struct Axis {
    int i0, step;   // the lower vertex; 1, or 0 on an axis of size 1 (both weights then fall on vertex 0: 1 and 0)
    float f;        // weights (1 - f, f) on (i0, i0 + step)
};

__device__ __forceinline__ Axis axis_of(float t, int n) {
    Axis a;
    if (n == 1) {
        a.i0 = 0, a.step = 0, a.f = 0.f;
        return a;
    }
    const float tc = fminf(fmaxf(t, 0.f), (float)(n - 1));
    a.i0 = min((int)floorf(tc), n - 2);
    a.step = 1;
    a.f = tc - (float)a.i0;
    return a;
}

// the weight of vertex g under a
__device__ __forceinline__ float weight_on(const Axis &a, int g) {
    return a.i0 == g ? 1.f - a.f : (a.step && a.i0 + 1 == g) ? a.f : 0.f;
}

__device__ __forceinline__ float coord_of(int p, int n_pix, int n_grid) {
    return ((float)p + 0.5f) / (float)n_pix * (float)(n_grid - 1);
}

__device__ __forceinline__ float gray_of(float r, float g, float b) {
#pragma clang fp contract(off)
    const float pr = r * 0.299f, pg = g * 0.587f, pb = b * 0.114f;
    return (pr + pg) + pb;
}

// Sum of v over the workgroup's 256 lanes in a fixed order, valid in thread 0.
__device__ __forceinline__ float block_sum(float v, float *s_red4) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_red4[0] + s_red4[1]) + s_red4[2]) + s_red4[3];
}

template <bool BWD>
__global__ void __launch_bounds__(kThreads, 6)
k_slice_tile(int H, int W, int L, int Gh, int Gw, const float *__restrict__ grids, const float *__restrict__ img,
             const float *__restrict__ v_out, float *__restrict__ out, int vec) {
    __shared__ __align__(16) float s_foot[kFootMax];
    __shared__ __align__(16) float s_img[kTY * kTW];   // the tile's colours, then its result
    __shared__ __align__(16) float s_vo[BWD ? kTY * kTW : 4];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY, b = blockIdx.z;
    const size_t rowf = (size_t)W * 3, base = (size_t)b * H * rowf;
    const size_t plane = (size_t)Gh * Gw;
    const float *gb = grids + (size_t)b * 12 * L * plane;

    if (vec) {   // rows of W * 3 floats with W % 4 == 0 from 16-byte aligned bases: a float4 is inside the row or outside it
        for (int i = tid; i < kTY * kTW / 4; i += kThreads) {
            const int r = i / (kTW / 4), j = (i - r * (kTW / 4)) * 4;
            const int gy = y0 + r;
            const size_t gj = (size_t)x0 * 3 + j;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f), vo = v;
            if (gy < H && gj < rowf) {
                const size_t o = base + (size_t)gy * rowf + gj;
                v = *(const float4 *)(img + o);
                if (BWD) vo = *(const float4 *)(v_out + o);
            }
            *(float4 *)(s_img + r * kTW + j) = v;
            if (BWD) *(float4 *)(s_vo + r * kTW + j) = vo;
        }
    } else {
        for (int i = tid; i < kTY * kTW; i += kThreads) {
            const int r = i / kTW, j = i - r * kTW;
            const int gy = y0 + r;
            const size_t gj = (size_t)x0 * 3 + j;
            float v = 0.f, vo = 0.f;
            if (gy < H && gj < rowf) {
                const size_t o = base + (size_t)gy * rowf + gj;
                v = img[o];
                if (BWD) vo = v_out[o];
            }
            s_img[i] = v;
            if (BWD) s_vo[i] = vo;
        }
    }
    // the footprint: vertices [fx0, fx0 + nfx) x [fy0, fy0 + nfy) x all levels (coordinates are monotone in the pixel index)
    const int xl = min(x0 + kTX, W) - 1, yl = min(y0 + kTY, H) - 1;
    const Axis ax_a = axis_of(coord_of(x0, W, Gw), Gw), ax_b = axis_of(coord_of(xl, W, Gw), Gw);
    const Axis ay_a = axis_of(coord_of(y0, H, Gh), Gh), ay_b = axis_of(coord_of(yl, H, Gh), Gh);
    const int fx0 = ax_a.i0, nfx = ax_b.i0 + ax_b.step - fx0 + 1;
    const int fy0 = ay_a.i0, nfy = ay_b.i0 + ay_b.step - fy0 + 1;
    const long long nfoot = (long long)nfx * nfy * L * 12;
    const bool foot = nfoot <= kFootMax;               // the same for the whole workgroup
    if (foot) {
        for (int i = tid; i < (int)nfoot; i += kThreads) {
            const int fx = i % nfx;
            int t = i / nfx;
            const int fy = t % nfy;
            t /= nfy;
            const int l = t % L, c = t / L;
            s_foot[((fy * nfx + fx) * L + l) * 12 + c] = gb[((size_t)c * L + l) * plane + (size_t)(fy0 + fy) * Gw + fx0 + fx];
        }
    }
    __syncthreads();

    const int col = tid & (kTX - 1), ry0 = (tid >> 5) * 2;
    const Axis ax = axis_of(coord_of(min(x0 + col, W - 1), W, Gw), Gw);   // (a lane past the image's edge computes its neighbour)
    const float zscale = (float)(L - 1);
    const size_t cstride = (size_t)L * plane;
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {   // (one pixel after the other: half the registers)
        const int row = ry0 + j;
        const Axis ay = axis_of(coord_of(min(y0 + row, H - 1), H, Gh), Gh);
        const int e = row * kTW + col * 3;              // this lane alone reads and writes elements e .. e + 2
        const float r = s_img[e], g = s_img[e + 1], bl = s_img[e + 2];
        const float z = gray_of(r, g, bl) * zscale;
        const Axis az = axis_of(z, L);
        float A[12], D[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) A[c] = 0.f, D[c] = 0.f;
#pragma unroll 1
        for (int yy = 0; yy < 2; ++yy) {   // (a vertex pair at a time: its 24 coefficients are what is in flight)
#pragma unroll 1
            for (int xx = 0; xx < 2; ++xx) {
                const float wxy = (yy ? ay.f : 1.f - ay.f) * (xx ? ax.f : 1.f - ax.f);
                const int iy = ay.i0 + yy * ay.step, ix = ax.i0 + xx * ax.step;
                float G0[12], G1[12];
                if (foot) {
                    const float4 *p0 = (const float4 *)(s_foot + (((iy - fy0) * nfx + (ix - fx0)) * L + az.i0) * 12);
                    const float4 *p1 = p0 + 3 * az.step;
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const float4 a = p0[q], d = p1[q];
                        G0[4 * q] = a.x, G0[4 * q + 1] = a.y, G0[4 * q + 2] = a.z, G0[4 * q + 3] = a.w;
                        G1[4 * q] = d.x, G1[4 * q + 1] = d.y, G1[4 * q + 2] = d.z, G1[4 * q + 3] = d.w;
                    }
                } else {
                    const float *p0 = gb + (size_t)az.i0 * plane + (size_t)iy * Gw + ix;
                    const float *p1 = p0 + (size_t)az.step * plane;
#pragma unroll
                    for (int c = 0; c < 12; ++c) G0[c] = p0[c * cstride];
#pragma unroll
                    for (int c = 0; c < 12; ++c) G1[c] = p1[c * cstride];
                }
                const float w0 = wxy * (1.f - az.f), w1 = wxy * az.f;
#pragma unroll
                for (int c = 0; c < 12; ++c) {
                    A[c] = fmaf(w0, G0[c], A[c]);
                    A[c] = fmaf(w1, G1[c], A[c]);
                    if (BWD) D[c] = fmaf(wxy, G1[c] - G0[c], D[c]);
                }
            }
        }
        if (!BWD) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
                s_img[e + i] = fmaf(A[4 * i], r, fmaf(A[4 * i + 1], g, fmaf(A[4 * i + 2], bl, A[4 * i + 3])));
        } else {
            const float v0 = s_vo[e], v1 = s_vo[e + 1], v2 = s_vo[e + 2];
            float gr = fmaf(A[0], v0, fmaf(A[4], v1, A[8] * v2));
            float gg = fmaf(A[1], v0, fmaf(A[5], v1, A[9] * v2));
            float gbl = fmaf(A[2], v0, fmaf(A[6], v1, A[10] * v2));
            if (L > 1 && z > 0.f && z < zscale) {       // grid_sample's border rule: nothing through a clamped guidance
                float s = 0.f;
                const float vo[3] = {v0, v1, v2};
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    s = fmaf(vo[i], fmaf(D[4 * i], r, fmaf(D[4 * i + 1], g, fmaf(D[4 * i + 2], bl, D[4 * i + 3]))), s);
                s *= zscale;
                gr = fmaf(s, 0.299f, gr);
                gg = fmaf(s, 0.587f, gg);
                gbl = fmaf(s, 0.114f, gbl);
            }
            s_img[e] = gr, s_img[e + 1] = gg, s_img[e + 2] = gbl;
        }
    }
    __syncthreads();
    if (vec) {
        for (int i = tid; i < kTY * kTW / 4; i += kThreads) {
            const int r = i / (kTW / 4), j = (i - r * (kTW / 4)) * 4;
            const int gy = y0 + r;
            const size_t gj = (size_t)x0 * 3 + j;
            if (gy < H && gj < rowf) *(float4 *)(out + base + (size_t)gy * rowf + gj) = *(const float4 *)(s_img + r * kTW + j);
        }
    } else {
        for (int i = tid; i < kTY * kTW; i += kThreads) {
            const int r = i / kTW, j = i - r * kTW;
            const int gy = y0 + r;
            const size_t gj = (size_t)x0 * 3 + j;
            if (gy < H && gj < rowf) out[base + (size_t)gy * rowf + gj] = s_img[i];
        }
    }
}

// The pixels [lo, hi) that can have a weight on vertex g of an axis of n_grid vertices over n_pix pixels: those whose
// coordinate lies in (g - 1, g + 1), two pixels more on either side (the coordinate's own rounding is far below one pixel).
__host__ __device__ inline void vertex_reach(int g, int n_grid, int n_pix, int *lo, int *hi) {
    if (n_grid == 1) {
        *lo = 0, *hi = n_pix;
        return;
    }
    const long long d = n_grid - 1;
    const long long a = ((long long)(g - 1) * n_pix) / d - 2, e = ((long long)(g + 1) * n_pix) / d + 3;
    *lo = (int)(a < 0 ? 0 : a);
    *hi = (int)(e > n_pix ? n_pix : e);
}

// an upper bound of hi - lo over the vertices of an axis
inline int max_reach(int n_grid, int n_pix) {
    if (n_grid == 1) return n_pix;
    const long long m = 2ll * n_pix / (n_grid - 1) + 7;
    return (int)(m < n_pix ? m : n_pix);
}

// Sums v[0 .. N) over the 64 lanes of a wave, step OFF = 32, 16, ... 1.  While N is even a step HALVES the values a lane
// carries: the lanes whose bit OFF is set keep the upper half, the others the lower half, and each receives its partner's
// sums of the half it keeps (N / 2 exchanges, not N).  Once N is odd the steps add all N values across.  Returns the index of
// v[0] among the original N; the order of every sum is fixed by the lane numbers alone.
template <int N, int OFF>
__device__ __forceinline__ int wave_reduce(float *v, int lane) {
    if constexpr (OFF == 0) {
        return 0;
    } else if constexpr (N % 2 == 0) {
        const bool hi = (lane & OFF) != 0;
#pragma unroll
        for (int k = 0; k < N / 2; ++k) {
            const float send = hi ? v[k] : v[k + N / 2], keep = hi ? v[k + N / 2] : v[k];
            v[k] = keep + __shfl_xor(send, OFF, 64);
        }
        return (hi ? N / 2 : 0) + wave_reduce<N / 2, OFF / 2>(v, lane);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] += __shfl_xor(v[k], OFF, 64);
        return wave_reduce<N, OFF / 2>(v, lane);
    }
}
// what wave_reduce<N, 32> leaves: values per lane, and the lane bits of the steps that halved nothing (lanes that differ
// only in those hold the same sums: the one with all of them clear stores)
constexpr int reduced_count(int n, int off) { return off == 0 ? n : reduced_count(n % 2 == 0 ? n / 2 : n, off / 2); }
constexpr int plain_steps(int n, int off) { return off == 0 ? 0 : (n % 2 == 0 ? 0 : off) | plain_steps(n % 2 == 0 ? n / 2 : n, off / 2); }

struct GatherPixel {
    float r, g, b, v0, v1, v2;
};
typedef float f32x2 __attribute__((ext_vector_type(2)));   // (two sums a register pair: packed fp32 multiply-adds)

// One pixel's share of the LC levels from l0 on: acc[l][c] += wxy * weight_l(z) * v_out_i * (rgb_j or 1), c = 4 i + j
template <int LC>
__device__ __forceinline__ void gather_add(f32x2 *acc, const GatherPixel &c, float wxy, float zscale, int L, int l0) {
    const Axis az = axis_of(gray_of(c.r, c.g, c.b) * zscale, L);
    const float w0 = wxy * (1.f - az.f), w1 = wxy * az.f;      // on levels i0 and i0 + 1 (one level: f = 0)
    const int d0 = az.i0 - l0;
    const f32x2 g2[6] = {{c.v0 * c.r, c.v0 * c.g}, {c.v0 * c.b, c.v0}, {c.v1 * c.r, c.v1 * c.g},
                         {c.v1 * c.b, c.v1},       {c.v2 * c.r, c.v2 * c.g}, {c.v2 * c.b, c.v2}};
#pragma unroll
    for (int l = 0; l < LC; ++l) {
        const float w = l == d0 ? w0 : l == d0 + 1 ? w1 : 0.f;
        const f32x2 w2 = {w, w};
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[l * 6 + k] = __builtin_elementwise_fma(w2, g2[k], acc[l * 6 + k]);
    }
}

// A workgroup is 16 columns x 16 rows of lanes: a lane owns rows r0 + ty and r0 + ty + 16 of its chunk (their weights are
// computed once) and walks the reach's columns 16 at a time, the next column's two pixels loaded while the current two are
// added.  Lanes past the reach's edge or the chunk's last row load the edge pixel and add it with weight zero.
template <int LC>
__global__ void __launch_bounds__(kThreads, 3)
k_slice_gather(int H, int W, int L, int Gh, int Gw, int S, int NL, const float *__restrict__ img,
               const float *__restrict__ v_out, float *__restrict__ slab) {
    constexpr int N = LC * 12;
    static_assert(kGatherRows == 32, "two rows a lane");
    __shared__ float s_red[4][N];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int vert = blockIdx.x, gy = vert / Gw, gx = vert - gy * Gw;
    const int s = blockIdx.y / NL, lc = blockIdx.y - s * NL, b = blockIdx.z;
    int xlo, xhi, ylo, yhi;
    vertex_reach(gx, Gw, W, &xlo, &xhi);
    vertex_reach(gy, Gh, H, &ylo, &yhi);
    const int r0 = min(ylo + s * kGatherRows, yhi), r1 = min(r0 + kGatherRows, yhi);
    const int wreg = xhi - xlo;
    const float zscale = (float)(L - 1);
    const int l0 = lc * LC;

    f32x2 acc[N / 2];
#pragma unroll
    for (int k = 0; k < N / 2; ++k) acc[k] = f32x2{0.f, 0.f};
    if (r1 > r0 && wreg > 0) {           // (the same for the whole workgroup)
        const int ya = r0 + ty, yb = ya + 16;
        const float wya = ya < r1 ? weight_on(axis_of(coord_of(ya, H, Gh), Gh), gy) : 0.f;
        const float wyb = yb < r1 ? weight_on(axis_of(coord_of(yb, H, Gh), Gh), gy) : 0.f;
        const size_t base = (size_t)b * H * W * 3;
        const size_t rowa = base + (size_t)min(ya, r1 - 1) * W * 3, rowb = base + (size_t)min(yb, r1 - 1) * W * 3;
        auto load = [&](size_t row, int x) {
            const size_t o = row + (size_t)x * 3;
            GatherPixel q;
            q.r = img[o], q.g = img[o + 1], q.b = img[o + 2];
            q.v0 = v_out[o], q.v1 = v_out[o + 1], q.v2 = v_out[o + 2];
            return q;
        };
        const int xfirst = min(xlo + tx, xhi - 1);
        GatherPixel qa = load(rowa, xfirst), qb = load(rowb, xfirst);
        for (int xb = 0; xb < wreg; xb += 16) {
            const int x = xlo + xb + tx;
            const GatherPixel ca = qa, cb = qb;
            if (xb + 16 < wreg) {
                const int xn = min(x + 16, xhi - 1);
                qa = load(rowa, xn), qb = load(rowb, xn);
            }
            const float wx = x < xhi ? weight_on(axis_of(coord_of(x, W, Gw), Gw), gx) : 0.f;
            gather_add<LC>(acc, ca, wya * wx, zscale, L, l0);
            gather_add<LC>(acc, cb, wyb * wx, zscale, L, l0);
        }
    }
    float v[N];
#pragma unroll
    for (int k = 0; k < N / 2; ++k) v[2 * k] = acc[k].x, v[2 * k + 1] = acc[k].y;
    const int lane = tid & 63;
    const int first = wave_reduce<N, 32>(v, lane);
    constexpr int M = reduced_count(N, 32), kSame = plain_steps(N, 32);
    if ((lane & kSame) == 0) {
#pragma unroll
        for (int k = 0; k < M; ++k) s_red[tid >> 6][first + k] = v[k];
    }
    __syncthreads();
    if (tid < N) {
        const size_t nv = (size_t)Gh * Gw;
        const size_t slot = ((((size_t)b * nv + vert) * S + s) * NL + lc) * N;
        slab[slot + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
    }
}

// v_grids[b][c][l][gy][gx] = the chunks of (b, vertex) at (level l, coefficient c), added in ascending chunk order
__global__ void __launch_bounds__(kThreads)
k_slice_sum(int64_t total, int L, int Gh, int Gw, int S, int NL, int LC, const float *__restrict__ slab,
            float *__restrict__ v_grids) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int64_t nv = (int64_t)Gh * Gw;
    const int64_t vert = i % nv;
    int64_t t = i / nv;
    const int l = (int)(t % L);
    t /= L;
    const int c = (int)(t % 12);
    const int64_t b = t / 12;
    const int lc = l / LC, li = l - lc * LC;
    const float *p = slab + (((size_t)(b * nv + vert) * S) * NL + lc) * (LC * 12) + li * 12 + c;
    const size_t step = (size_t)NL * LC * 12;
    float v = 0.f;
    for (int s = 0; s < S; ++s) v += p[s * step];
    v_grids[i] = v;
}

// ------------------------------------------------------------------ total variation
struct TvIndex {
    int x, y, l;
};

__device__ __forceinline__ TvIndex tv_index(int64_t e, int L, int Gh, int Gw) {
    TvIndex q;
    q.x = (int)(e % Gw);
    int64_t t = e / Gw;
    q.y = (int)(t % Gh);
    t /= Gh;
    q.l = (int)(t % L);
    return q;
}

template <int V>
__device__ __forceinline__ void tv_load(const float *p, float *v) {
    if constexpr (V == 4) {
        const float4 a = *(const float4 *)p;
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    } else {
        v[0] = *p;
    }
}

// V elements along Gw per lane (V = 4: Gw % 4 == 0 and a 16-byte aligned base)
template <int V>
__global__ void __launch_bounds__(kThreads)
k_tv_fwd(int64_t items, int L, int Gh, int Gw, const float *__restrict__ grids, float *__restrict__ partials) {
    __shared__ float s_red[3][4];
    const int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    if (it < items) {
        const int64_t e = it * V;
        const TvIndex q = tv_index(e, L, Gh, Gw);
        const int64_t plane = (int64_t)Gh * Gw;
        float a[V + 1], n[V];
        tv_load<V>(grids + e, a);
        a[V] = q.x + V < Gw ? grids[e + V] : a[V - 1];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float d = a[k + 1] - a[k];
            sx = fmaf(d, d, sx);
        }
        if (q.y + 1 < Gh) {
            tv_load<V>(grids + e + Gw, n);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float d = n[k] - a[k];
                sy = fmaf(d, d, sy);
            }
        }
        if (q.l + 1 < L) {
            tv_load<V>(grids + e + plane, n);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float d = n[k] - a[k];
                sz = fmaf(d, d, sz);
            }
        }
    }
    const float tx = block_sum(sx, s_red[0]), ty = block_sum(sy, s_red[1]), tz = block_sum(sz, s_red[2]);
    if (threadIdx.x == 0) {
        partials[3 * (size_t)blockIdx.x] = tx;
        partials[3 * (size_t)blockIdx.x + 1] = ty;
        partials[3 * (size_t)blockIdx.x + 2] = tz;
    }
}

// One workgroup: lane t adds rows t, t + 256, ... in that order, then the 256 lane totals are added as a fixed tree.
__global__ void __launch_bounds__(kThreads)
k_tv_finalize(const float *__restrict__ partials, int64_t rows, double cx, double cy, double cz, float *__restrict__ out1) {
    __shared__ double s_a[kThreads];
    const int tid = threadIdx.x;
    double a = 0.0;
    for (int64_t i = tid; i < rows; i += kThreads)
        a += (double)partials[3 * i] * cx + (double)partials[3 * i + 1] * cy + (double)partials[3 * i + 2] * cz;
    s_a[tid] = a;
    __syncthreads();
    for (int half = kThreads / 2; half >= 1; half >>= 1) {
        if (tid < half) s_a[tid] += s_a[tid + half];
        __syncthreads();
    }
    if (tid == 0) out1[0] = (float)s_a[0];
}

template <int V>
__global__ void __launch_bounds__(kThreads)
k_tv_bwd(int64_t items, int L, int Gh, int Gw, const float *__restrict__ grids, const float *__restrict__ v_loss, float kx,
         float ky, float kz, float *__restrict__ v_grids) {
    const int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (it >= items) return;
    const int64_t e = it * V;
    const TvIndex q = tv_index(e, L, Gh, Gw);
    const int64_t plane = (int64_t)Gh * Gw;
    const float vl = *v_loss;
    float a[V + 2], n[V], d[V];      // a[1 .. V]: the lane's elements; a[0], a[V + 1]: their neighbours along x (or copies)
    tv_load<V>(grids + e, a + 1);
    a[0] = q.x > 0 ? grids[e - 1] : a[1];
    a[V + 1] = q.x + V < Gw ? grids[e + V] : a[V];
#pragma unroll
    for (int k = 0; k < V; ++k) d[k] = kx * ((a[k + 1] - a[k]) - (a[k + 2] - a[k + 1]));
    if (q.y > 0) {
        tv_load<V>(grids + e - Gw, n);
#pragma unroll
        for (int k = 0; k < V; ++k) d[k] = fmaf(ky, a[k + 1] - n[k], d[k]);
    }
    if (q.y + 1 < Gh) {
        tv_load<V>(grids + e + Gw, n);
#pragma unroll
        for (int k = 0; k < V; ++k) d[k] = fmaf(-ky, n[k] - a[k + 1], d[k]);
    }
    if (q.l > 0) {
        tv_load<V>(grids + e - plane, n);
#pragma unroll
        for (int k = 0; k < V; ++k) d[k] = fmaf(kz, a[k + 1] - n[k], d[k]);
    }
    if (q.l + 1 < L) {
        tv_load<V>(grids + e + plane, n);
#pragma unroll
        for (int k = 0; k < V; ++k) d[k] = fmaf(-kz, n[k] - a[k + 1], d[k]);
    }
    if constexpr (V == 4) {
        *(float4 *)(v_grids + e) = make_float4(vl * d[0], vl * d[1], vl * d[2], vl * d[V - 1]);
    } else {
        v_grids[e] = vl * d[0];
    }
}

// ------------------------------------------------------------------ host
struct SliceDims {
    dim3 tiles;
    int S, NL, LC;          // chunks of pixel rows per vertex, groups of LC levels
    int64_t grid_elems;
    size_t slab_bytes;
};

int check_grid(int B, int L, int Gh, int Gw, const char *who, int64_t *elems) {
    MS_REQUIRE(B > 0 && L > 0 && Gh > 0 && Gw > 0, MS_ERR_INVALID_ARG, "%s: non-positive size (B %d, L %d, Gh %d, Gw %d)", who, B,
               L, Gh, Gw);
    // (each factor is below 2^31: the product of the first three fits 64 bits only after this division)
    const int64_t vol = (int64_t)L * Gh;
    MS_REQUIRE(vol <= 0x7fffffff && vol * Gw <= 0x7fffffff && vol * Gw * 12 <= 0x7fffffff / B, MS_ERR_TOO_LARGE,
               "%s: the grids exceed 2^31 - 1 elements", who);
    *elems = vol * Gw * 12 * B;
    return MS_OK;
}

int check_slice(int B, int H, int W, int L, int Gh, int Gw, const char *who, SliceDims *d) {
    MS_REQUIRE(H > 0 && W > 0, MS_ERR_INVALID_ARG, "%s: non-positive size (H %d, W %d)", who, H, W);
    if (int rc = check_grid(B, L, Gh, Gw, who, &d->grid_elems)) return rc;
    MS_REQUIRE(H <= kMaxExtent && W <= kMaxExtent, MS_ERR_TOO_LARGE, "%s: an image side above 2^23 pixels", who);
    const int64_t gx = ms::ceil_div(W, kTX), gy = ms::ceil_div(H, kTY);
    d->LC = L == 1 ? 1 : 8;
    d->NL = (int)ms::ceil_div(L, d->LC);
    d->S = (int)ms::ceil_div(max_reach(Gh, H), kGatherRows);
    MS_REQUIRE(gy <= 65535 && B <= 65535 && (int64_t)d->S * d->NL <= 65535, MS_ERR_TOO_LARGE,
               "%s: more than 65535 tile rows, images or chunks of a vertex", who);
    d->tiles = dim3((unsigned)gx, (unsigned)gy, (unsigned)B);
    d->slab_bytes = (size_t)B * Gh * Gw * d->S * d->NL * d->LC * 12 * sizeof(float);
    return MS_OK;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" size_t ms_bilagrid_slice_workspace_bytes(int B, int H, int W, int L, int Gh, int Gw) {
    SliceDims d;
    if (check_slice(B, H, W, L, Gh, Gw, "bilagrid_slice_workspace_bytes", &d)) return 0;
    return d.slab_bytes;
}

extern "C" int ms_bilagrid_slice_fwd(int B, int H, int W, int L, int Gh, int Gw, const float *grids, const float *img,
                                     float *out, void *stream_) {
    SliceDims d;
    if (int rc = check_slice(B, H, W, L, Gh, Gw, "bilagrid_slice_fwd", &d)) return rc;
    MS_REQUIRE(grids && img && out, MS_ERR_INVALID_ARG, "bilagrid_slice_fwd: null pointer");
    hipLaunchKernelGGL((k_slice_tile<false>), d.tiles, dim3(kThreads), 0, (hipStream_t)stream_, H, W, L, Gh, Gw, grids, img,
                       (const float *)nullptr, out, (int)(W % 4 == 0 && aligned16(img) && aligned16(out)));
    MS_LAUNCH_CHECK();
    return MS_OK;
}

extern "C" int ms_bilagrid_slice_bwd(int B, int H, int W, int L, int Gh, int Gw, const float *grids, const float *img,
                                     const float *v_out, void *workspace, size_t workspace_bytes, float *v_grids,
                                     float *v_img, void *stream_) {
    SliceDims d;
    if (int rc = check_slice(B, H, W, L, Gh, Gw, "bilagrid_slice_bwd", &d)) return rc;
    MS_REQUIRE(grids && img && v_out, MS_ERR_INVALID_ARG, "bilagrid_slice_bwd: null pointer");
    MS_REQUIRE(!v_grids || workspace, MS_ERR_INVALID_ARG, "bilagrid_slice_bwd: null pointer (a workspace goes with v_grids)");
    MS_REQUIRE(!v_grids || workspace_bytes >= d.slab_bytes, MS_ERR_WORKSPACE,
               "bilagrid_slice_bwd: workspace of %zu bytes, needs %zu", workspace_bytes, d.slab_bytes);
    hipStream_t stream = (hipStream_t)stream_;
    if (v_img) {
        hipLaunchKernelGGL((k_slice_tile<true>), d.tiles, dim3(kThreads), 0, stream, H, W, L, Gh, Gw, grids, img, v_out, v_img,
                           (int)(W % 4 == 0 && aligned16(img) && aligned16(v_out) && aligned16(v_img)));
        MS_LAUNCH_CHECK();
    }
    if (v_grids) {
        float *slab = (float *)workspace;
        const dim3 grid((unsigned)(Gh * Gw), (unsigned)(d.S * d.NL), (unsigned)B);
        if (d.LC == 1)
            hipLaunchKernelGGL((k_slice_gather<1>), grid, dim3(kThreads), 0, stream, H, W, L, Gh, Gw, d.S, d.NL, img, v_out, slab);
        else
            hipLaunchKernelGGL((k_slice_gather<8>), grid, dim3(kThreads), 0, stream, H, W, L, Gh, Gw, d.S, d.NL, img, v_out, slab);
        MS_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_slice_sum, dim3((unsigned)ms::ceil_div(d.grid_elems, kThreads)), dim3(kThreads), 0, stream,
                           d.grid_elems, L, Gh, Gw, d.S, d.NL, d.LC, (const float *)slab, v_grids);
        MS_LAUNCH_CHECK();
    }
    return MS_OK;
}

extern "C" size_t ms_bilagrid_tv_workspace_bytes(int B, int L, int Gh, int Gw) {
    int64_t elems;
    if (check_grid(B, L, Gh, Gw, "bilagrid_tv_workspace_bytes", &elems)) return 0;
    // (sized for one element per lane: what an unaligned base or a Gw that is no multiple of 4 needs)
    return ms::align_up((size_t)ms::ceil_div(elems, kThreads) * 3 * sizeof(float), 256);
}

extern "C" int ms_bilagrid_tv_fwd(int B, int L, int Gh, int Gw, const float *grids, void *workspace, size_t workspace_bytes,
                                  float *out1, void *stream_) {
    int64_t elems;
    if (int rc = check_grid(B, L, Gh, Gw, "bilagrid_tv_fwd", &elems)) return rc;
    MS_REQUIRE(grids && workspace && out1, MS_ERR_INVALID_ARG, "bilagrid_tv_fwd: null pointer");
    const size_t need = ms::align_up((size_t)ms::ceil_div(elems, kThreads) * 3 * sizeof(float), 256);
    MS_REQUIRE(workspace_bytes >= need, MS_ERR_WORKSPACE, "bilagrid_tv_fwd: workspace of %zu bytes, needs %zu", workspace_bytes,
               need);
    hipStream_t stream = (hipStream_t)stream_;
    float *partials = (float *)workspace;
    const bool vec = Gw % 4 == 0 && aligned16(grids);
    const int64_t items = vec ? elems / 4 : elems, rows = ms::ceil_div(items, kThreads);
    if (vec)
        hipLaunchKernelGGL((k_tv_fwd<4>), dim3((unsigned)rows), dim3(kThreads), 0, stream, items, L, Gh, Gw, grids, partials);
    else
        hipLaunchKernelGGL((k_tv_fwd<1>), dim3((unsigned)rows), dim3(kThreads), 0, stream, items, L, Gh, Gw, grids, partials);
    MS_LAUNCH_CHECK();
    // the three means' weights: 1 / (differences along the axis in one batch entry) / B; an axis of size 1 has none
    const double per = 12.0 * B;
    const double cx = Gw > 1 ? 1.0 / (per * L * Gh * (Gw - 1.0)) : 0.0, cy = Gh > 1 ? 1.0 / (per * L * (Gh - 1.0) * Gw) : 0.0,
                 cz = L > 1 ? 1.0 / (per * (L - 1.0) * Gh * Gw) : 0.0;
    hipLaunchKernelGGL(k_tv_finalize, dim3(1), dim3(kThreads), 0, stream, (const float *)partials, rows, cx, cy, cz, out1);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

extern "C" int ms_bilagrid_tv_bwd(int B, int L, int Gh, int Gw, const float *grids, const float *v_loss, float *v_grids,
                                  void *stream_) {
    int64_t elems;
    if (int rc = check_grid(B, L, Gh, Gw, "bilagrid_tv_bwd", &elems)) return rc;
    MS_REQUIRE(grids && v_loss && v_grids, MS_ERR_INVALID_ARG, "bilagrid_tv_bwd: null pointer");
    const double per = 12.0 * B;
    const float kx = Gw > 1 ? (float)(2.0 / (per * L * Gh * (Gw - 1.0))) : 0.f,
                ky = Gh > 1 ? (float)(2.0 / (per * L * (Gh - 1.0) * Gw)) : 0.f,
                kz = L > 1 ? (float)(2.0 / (per * (L - 1.0) * Gh * Gw)) : 0.f;
    const bool vec = Gw % 4 == 0 && aligned16(grids) && aligned16(v_grids);
    const int64_t items = vec ? elems / 4 : elems, rows = ms::ceil_div(items, kThreads);
    hipStream_t stream = (hipStream_t)stream_;
    if (vec)
        hipLaunchKernelGGL((k_tv_bwd<4>), dim3((unsigned)rows), dim3(kThreads), 0, stream, items, L, Gh, Gw, grids, v_loss, kx, ky,
                           kz, v_grids);
    else
        hipLaunchKernelGGL((k_tv_bwd<1>), dim3((unsigned)rows), dim3(kThreads), 0, stream, items, L, Gh, Gw, grids, v_loss, kx, ky,
                           kz, v_grids);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
