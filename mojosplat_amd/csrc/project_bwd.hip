// Backward of the EWA projection (project.hip) for gfx950: one lane per Gaussian.
//
// No reference counterpart (the reference renderer is forward-only, mojosplat/render.py:11);
// the chain rule is applied to the forward stated in mojosplat/kernels/projection.mojo:50-257:
//   (v_means2d, v_conics, v_depths) -> v_means3d, v_scales (w.r.t. the log-scales when the
//   forward took log-scales), v_quats (w.r.t. the un-normalised quaternion).
// Culled Gaussians (radii == 0) get zero gradients.  Recomputes the forward intermediates in
// registers instead of storing them: 44 B in + 24 B of upstream grads + 40 B out per Gaussian.
//
// Also here: the densification statistics of 3DGS adaptive density control (Kerbl et al. 2023; gsplat's default
// strategy), accumulated per view into caller-owned f32[N] buffers -- ms_render_bwd_finish_densify (inside the
// quad-wave backward projection, where v_means2d lives in registers only) and ms_densify_stats_update (from a
// v_means2d / radii pair the caller already holds).  Semantics: mojosplat_amd/densify.py, update_torch.
#include "ms_common.hpp"
#include "project_device.hpp"
#include "pose_grad.hpp"

namespace {

// The densification statistics of one view: the buffers and the frame's projection (near / far, opacity-aware extent,
// radius_clip 0), whose verdict decides which Gaussians count.
struct DensifyArgs {
    ms::ProjParams P;
    float half_w, half_h, max_wh;
    float *grad2d, *count, *max_radii;
};

// One Gaussian's update; each Gaussian has one owner lane, so plain read-modify-writes.  r0 / r1: its radii in the view
// (a Gaussian with a zero radius was culled and is left untouched); g0 / g1: dL/dmeans2d in pixels.  Uncontracted and
// IEEE (sqrt, divide) like the torch definition: count and max_radii are exact, grad2d within an ulp of its square root.
__device__ __forceinline__ void densify_update(int64_t i, int r0, int r1, float g0, float g1, float half_w, float half_h,
                                               float max_wh, float *__restrict__ grad2d, float *__restrict__ count,
                                               float *__restrict__ max_radii) {
#pragma clang fp contract(off)
    if (r0 > 0 && r1 > 0) {
        const float gx = g0 * half_w, gy = g1 * half_h;
        grad2d[i] += sqrtf(gx * gx + gy * gy);
        count[i] += 1.0f;
        max_radii[i] = fmaxf(max_radii[i], (float)max(r0, r1) / max_wh);
    }
}

// Hides a pointer's provenance from the optimiser: STATS's projection then loads and computes on values of its own,
// and nothing of it is merged with the backward's own chain (whose contraction -- and so whose bits -- must not move).
// (Kept in the global address space, so that its loads stay global_load.)
template <class T>
__device__ __forceinline__ const T *opaque(const T *p) {
    auto g = (const __attribute__((address_space(1))) T *)p;
    asm volatile("" : "+s"(g));
    return (const T *)g;
}

struct ProjBwdParams {
    float fx, fy, cx, cy, eps2d;
    float lim_x_pos, lim_x_neg, lim_y_pos, lim_y_neg;
    int scales_are_log;
};

// ROWS: the upstream gradients come as the backward rasteriser's packed 64-byte rows (rasterize_bwd.hip: mx my ca cb cc
// op c0 c1 c2 c3 ...) instead of v_means2d / v_conics; the kernel then also writes v_opacities and v_colors from the row
// (what k_unpack_grads would have done in a pass of its own).
// ROWS == 2: the rows of the quad-wave rasteriser (rasterize_bwdq.hip) -- RAW sums over the Gaussian's pixels,
//   gx gy s1 s2 s3 m0 c0 c1 c2  =  sum vs dx, sum vs dy, sum vs dx^2, sum vs dx dy, sum vs dy^2, sum vs, colour gradients
// (vs = dL/dsigma of a pixel-Gaussian pair, dx = mean - pixel): with the conic (a, b, c) this kernel recomputes anyway,
// v_mean = (a gx + b gy, b gx + c gy), v_conic = (s1 / 2, s2, s3 / 2), v_opacity = -m0 / opacity.  A Gaussian whose row is
// all zero was never blended (or culled): zero gradients, no radii needed.
// STATS (ROWS == 2 only): every lane also re-projects its Gaussian with the forward's own project_one -- the alive verdict
// and the radii, which a lean frame never wrote -- and updates the densification statistics D with its vm0 / vm1 (zero
// for a Gaussian alive but never blended).  The gradients are those of STATS == false, bit for bit.
// POSE: the lane also forms its Gaussian's 12 terms of dL/d[Rv | t] (the world->camera view matrix's top three rows) in
// `pose`, from values the backward holds anyway: with p_c = Rv p + t and Sigma_c = Rv Sigma Rv^T,
//   v_Rv = v_p_c p^T + (v_cc + v_cc^T) Rv Sigma,   v_t = v_p_c
// (zero for a culled or never-blended Gaussian).  The terms are formed in a block of their own without contraction, and
// nothing of the existing chain consumes them: the Gaussian's gradients are those of POSE == false, bit for bit.
template <int ROWS, bool STATS = false, bool POSE = false>
__global__ __launch_bounds__(256) void k_project_ewa_bwd(
    int64_t N, const float *__restrict__ means3d, const float *__restrict__ scales,
    const float *__restrict__ quats, const float *__restrict__ viewmat, ProjBwdParams P,
    const int32_t *__restrict__ radii, const float *__restrict__ v_means2d,
    const float *__restrict__ v_conics, const float *__restrict__ v_depths,
    float *__restrict__ v_means3d, float *__restrict__ v_scales, float *__restrict__ v_quats,
    const float *__restrict__ rows, int cdim, float *__restrict__ v_colors, float *__restrict__ v_opacities,
    const float *__restrict__ opacities, DensifyArgs D, float *__restrict__ pose_slab) {
    static_assert(!STATS || ROWS == 2, "the statistics ride on the quad-wave rows");
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (!POSE && i >= N) return;
    float pose[12];   // POSE: this Gaussian's terms (zero past N)
    if constexpr (POSE)
#pragma unroll
        for (int k = 0; k < 12; ++k) pose[k] = 0.f;
    if (!POSE || i < N) {
        int st_r0 = 0, st_r1 = 0;
        if constexpr (STATS) {
            const ms::ProjOut o = ms::project_one(i, opaque(means3d), opaque(scales), opaque(quats), opaque(opacities),
                                                  opaque(viewmat), D.P);
            st_r0 = o.r0; st_r1 = o.r1;
        }
        float4 row0 = make_float4(0.f, 0.f, 0.f, 0.f), row1 = row0;
        bool visible;
        if constexpr (ROWS == 1) {
            const float4 *row = reinterpret_cast<const float4 *>(rows + i * 16);
            row0 = row[0]; row1 = row[1];
            const float4 row2 = row[2];
            v_opacities[i] = row1.y;
            const float c[4] = {row1.z, row1.w, row2.x, row2.y};
            for (int k = 0; k < cdim && k < 4; ++k) v_colors[i * cdim + k] = c[k];
        }
        if constexpr (ROWS == 2) {
            const float4 *row = reinterpret_cast<const float4 *>(rows + i * 16);
            row0 = row[0]; row1 = row[1];
            const float c2 = rows[i * 16 + 8];
            const float op = opacities[i];
            v_opacities[i] = row1.y != 0.f ? -row1.y / op : 0.f;
            v_colors[i * 3] = row1.z; v_colors[i * 3 + 1] = row1.w; v_colors[i * 3 + 2] = c2;
            visible = row0.x != 0.f || row0.y != 0.f || row0.z != 0.f || row0.w != 0.f || row1.x != 0.f || row1.y != 0.f;
        } else {
            const int2 rad = reinterpret_cast<const int2 *>(radii)[i];
            visible = rad.x > 0 && rad.y > 0;
        }
        float o_p[3] = {0.f, 0.f, 0.f}, o_s[3] = {0.f, 0.f, 0.f}, o_q[4] = {0.f, 0.f, 0.f, 0.f};
        float st_g0 = 0.f, st_g1 = 0.f;
        if (visible) {
            float V[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) V[k] = viewmat[k];
            // ---- recompute forward -----------------------------------------------------------
            const float p0 = means3d[3 * i], p1 = means3d[3 * i + 1], p2 = means3d[3 * i + 2];
            const float x = V[0] * p0 + V[1] * p1 + V[2] * p2 + V[3];
            const float y = V[4] * p0 + V[5] * p1 + V[6] * p2 + V[7];
            const float z = V[8] * p0 + V[9] * p1 + V[10] * p2 + V[11];
            const float4 q4 = reinterpret_cast<const float4 *>(quats)[i];
            const float qn2 = q4.x * q4.x + q4.y * q4.y + q4.z * q4.z + q4.w * q4.w;
            const float inv_norm = 1.0f / sqrtf(qn2);
            const float w = q4.x * inv_norm, qx = q4.y * inv_norm, qy = q4.z * inv_norm, qz = q4.w * inv_norm;
            float R[3][3];
            R[0][0] = 1.f - 2.f * (qy * qy + qz * qz); R[0][1] = 2.f * (qx * qy - w * qz); R[0][2] = 2.f * (qx * qz + w * qy);
            R[1][0] = 2.f * (qx * qy + w * qz); R[1][1] = 1.f - 2.f * (qx * qx + qz * qz); R[1][2] = 2.f * (qy * qz - w * qx);
            R[2][0] = 2.f * (qx * qz - w * qy); R[2][1] = 2.f * (qy * qz + w * qx); R[2][2] = 1.f - 2.f * (qx * qx + qy * qy);
            float s[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
            if (P.scales_are_log) { s[0] = expf(s[0]); s[1] = expf(s[1]); s[2] = expf(s[2]); }
            float Mx[3][3], cov[3][3], tmp[3][3], cc[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) Mx[r][c] = R[r][c] * s[c];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) cov[r][c] = Mx[r][0] * Mx[c][0] + Mx[r][1] * Mx[c][1] + Mx[r][2] * Mx[c][2];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) tmp[r][c] = V[4 * r] * cov[0][c] + V[4 * r + 1] * cov[1][c] + V[4 * r + 2] * cov[2][c];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) cc[r][c] = tmp[r][0] * V[4 * c] + tmp[r][1] * V[4 * c + 1] + tmp[r][2] * V[4 * c + 2];
            const float rz = 1.0f / z, rz2 = rz * rz, rz3 = rz2 * rz;
            const float xr = x * rz, yr = y * rz;
            const bool x_free = xr <= P.lim_x_pos && xr >= -P.lim_x_neg;
            const bool y_free = yr <= P.lim_y_pos && yr >= -P.lim_y_neg;
            const float tx = z * fminf(P.lim_x_pos, fmaxf(-P.lim_x_neg, xr));
            const float ty = z * fminf(P.lim_y_pos, fmaxf(-P.lim_y_neg, yr));
            const float J00 = P.fx * rz, J02 = -P.fx * tx * rz2, J11 = P.fy * rz, J12 = -P.fy * ty * rz2;
            float JC[2][3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                JC[0][c] = J00 * cc[0][c] + J02 * cc[2][c];
                JC[1][c] = J11 * cc[1][c] + J12 * cc[2][c];
            }
            const float a = JC[0][0] * J00 + JC[0][2] * J02 + P.eps2d;
            const float b = JC[0][1] * J11 + JC[0][2] * J12;
            const float c = JC[1][1] * J11 + JC[1][2] * J12 + P.eps2d;
            const float inv_det = 1.0f / (a * c - b * b);
            const float ka = c * inv_det, kb = -b * inv_det, kc = a * inv_det;  // conic

            // ---- backward --------------------------------------------------------------------
            float vm0, vm1, vka, vkb, vkc;
            if constexpr (ROWS == 2) {
                vm0 = ka * row0.x + kb * row0.y;
                vm1 = kb * row0.x + kc * row0.y;
                vka = 0.5f * row0.z; vkb = 0.5f * row0.w; vkc = 0.5f * row1.x;
            } else {
                vm0 = ROWS ? row0.x : v_means2d[2 * i]; vm1 = ROWS ? row0.y : v_means2d[2 * i + 1];
                vka = ROWS ? row0.z : v_conics[3 * i]; vkb = (ROWS ? row0.w : v_conics[3 * i + 1]) * 0.5f;
                vkc = ROWS ? row1.x : v_conics[3 * i + 2];
            }
            if constexpr (STATS) { st_g0 = vm0; st_g1 = vm1; }
            const float vd = v_depths ? v_depths[i] : 0.f;
            // conic = inverse(cov2d): v_cov2d = -K vK K  (K symmetric; off-diagonal grad halved)
            const float t00 = ka * vka + kb * vkb, t01 = ka * vkb + kb * vkc;
            const float t10 = kb * vka + kc * vkb, t11 = kb * vkb + kc * vkc;
            const float g00 = -(t00 * ka + t01 * kb), g01 = -(t00 * kb + t01 * kc);
            const float g10 = -(t10 * ka + t11 * kb), g11 = -(t10 * kb + t11 * kc);
            // cov2d = J cc J^T :  v_cc = J^T G J ;  v_J = G J cc^T + G^T J cc
            const float Jm[2][3] = {{J00, 0.f, J02}, {0.f, J11, J12}};
            const float G[2][2] = {{g00, g01}, {g10, g11}};
            float v_cc[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int cidx = 0; cidx < 3; ++cidx)
                    v_cc[r][cidx] = Jm[0][r] * (G[0][0] * Jm[0][cidx] + G[0][1] * Jm[1][cidx]) +
                                    Jm[1][r] * (G[1][0] * Jm[0][cidx] + G[1][1] * Jm[1][cidx]);
            // JCt[r][c] = (J cc^T)[r][c] ; cc is symmetric up to rounding, keep both forms
            float v_J[2][3];
#pragma unroll
            for (int cidx = 0; cidx < 3; ++cidx) {
                const float jct0 = Jm[0][0] * cc[cidx][0] + Jm[0][1] * cc[cidx][1] + Jm[0][2] * cc[cidx][2];
                const float jct1 = Jm[1][0] * cc[cidx][0] + Jm[1][1] * cc[cidx][1] + Jm[1][2] * cc[cidx][2];
                v_J[0][cidx] = G[0][0] * jct0 + G[0][1] * jct1 + G[0][0] * JC[0][cidx] + G[1][0] * JC[1][cidx];
                v_J[1][cidx] = G[1][0] * jct0 + G[1][1] * jct1 + G[0][1] * JC[0][cidx] + G[1][1] * JC[1][cidx];
            }
            // camera-space mean
            float v_x = P.fx * rz * vm0, v_y = P.fy * rz * vm1;
            float v_z = -(P.fx * x * vm0 + P.fy * y * vm1) * rz2 + vd;
            v_z += -P.fx * rz2 * v_J[0][0] - P.fy * rz2 * v_J[1][1];
            if (x_free) { v_x += -P.fx * rz2 * v_J[0][2]; v_z += 2.f * P.fx * tx * rz3 * v_J[0][2]; }
            else        { v_z += P.fx * tx * rz3 * v_J[0][2]; }
            if (y_free) { v_y += -P.fy * rz2 * v_J[1][2]; v_z += 2.f * P.fy * ty * rz3 * v_J[1][2]; }
            else        { v_z += P.fy * ty * rz3 * v_J[1][2]; }
            // world mean: p = Wv^T v_mean_c
            o_p[0] = V[0] * v_x + V[4] * v_y + V[8] * v_z;
            o_p[1] = V[1] * v_x + V[5] * v_y + V[9] * v_z;
            o_p[2] = V[2] * v_x + V[6] * v_y + V[10] * v_z;
            // world covariance: v_cov = Wv^T v_cc Wv
            float t2[3][3], v_cov[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int cidx = 0; cidx < 3; ++cidx)
                    t2[r][cidx] = V[r] * v_cc[0][cidx] + V[4 + r] * v_cc[1][cidx] + V[8 + r] * v_cc[2][cidx];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int cidx = 0; cidx < 3; ++cidx)
                    v_cov[r][cidx] = t2[r][0] * V[cidx] + t2[r][1] * V[4 + cidx] + t2[r][2] * V[8 + cidx];
            // cov = M M^T : v_M = (v_cov + v_cov^T) M ; M = R diag(s)
            float v_M[3][3], v_R[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int cidx = 0; cidx < 3; ++cidx)
                    v_M[r][cidx] = (v_cov[r][0] + v_cov[0][r]) * Mx[0][cidx] + (v_cov[r][1] + v_cov[1][r]) * Mx[1][cidx] +
                                   (v_cov[r][2] + v_cov[2][r]) * Mx[2][cidx];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float vs = R[0][k] * v_M[0][k] + R[1][k] * v_M[1][k] + R[2][k] * v_M[2][k];
                o_s[k] = P.scales_are_log ? vs * s[k] : vs;
#pragma unroll
                for (int r = 0; r < 3; ++r) v_R[r][k] = v_M[r][k] * s[k];
            }
            // rotation -> normalised quaternion -> raw quaternion
            const float vw = 2.f * (qz * (v_R[1][0] - v_R[0][1]) + qy * (v_R[0][2] - v_R[2][0]) + qx * (v_R[2][1] - v_R[1][2]));
            const float vx = 2.f * (qy * (v_R[0][1] + v_R[1][0]) + qz * (v_R[0][2] + v_R[2][0]) + w * (v_R[2][1] - v_R[1][2])) -
                             4.f * qx * (v_R[1][1] + v_R[2][2]);
            const float vy = 2.f * (qx * (v_R[0][1] + v_R[1][0]) + w * (v_R[0][2] - v_R[2][0]) + qz * (v_R[1][2] + v_R[2][1])) -
                             4.f * qy * (v_R[0][0] + v_R[2][2]);
            const float vz = 2.f * (w * (v_R[1][0] - v_R[0][1]) + qx * (v_R[0][2] + v_R[2][0]) + qy * (v_R[1][2] + v_R[2][1])) -
                             4.f * qz * (v_R[0][0] + v_R[1][1]);
            const float dotn = vw * w + vx * qx + vy * qy + vz * qz;
            o_q[0] = (vw - dotn * w) * inv_norm;
            o_q[1] = (vx - dotn * qx) * inv_norm;
            o_q[2] = (vy - dotn * qy) * inv_norm;
            o_q[3] = (vz - dotn * qz) * inv_norm;
            if constexpr (POSE) {
#pragma clang fp contract(off)
                const float vpc[3] = {v_x, v_y, v_z}, p[3] = {p0, p1, p2};
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int cidx = 0; cidx < 3; ++cidx)
                        pose[4 * r + cidx] = vpc[r] * p[cidx] + (v_cc[r][0] + v_cc[0][r]) * tmp[0][cidx] +
                                             (v_cc[r][1] + v_cc[1][r]) * tmp[1][cidx] + (v_cc[r][2] + v_cc[2][r]) * tmp[2][cidx];
                    pose[4 * r + 3] = vpc[r];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v_means3d[3 * i + k] = o_p[k];
            v_scales[3 * i + k] = o_s[k];
        }
        reinterpret_cast<float4 *>(v_quats)[i] = make_float4(o_q[0], o_q[1], o_q[2], o_q[3]);
        if constexpr (STATS)
            densify_update(i, st_r0, st_r1, st_g0, st_g1, D.half_w, D.half_h, D.max_wh, D.grad2d, D.count, D.max_radii);
    }
    if constexpr (POSE) ms::pose_block_sum_store<12>(pose, pose_slab + (int64_t)blockIdx.x * ms::kPoseSlabStride);
}

// ms_densify_stats_update: one lane per Gaussian
__global__ __launch_bounds__(256) void k_densify_stats_update(int64_t N, const int32_t *__restrict__ radii,
                                                              const float *__restrict__ v_means2d, float half_w, float half_h,
                                                              float max_wh, float *__restrict__ grad2d,
                                                              float *__restrict__ count, float *__restrict__ max_radii) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int2 r = reinterpret_cast<const int2 *>(radii)[i];
    if (r.x > 0 && r.y > 0) {
        const float2 g = reinterpret_cast<const float2 *>(v_means2d)[i];
        densify_update(i, r.x, r.y, g.x, g.y, half_w, half_h, max_wh, grad2d, count, max_radii);
    }
}

// The launch-boundary half of the pose sum (pose_grad.hpp): one workgroup of kSlabThreads; thread t sums slab rows t,
// t + kSlabThreads, ... in that order, then the workgroup's block sum in wave order.  Threads k < K store the total,
// K <= k < out_len a zero.  (The 3 907 rows of 1 M Gaussians take 6 - 7 us at 256 lanes and at 1024 alike: the launch's
// own latency, not its 250 KB.)
constexpr int kSlabThreads = 1024;
template <int K>
__global__ __launch_bounds__(kSlabThreads) void k_pose_slab_sum(const float *__restrict__ slab, int64_t rows,
                                                                float *__restrict__ out, int out_len) {
    constexpr int K4 = (K + 3) / 4;
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
#pragma unroll 4
    for (int64_t r = threadIdx.x; r < rows; r += kSlabThreads) {
        const float4 *row = reinterpret_cast<const float4 *>(slab + r * ms::kPoseSlabStride);
#pragma unroll
        for (int j = 0; j < K4; ++j) {
            const float4 v = row[j];
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (4 * j + c < K) acc[4 * j + c] += e[c];
        }
    }
    ms::pose_block_sum_store<K, kSlabThreads / 64>(acc, out);
    if ((int)threadIdx.x >= K && (int)threadIdx.x < out_len) out[threadIdx.x] = 0.f;
}

// The projection backward k_project_ewa_bwd<ROWS, STATS>(N, args...) on `stream`; with v_viewmat, its POSE twin on the
// slab `pose_scratch` (>= ms::pose_slab_bytes(N) bytes, checked by the caller) and the slab sum into v_viewmat f32[16].
template <int ROWS, bool STATS, class... Args>
int launch_ewa_bwd(int64_t N, float *v_viewmat, void *pose_scratch, void *stream_, Args... args) {
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t grid = ms::ceil_div(N, 256);
    MS_REQUIRE(grid <= 0x7fffffff, MS_ERR_INVALID_ARG, "project_bwd: N too large");
    if (!v_viewmat) {
        hipLaunchKernelGGL((k_project_ewa_bwd<ROWS, STATS>), dim3((unsigned)grid), dim3(256), 0, stream, N, args...,
                           (float *)nullptr);
        MS_LAUNCH_CHECK();
        return MS_OK;
    }
    float *slab = (float *)pose_scratch;
    hipLaunchKernelGGL((k_project_ewa_bwd<ROWS, STATS, true>), dim3((unsigned)grid), dim3(256), 0, stream, N, args..., slab);
    MS_LAUNCH_CHECK();
    return ms::pose_slab_sum(slab, grid, 12, v_viewmat, 16, stream_);
}

}  // namespace

int ms::pose_slab_sum(const float *slab, int64_t rows, int K, float *out, int out_len, void *stream) {
    MS_REQUIRE(out && out_len >= K && out_len <= kSlabThreads && rows >= 0 && (rows == 0 || slab), MS_ERR_INVALID_ARG,
               "pose_slab_sum: bad argument");
    MS_REQUIRE(((uintptr_t)slab & 15) == 0, MS_ERR_INVALID_ARG, "pose_slab_sum: the slab must be 16-byte aligned");
    if (K == 12)
        hipLaunchKernelGGL(k_pose_slab_sum<12>, dim3(1), dim3(kSlabThreads), 0, (hipStream_t)stream, slab, rows, out, out_len);
    else if (K == 3)
        hipLaunchKernelGGL(k_pose_slab_sum<3>, dim3(1), dim3(kSlabThreads), 0, (hipStream_t)stream, slab, rows, out, out_len);
    else
        MS_REQUIRE(false, MS_ERR_INVALID_ARG, "pose_slab_sum: %d components", K);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

extern "C" size_t ms_pose_scratch_bytes(int64_t N) { return ms::pose_slab_bytes(N); }

int ms::check_pose_out(int64_t N, const float *out, const void *scratch, size_t scratch_bytes, const char *who) {
    MS_REQUIRE(((uintptr_t)out & 3) == 0, MS_ERR_INVALID_ARG, "%s: the pose gradient must be 4-byte aligned", who);
    MS_REQUIRE(N == 0 || (scratch && ((uintptr_t)scratch & 15) == 0), MS_ERR_INVALID_ARG,
               "%s: the pose gradient needs 16-byte aligned scratch", who);
    MS_REQUIRE(N == 0 || scratch_bytes >= ms::pose_slab_bytes(N), MS_ERR_WORKSPACE, "%s: pose scratch %zu < %zu", who,
               scratch_bytes, ms::pose_slab_bytes(N));
    return MS_OK;
}

// (the limits are the forward projection's, from make_proj_params's own expressions)
static ProjBwdParams proj_bwd_params(const ms::View &v, int scales_are_log) {
    const ms::ProjParams F = ms::make_proj_params(v, 0.0f, scales_are_log, false);
    return ProjBwdParams{F.fx, F.fy, F.cx, F.cy, F.eps2d, F.lim_x_pos, F.lim_x_neg, F.lim_y_pos, F.lim_y_neg, scales_are_log};
}

int ms::project_bwd(const ms::Gaussians &g, const ms::View &v, const int32_t *radii, const float *v_means2d, const float *v_conics,
                    const float *v_depths, float *v_means3d, float *v_scales, float *v_quats, float *v_viewmat, void *pose_scratch,
                    void *stream) {
    MS_REQUIRE(g.N >= 0, MS_ERR_INVALID_ARG, "project_bwd: N < 0");
    if (g.N == 0) return v_viewmat ? ms::pose_slab_sum(nullptr, 0, 12, v_viewmat, 16, stream) : MS_OK;
    MS_REQUIRE(g.means3d && g.scales && g.quats && v.viewmat && radii && v_means2d && v_conics && v_means3d &&
                   v_scales && v_quats, MS_ERR_INVALID_ARG, "project_bwd: null pointer");
    MS_REQUIRE(v.W > 0 && v.H > 0 && v.fx != 0.f && v.fy != 0.f, MS_ERR_INVALID_ARG, "project_bwd: bad camera");
    MS_REQUIRE(((uintptr_t)g.quats & 15) == 0 && ((uintptr_t)v_quats & 15) == 0 && ((uintptr_t)radii & 7) == 0,
               MS_ERR_INVALID_ARG, "project_bwd: quats/v_quats must be 16-byte, radii 8-byte aligned");
    const ProjBwdParams P = proj_bwd_params(v, g.scales_are_log);
    return launch_ewa_bwd<0, false>(g.N, v_viewmat, pose_scratch, stream, g.means3d, g.scales, g.quats, v.viewmat, P, radii,
                                    v_means2d, v_conics, v_depths, v_means3d, v_scales, v_quats, (const float *)nullptr, 0,
                                    (float *)nullptr, (float *)nullptr, (const float *)nullptr, DensifyArgs{});
}

extern "C" int ms_project_gaussians_bwd(int64_t N, const float *means3d, const float *scales,
                                        int scales_are_log, const float *quats, const float *viewmat,
                                        float fx, float fy, float cx, float cy, int W, int H,
                                        float eps2d, const int32_t *radii, const float *v_means2d,
                                        const float *v_conics, const float *v_depths,
                                        float *v_means3d, float *v_scales, float *v_quats,
                                        void *stream) {
    const ms::Gaussians g{N, means3d, scales, scales_are_log, quats, nullptr, nullptr, 0, 0};
    const ms::View v{viewmat, fx, fy, cx, cy, W, H, eps2d, 0.f, 0.f};
    return ms::project_bwd(g, v, radii, v_means2d, v_conics, v_depths, v_means3d, v_scales, v_quats, nullptr, nullptr, stream);
}

extern "C" int ms_project_gaussians_bwd_pose(int64_t N, const float *means3d, const float *scales, int scales_are_log,
                                             const float *quats, const float *viewmat, float fx, float fy, float cx, float cy,
                                             int W, int H, float eps2d, const int32_t *radii, const float *v_means2d,
                                             const float *v_conics, const float *v_depths, float *v_means3d, float *v_scales,
                                             float *v_quats, float *v_viewmat, void *pose_scratch, size_t pose_scratch_bytes,
                                             void *stream) {
    const ms::Gaussians g{N, means3d, scales, scales_are_log, quats, nullptr, nullptr, 0, 0};
    const ms::View v{viewmat, fx, fy, cx, cy, W, H, eps2d, 0.f, 0.f};
    if (v_viewmat)
        if (int rc = ms::check_pose_out(N, v_viewmat, pose_scratch, pose_scratch_bytes, "project_bwd")) return rc;
    return ms::project_bwd(g, v, radii, v_means2d, v_conics, v_depths, v_means3d, v_scales, v_quats, v_viewmat, pose_scratch,
                            stream);
}

// ms_render_bwd: the same backward straight from the backward rasteriser's packed rows (which it also unpacks into
// v_colors / v_opacities)
int ms::project_bwd_from_rows(const ms::Gaussians &g, const ms::View &v, const int32_t *radii, const float *rows,
                              float *v_means3d, float *v_scales, float *v_quats, float *v_colors, float *v_opacities,
                              void *stream, bool raw, float *v_viewmat, void *pose_scratch) {
    if (g.N == 0) return v_viewmat ? ms::pose_slab_sum(nullptr, 0, 12, v_viewmat, 16, stream) : MS_OK;
    // raw: the quad-wave rasteriser's raw sums (ROWS == 2)
    MS_REQUIRE(g.means3d && g.scales && g.quats && v.viewmat && (radii || raw) && rows && v_means3d && v_scales && v_quats && v_colors && v_opacities,
               MS_ERR_INVALID_ARG, "project_bwd: null pointer");
    MS_REQUIRE(!raw || g.CDIM == 3, MS_ERR_INVALID_ARG, "project_bwd: raw rows carry three channels");
    MS_REQUIRE(v.W > 0 && v.H > 0 && v.fx != 0.f && v.fy != 0.f && g.CDIM >= 1 && g.CDIM <= 4, MS_ERR_INVALID_ARG, "project_bwd: bad camera / channels");
    MS_REQUIRE(((uintptr_t)g.quats & 15) == 0 && ((uintptr_t)v_quats & 15) == 0 && ((uintptr_t)radii & 7) == 0 && ((uintptr_t)rows & 15) == 0,
               MS_ERR_INVALID_ARG, "project_bwd: quats / v_quats / rows must be 16-byte, radii 8-byte aligned");
    const ProjBwdParams P = proj_bwd_params(v, g.scales_are_log);
    const float *none = nullptr;
    if (raw)
        return launch_ewa_bwd<2, false>(g.N, v_viewmat, pose_scratch, stream, g.means3d, g.scales, g.quats, v.viewmat, P, radii, none,
                                        none, none, v_means3d, v_scales, v_quats, rows, g.CDIM, v_colors, v_opacities, g.opacities,
                                        DensifyArgs{});
    return launch_ewa_bwd<1, false>(g.N, v_viewmat, pose_scratch, stream, g.means3d, g.scales, g.quats, v.viewmat, P, radii, none,
                                    none, none, v_means3d, v_scales, v_quats, rows, g.CDIM, v_colors, v_opacities, none, DensifyArgs{});
}

// ms_render_bwd_finish with the densification statistics: k_project_ewa_bwd<2, true>
static int finish_densify_impl(const ms::Gaussians &g, const ms::View &v, const float *rows, float *v_means3d, float *v_scales,
                               float *v_quats, float *v_opacities, float *v_colors, float *grad2d, float *count,
                               float *max_radii, float *v_viewmat, void *pose_scratch, void *stream) {
    MS_REQUIRE(g.N >= 0 && g.CDIM == 3 && v_means3d && v_scales && v_quats && v_opacities && v_colors && grad2d && count && max_radii,
               MS_ERR_INVALID_ARG, "render_bwd_finish_densify: bad argument");
    if (g.N == 0) return v_viewmat ? ms::pose_slab_sum(nullptr, 0, 12, v_viewmat, 16, stream) : MS_OK;
    MS_REQUIRE(g.means3d && g.scales && g.quats && v.viewmat && rows && g.opacities, MS_ERR_INVALID_ARG,
               "render_bwd_finish_densify: null pointer");
    MS_REQUIRE(v.W > 0 && v.H > 0 && v.fx != 0.f && v.fy != 0.f, MS_ERR_INVALID_ARG, "render_bwd_finish_densify: bad camera");
    MS_REQUIRE(((uintptr_t)g.quats & 15) == 0 && ((uintptr_t)v_quats & 15) == 0 && ((uintptr_t)rows & 15) == 0,
               MS_ERR_INVALID_ARG, "render_bwd_finish_densify: quats / v_quats / rows must be 16-byte aligned");
    MS_REQUIRE((((uintptr_t)grad2d | (uintptr_t)count | (uintptr_t)max_radii) & 3) == 0, MS_ERR_INVALID_ARG,
               "render_bwd_finish_densify: statistics must be 4-byte aligned");
    const ProjBwdParams P = proj_bwd_params(v, g.scales_are_log);
    DensifyArgs D;
    // the frame's projection: its planes, the opacity-aware extent and no radius clip (pipeline.hip, ms_render_fwd)
    D.P = ms::make_proj_params(v, 0.0f, g.scales_are_log, true);
    D.half_w = 0.5f * (float)v.W; D.half_h = 0.5f * (float)v.H; D.max_wh = (float)(v.W > v.H ? v.W : v.H);
    D.grad2d = grad2d; D.count = count; D.max_radii = max_radii;
    const float *none = nullptr;
    return launch_ewa_bwd<2, true>(g.N, v_viewmat, pose_scratch, stream, g.means3d, g.scales, g.quats, v.viewmat, P,
                                   (const int32_t *)nullptr, none, none, none, v_means3d, v_scales, v_quats, rows, g.CDIM, v_colors,
                                   v_opacities, g.opacities, D);
}

extern "C" int ms_render_bwd_finish_densify(int64_t N, const float *means3d, const float *scales, int scales_are_log,
                                            const float *quats, const float *opacities, int CDIM, const float *viewmat,
                                            float fx, float fy, float cx, float cy, int W, int H, float eps2d,
                                            const float *rows, float *v_means3d, float *v_scales, float *v_quats,
                                            float *v_opacities, float *v_colors, float near_plane, float far_plane,
                                            float *grad2d, float *count, float *max_radii, void *stream) {
    const ms::Gaussians g{N, means3d, scales, scales_are_log, quats, opacities, nullptr, 0, CDIM};
    const ms::View v{viewmat, fx, fy, cx, cy, W, H, eps2d, near_plane, far_plane};
    return finish_densify_impl(g, v, rows, v_means3d, v_scales, v_quats, v_opacities, v_colors, grad2d, count, max_radii, nullptr,
                               nullptr, stream);
}

extern "C" int ms_render_bwd_finish_densify_pose(int64_t N, const float *means3d, const float *scales, int scales_are_log,
                                                 const float *quats, const float *opacities, int CDIM, const float *viewmat,
                                                 float fx, float fy, float cx, float cy, int W, int H, float eps2d,
                                                 const float *rows, float *v_means3d, float *v_scales, float *v_quats,
                                                 float *v_opacities, float *v_colors, float near_plane, float far_plane,
                                                 float *grad2d, float *count, float *max_radii, float *v_viewmat,
                                                 void *pose_scratch, size_t pose_scratch_bytes, void *stream) {
    const ms::Gaussians g{N, means3d, scales, scales_are_log, quats, opacities, nullptr, 0, CDIM};
    const ms::View v{viewmat, fx, fy, cx, cy, W, H, eps2d, near_plane, far_plane};
    if (v_viewmat)
        if (int rc = ms::check_pose_out(N, v_viewmat, pose_scratch, pose_scratch_bytes, "render_bwd_finish_densify")) return rc;
    return finish_densify_impl(g, v, rows, v_means3d, v_scales, v_quats, v_opacities, v_colors, grad2d, count, max_radii, v_viewmat,
                               pose_scratch, stream);
}

extern "C" int ms_densify_stats_update(int64_t N, int W, int H, const int32_t *radii, const float *v_means2d, float *grad2d,
                                       float *count, float *max_radii, void *stream) {
    MS_REQUIRE(N >= 0, MS_ERR_INVALID_ARG, "densify_stats_update: N < 0");
    if (N == 0) return MS_OK;
    MS_REQUIRE(radii && v_means2d && grad2d && count && max_radii, MS_ERR_INVALID_ARG, "densify_stats_update: null pointer");
    MS_REQUIRE(W > 0 && H > 0, MS_ERR_INVALID_ARG, "densify_stats_update: bad image size");
    MS_REQUIRE((((uintptr_t)radii | (uintptr_t)v_means2d) & 7) == 0 &&
                   (((uintptr_t)grad2d | (uintptr_t)count | (uintptr_t)max_radii) & 3) == 0,
               MS_ERR_INVALID_ARG, "densify_stats_update: radii / v_means2d must be 8-byte, statistics 4-byte aligned");
    const int64_t grid = ms::ceil_div(N, 256);
    MS_REQUIRE(grid <= 0x7fffffff, MS_ERR_INVALID_ARG, "densify_stats_update: N too large");
    hipLaunchKernelGGL(k_densify_stats_update, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, N, radii, v_means2d,
                       0.5f * (float)W, 0.5f * (float)H, (float)(W > H ? W : H), grad2d, count, max_radii);
    MS_LAUNCH_CHECK();
    return MS_OK;
}
