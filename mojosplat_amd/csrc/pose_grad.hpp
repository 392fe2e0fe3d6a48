// Camera-pose gradients: the deterministic sum of per-Gaussian terms into one small vector (v_viewmat: 12 floats of the
// world->camera [R|t]; v_campos: 3 floats of the camera centre).
//
// Two steps, no float atomics (cdna_hip_programming.md Guideline 12: adders on one row are an order of magnitude slower,
// and their sum depends on arrival order):
//   1. inside each 256-lane workgroup of the backward kernel: a butterfly across the wave (cross-lane shuffles), then the
//      4 waves' totals through LDS, summed in wave order; thread k stores component k of the workgroup's partial with a
//      plain store into row blockIdx.x of a slab (kPoseSlabStride floats a row);
//   2. at the launch boundary, one workgroup of 1024 lanes (k_pose_slab_sum, project_bwd.hip) sums the slab's rows in a
//      fixed order and OVERWRITES the caller's output.
// Every add happens in an order fixed by N alone, so the result is bitwise the same from run to run.
#pragma once
#include "ms_common.hpp"

namespace ms {

constexpr int kPoseSlabStride = 16;   // floats per workgroup partial (64-byte rows: float4 loads in the slab sum)

// Scratch of the slab for a launch of ceil(N / 256) workgroups of 256 lanes (at least one row).
inline size_t pose_slab_bytes(int64_t N) {
    const int64_t rows = N > 0 ? (N + 255) / 256 : 1;
    return align_up((size_t)rows * kPoseSlabStride * sizeof(float), 256);
}

// Sums v[0..K) over the WAVES * 64 lanes of the workgroup; lanes k < K then store component k of the total to row[k].
// Every lane of the workgroup must call it (one barrier inside).
template <int K, int WAVES = 4>
__device__ __forceinline__ void pose_block_sum_store(float (&v)[K], float *__restrict__ row) {
    static_assert(K <= 64, "one lane per component");
    __shared__ float s_part[WAVES][K];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], off, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s_part[w][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        float t = s_part[0][k];
#pragma unroll
        for (int w2 = 1; w2 < WAVES; ++w2) t += s_part[w2][k];
        row[k] = t;
    }
}

// Sums `rows` slab rows of K components (k_pose_slab_sum, one workgroup) into out[0..K) and writes zeros to
// out[K..out_len): an overwrite, on `stream`, behind the kernel that filled the slab.
int pose_slab_sum(const float *slab, int64_t rows, int K, float *out, int out_len, void *stream);

}  // namespace ms
