/*
 * mojosplat_hip.h -- C ABI of libmojosplat_hip.so, the MI355X (gfx950) backend for the
 * mojosplat render path: EWA projection -> tile binning/sort -> tile rasteriser.
 *
 * This is the drop-in boundary.  Each entry point replaces one custom-op / external call
 * of the reference (paths relative to the reference repo root):
 *
 *   ms_project_gaussians_fwd          op "project_gaussians", mojosplat/kernels/projection.mojo:260-326,
 *                                     called from mojosplat/projection.py:429-454; and
 *                                     gsplat.fully_fused_projection, projection.py:381-397
 *   ms_isect_tiles_count / _emit      gsplat.isect_tiles, mojosplat/binning.py:73-82
 *   ms_isect_offset_encode            gsplat.isect_offset_encode, mojosplat/binning.py:84
 *   ms_rasterize_to_pixels_3dgs_fwd   op "rasterize_to_pixels_3dgs_fwd",
 *                                     mojosplat/kernels/rasterization.mojo:169-240, called from
 *                                     mojosplat/rasterization.py:169-183; and
 *                                     gsplat.rasterize_to_pixels, rasterization.py:109-122
 *   ms_rasterize_to_pixels_3dgs_bwd,  no reference counterpart (reference is forward-only,
 *   ms_project_gaussians_bwd          render.py:11); gsplat's backward semantics
 *   ms_render_fwd                     the whole of render_gaussians' device work
 *                                     (mojosplat/render.py:63-101) in one call
 *   ms_render_bwd                     the backward of such a frame (no reference counterpart) in one call
 *   ms_render_bwd_finish_densify,     3DGS densification statistics accumulated in a training backward
 *   ms_densify_stats_update           (no reference counterpart)
 *   ms_*_pose, ms_pose_scratch_bytes  the gradient w.r.t. the camera pose (view matrix / camera centre) in the
 *                                     training backward (no reference counterpart; gsplat returns it)
 *   ms_photometric_loss_*             the L1 + D-SSIM training loss, fused forward and backward (nothing in the
 *                                     reference: it is forward-only, README.md:145; the CUDA stack's fused-ssim)
 *   ms_adam_step                      the Adam update of up to 8 parameter tensors in one launch, optionally masked by
 *                                     the view's visibility (nothing in the reference: it is forward-only and updates no
 *                                     parameter; the CUDA stack's torch.optim.Adam(fused=True), gsplat's SelectiveAdam)
 *   ms_densify_classify,              the densification step (clone, split, prune) over every parameter tensor and its Adam
 *   ms_densify_move                   moments (nothing in the reference; the CUDA stack's gsplat DefaultStrategy)
 *   ms_mcmc_sample, ms_mcmc_apply,    the MCMC strategy: relocate dead Gaussians, grow, perturb the means (nothing in the
 *   ms_mcmc_noise                     reference; the CUDA stack's gsplat MCMCStrategy)
 *   ms_knn                            exact k nearest neighbours of a point cloud, the distances a scene's initial scales
 *                                     come from (nothing in the reference: it has no training; the CUDA stack's simple-knn)
 *   ms_ply_pack, ms_ply_unpack        the row move between a scene's parameter tensors and the float32 rows of a 3DGS PLY
 *                                     file (nothing in the reference: it reads and writes no scene; the CUDA stack's
 *                                     save_ply / load_ply of 3DGS and gsplat's export_splats, composed from torch ops)
 *   ms_splat_compress, _decompress,   the bit packing of the viewer formats, compressed PLY and .splat (nothing in the
 *   ms_splat32_pack, _unpack          reference; gsplat's export_splats(format="ply_compressed" | "splat"), numpy on the host)
 *   ms_bilagrid_slice_*,              bilateral-grid colour correction between the render and the loss, and the grids'
 *   ms_bilagrid_tv_*                  total-variation loss (nothing in the reference; gsplat's use_bilateral_grid / lib_bilagrid)
 *   ms_contrib_accumulate             per-Gaussian contribution statistics of a view (blended pixels, largest and summed blend
 *                                     weight, the sum under a pixel weight map), for pruning before export and for lifting
 *                                     image masks to Gaussians (nothing in the reference; RadSplat's and LightGaussian's scores)
 *   ms_render_fwd_batch               the same for C cameras: the camera dimension of the reference's
 *                                     kernels (kernels/projection.mojo:32-37) that its wrappers pin to 1
 *
 * Conventions (same as the reference's op convention, projection.py:438-454):
 *   - destination passing: the caller (PyTorch) owns and pre-allocates every buffer,
 *     including scratch; the library never allocates device memory and keeps no per-frame or
 *     per-scene state.  What it does keep, process-wide and thread-safe: the thread-local
 *     error string, the environment switches it reads once (MOJOSPLAT_LAZY_SORT, MOJOSPLAT_SPLIT,
 *     MOJOSPLAT_SPLIT_MAX_ENTRIES and the measurement knobs listed in
 *     INTEGRATION.md; MOJOSPLAT_DEPTH_CUT / MOJOSPLAT_DEPTH_CUT_MIN_PAIRS too: ms_config_depth_cut changes them in-process),
 *     a counter that stamps depth-cut frames, and a mutex-guarded table of the (device, kernel) pairs whose dynamic-LDS ceiling it has
 *     already raised (hipFuncSetAttribute);
 *   - all pointers are DEVICE pointers unless a parameter says "host"; tensors are
 *     contiguous row-major with the layouts written next to each parameter;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*); the per-stage
 *     entry points never synchronise, so they can be captured into a hipGraph (the one
 *     exception, ms_render_fwd, says so below);
 *   - every function returns 0 on success or a non-zero ms_status; no C++ exception
 *     crosses this boundary.  ms_last_error_string() describes the last failure on the
 *     calling thread.
 *   - single camera (C = 1), like every wrapper of the reference (projection.py:431,
 *     rasterization.py:175); ms_render_fwd_batch is the one entry point with C > 1.
 */
#ifndef MOJOSPLAT_HIP_H
#define MOJOSPLAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MS_ABI_VERSION 5   /* 2: ms_render_bwd takes the frame's image (render_colors); 3: ms_render_redo_counts, the band-frame pair, ms_scene_prepare;
                              4: the pose-gradient entry points (ms_pose_scratch_bytes, ms_*_pose); 5: ms_adam_step
                              (the ms_densify_*, ms_mcmc_*, ms_knn*, ms_ply_* and ms_splat* entry points, ms_config_fused_sort, ms_render_front_count_offset and bits 48 and 49
                              of the flag word were added under 5: new symbols and a new bit, nothing existing changed) */

typedef enum ms_status {
    MS_OK = 0,
    MS_ERR_INVALID_ARG = 1,   /* null pointer, negative size, unsupported channel count ... */
    MS_ERR_WORKSPACE = 2,     /* workspace too small (ask ms_*_workspace_bytes)           */
    MS_ERR_TOO_LARGE = 3,     /* tile grid does not fit the binning kernels' LDS budget   */
    MS_ERR_HIP = 4            /* a HIP runtime call failed; see ms_last_error_string()    */
} ms_status;

typedef enum ms_color_dtype { MS_COLOR_F32 = 0, MS_COLOR_F16 = 1 } ms_color_dtype;

int ms_version(void);
const char *ms_last_error_string(void);

/* ---------------------------------------------------------------------------------------
 * Projection (EWA 3D -> 2D), gsplat semantics.
 *   in : means3d f32[N,3]; scales f32[N,3] (log-space when scales_are_log != 0, the exp is
 *        fused; linear otherwise, which is what the reference's kernel receives);
 *        quats f32[N,4] wxyz (normalised in-kernel); opacities f32[N] or NULL (NULL = no
 *        opacity cull / no opacity-aware extent); viewmat f32[16] row-major world->camera
 *        IN DEVICE MEMORY; pinhole fx fy cx cy; image W H; eps2d (0.3), near, far,
 *        radius_clip (0).
 *   out: means2d f32[N,2]; conics f32[N,3] (a,b,c of the inverse blurred 2x2 covariance);
 *        depths f32[N]; radii i32[N,2].  Culled Gaussians get radii = 0 and zeros elsewhere.
 * ------------------------------------------------------------------------------------- */
int ms_project_gaussians_fwd(int64_t N, const float *means3d, const float *scales,
                             int scales_are_log, const float *quats, const float *opacities,
                             const float *viewmat, float fx, float fy, float cx, float cy,
                             int W, int H, float eps2d, float near_plane, float far_plane,
                             float radius_clip, float *means2d, float *conics, float *depths,
                             int32_t *radii, void *stream);

/* ---------------------------------------------------------------------------------------
 * Binning.  Two calls around the one unavoidable size hand-off (the number of
 * intersections M is data dependent), exactly where gsplat.isect_tiles has its own.
 *
 * ms_isect_tiles_count: per-tile counts -> exclusive offsets.
 *   in : means2d f32[N,2], radii i32[N,2]; tile_size; tile grid tile_w x tile_h;
 *        [row_begin,row_end) restricts binning to a band of tile rows (multi-GPU
 *        sharding; pass 0,tile_h for the whole image);
 *        workspace of ms_isect_workspace_bytes(...) bytes.
 *   out: tile_ranges i32[tile_h,tile_w,2] = [start,end) into the sorted intersection list
 *        (tiles outside the band get empty ranges);
 *        tiles_per_gauss i32[N] or NULL;
 *        isect_info i64[8] (device): {M, largest per-tile count, #tiles in the medium /
 *        large / merge-fallback sort classes, 0, G_on, 0}.  G_on = number of Gaussians whose
 *        tile box touches the FULL grid, whatever the band: a band-sharded caller applies
 *        the reference's frame-level "no intersections -> zeros image" rule
 *        (mojosplat/render.py:73-76) from it without a collective.  Copy the record to the
 *        host to size flatten_ids and to drive ms_isect_tiles_emit.
 *
 * ms_isect_tiles_emit: scatter (depth,id) keys into their tile segments and depth-sort
 * every segment.  Order inside a tile: ascending (float bits of depth, Gaussian index) --
 * identical to a stable radix sort of (tile<<32 | depth_bits) keys emitted in Gaussian
 * order, i.e. gsplat.isect_tiles(sort=True).
 *   in : as above plus depths f32[N]; the SAME workspace the count call filled;
 *        host_info = the 8 values of isect_info as read by the host; M = host_info[0].
 *   out: flatten_ids i32[M]; isect_ids i64[M] or NULL (sorted keys (tile<<32)|depth_bits).
 *        sort_keys u64[M] and sort_tmp u64[M or 0] are caller-allocated scratch
 *        (sort_tmp is only touched when host_info[4] > 0).
 * ------------------------------------------------------------------------------------- */
size_t ms_isect_workspace_bytes(int64_t N, int tile_w, int tile_h);

int ms_isect_tiles_count(int64_t N, const float *means2d, const int32_t *radii, int tile_size,
                         int tile_w, int tile_h, int row_begin, int row_end, void *workspace,
                         size_t workspace_bytes, int32_t *tiles_per_gauss, int32_t *tile_ranges,
                         int64_t *isect_info, void *stream);

int ms_isect_tiles_emit(int64_t N, const float *means2d, const int32_t *radii,
                        const float *depths, int tile_size, int tile_w, int tile_h,
                        int row_begin, int row_end, void *workspace, size_t workspace_bytes,
                        const int32_t *tile_ranges, const int64_t *host_info, int tight, int lazy,
                        float depth_near, float depth_far, uint64_t *sort_keys,
                        uint64_t *sort_tmp, int32_t *flatten_ids, int64_t *isect_ids,
                        void *stream);

/* ms_project_gaussians_fwd + ms_isect_tiles_count in ONE pass over the Gaussians (same outputs,
 * same semantics; the tile grid is derived from W, H, tile_size).  What ms_render_fwd starts a
 * frame with: the projected means / radii are not re-read and one kernel launch is saved.
 *
 * isect_info_mirror (nullable): a DEVICE-VISIBLE address of pinned host memory (hipHostGetDevicePointer)
 * that receives words 0..6 of the record straight from the kernel -- no copy kernel; read it after
 * an event recorded behind this call has completed.
 * `tight` is a bit set.  Bit 1 (value 2): tile_ranges is written for the tiles of the band only
 * (for a caller whose later stages all stay inside the band).  Bit 0 (needs opacities): TIGHT binning.  gsplat.isect_tiles lists every tile of a
 * Gaussian's bounding box; ~18 % of those pairs (config 3) can never blend because the
 * alpha >= 1/255 ellipse does not reach the tile (box corners, elongated / rotated footprints).
 * Tight mode drops them (per tile row, the x-extent of the ellipse inside the row's band of pixel
 * centres; boxes of more than 64 tiles are kept whole), so every later stage handles fewer
 * intersections and the IMAGE IS UNCHANGED (the dropped pairs are ones the rasteriser would skip).
 * The lists are then no longer gsplat's: tight mode is for callers that only want pixels
 * (ms_render_fwd); M and tile_ranges count the kept pairs, isect_info[6] still counts bounding
 * boxes.  The per-Gaussian reach masks stay in the workspace: the emit that follows a tight count
 * MUST pass tight = 1 (and tight = 0 after ms_isect_tiles_count or a non-tight count).
 * Bit 2 (value 4, with bit 0, even tile_size, N < 2^28): BLOCK MASKS, what ms_render_fwd's split frames
 * bin with.  The tile box of a Gaussian is derived from its gsplat box on the HALF-tile grid (bits 3 / 4:
 * that grid has 2 tile_w - 1 columns / 2 tile_h - 1 rows), reach masks are kept per half-tile cell, and
 * every emitted key carries `id << 4 | blocks` in its low word (blocks: the 2x2 half-tile blocks of
 * the tile, bit 2 dy + dx, that hold exactly what a grid of half-size tiles would list there).  The
 * emit that follows must pass the same bits.
 *
 * lazy != 0 on the emit calls: LAZY SORTING, also for pixel-only callers.  Tiles of more than 1024
 * entries get only their front (about the 1024 nearest entries) selected and sorted; the workspace
 * then holds, per tile, the length of that sorted front, and flatten_ids beyond it is undefined.
 * depth_near / depth_far (> 0, the camera planes every surviving depth lies between) let the
 * selection use fixed depth buckets and skip a pass; 0, 0 = unknown.  Only ms_render_fwd's
 * rasteriser understands such lists (it redoes a tile whose front did not saturate its pixels);
 * pass lazy = 0 for lists that anyone else reads.  Bits 1-2 of `lazy`: front level, fronts 2^level
 * times as deep (up to the 4096 entries of LDS room).  Bit 3 of `lazy` on the SPECULATIVE emit: the caller
 * expects no tile of more than 1024 entries (its previous frame had none) -- only the short lists are
 * sorted, and the caller must redo the frame if the size record then reports such tiles.
 * MOJOSPLAT_LAZY_SORT=0 in the environment makes ms_render_fwd sort fully. */
int ms_project_isect_count(int64_t N, const float *means3d, const float *scales, int scales_are_log,
                           const float *quats, const float *opacities, const float *viewmat, float fx,
                           float fy, float cx, float cy, int W, int H, float eps2d, float near_plane,
                           float far_plane, float radius_clip, int tile_size, int row_begin,
                           int row_end, int tight, float *means2d, float *conics, float *depths,
                           int32_t *radii,
                           void *workspace, size_t workspace_bytes, int32_t *tile_ranges,
                           int64_t *isect_info, int64_t *isect_info_mirror, void *stream);

/* gsplat.isect_offset_encode: from SORTED keys (tile<<32|depth_bits) to per-tile start
 * offsets i32[tile_h*tile_w] (empty tiles inherit the next start; trailing tiles get M). */
int ms_isect_offset_encode(int64_t M, const int64_t *isect_ids_sorted, int tile_w, int tile_h,
                           int32_t *offsets, void *stream);

/* ---------------------------------------------------------------------------------------
 * Rasteriser forward: per tile, front-to-back alpha compositing of its sorted list.
 *   in : means2d f32[N,2], conics f32[N,3], colors [N,CDIM] (f32 or f16, CDIM 1..32),
 *        opacities f32[N], backgrounds f32[CDIM] or NULL, tile_ranges i32[th,tw,2],
 *        flatten_ids i32[M].
 *   out: render_colors f32[H,W,CDIM]; render_alphas f32[H,W] or NULL; last_ids i32[H,W]
 *        or NULL (index into flatten_ids of the last contributing intersection).
 *   Only tiles in rows [tile_row_begin, tile_row_end) are rendered (0, tile_h = whole image;
 *   a band for multi-GPU sharding); output pointers always address the FULL image.
 * ------------------------------------------------------------------------------------- */
int ms_rasterize_to_pixels_3dgs_fwd(int64_t N, int64_t M, const float *means2d,
                                    const float *conics, const void *colors, int color_dtype,
                                    int CDIM, const float *opacities, const float *backgrounds,
                                    int W, int H, int tile_size, int tile_row_begin,
                                    int tile_row_end, const int32_t *tile_ranges,
                                    const int32_t *flatten_ids, float *render_colors,
                                    float *render_alphas, int32_t *last_ids, void *stream);

/* Rasteriser backward (gsplat rasterize_to_pixels backward semantics, absgrad off).
 *   in : forward inputs + render_alphas, last_ids from the forward,
 *        v_render_colors f32[H,W,CDIM], v_render_alphas f32[H,W] or NULL.
 *   out: v_means2d f32[N,2], v_conics f32[N,3], v_colors f32[N,CDIM], v_opacities f32[N];
 *        ACCUMULATED INTO (caller zero-fills, gsplat's convention) when overwrite == 0;
 *        OVERWRITTEN (no zero-fill needed) when overwrite != 0.                            */
int ms_rasterize_to_pixels_3dgs_bwd(int64_t N, int64_t M, const float *means2d,
                                    const float *conics, const float *colors, int CDIM,
                                    const float *opacities, const float *backgrounds, int W,
                                    int H, int tile_size, const int32_t *tile_ranges,
                                    const int32_t *flatten_ids, const float *render_alphas,
                                    const int32_t *last_ids, const float *v_render_colors,
                                    const float *v_render_alphas, float *v_means2d,
                                    float *v_conics, float *v_colors, float *v_opacities,
                                    void *workspace, size_t workspace_bytes, int overwrite,
                                    void *stream);
/* scratch for the packed-gradient path of the backward rasteriser (0 = not needed / not used:
 * without it, or for CDIM > 4, the call still works through the one-atomic-per-component path) */
size_t ms_rasterize_bwd_workspace_bytes(int64_t N, int CDIM);

/* Projection backward: gradients of (means2d, conics, depths) w.r.t. means3d, scales
 * (w.r.t. the log-scales when scales_are_log), quats.  Culled Gaussians get zero grads.
 *   out: v_means3d f32[N,3], v_scales f32[N,3], v_quats f32[N,4] (overwritten).          */
int ms_project_gaussians_bwd(int64_t N, const float *means3d, const float *scales,
                             int scales_are_log, const float *quats, const float *viewmat,
                             float fx, float fy, float cx, float cy, int W, int H, float eps2d,
                             const int32_t *radii, const float *v_means2d,
                             const float *v_conics, const float *v_depths, float *v_means3d,
                             float *v_scales, float *v_quats, void *stream);

/* Backward of a DIFFERENTIABLE ms_render_fwd frame (one that was asked for render_alphas and last_ids; declared
 * below), from the scratch that frame left behind: `workspace` / `isect_buf` / `host_info` exactly as the forward
 * call returned them (same N, image and tile size, untouched since), render_alphas / last_ids its per-pixel records.
 * One call runs the backward rasteriser -- staging from the frame's ready-made records -- and the backward
 * projection: what a training loop's backward() does between two Python statements (the reference has no backward:
 * render.py:11, README.md:145).
 *   in : the forward's inputs; v_render_colors f32[H,W,CDIM], v_render_alphas f32[H,W] or NULL;
 *        render_colors f32[H,W,CDIM]: the image that frame returned, or NULL.  With it a 3-channel frame's backward
 *        rasteriser walks the lists front to back, one wave per 8x8 quad (csrc/rasterize_bwdq.hip), and last_ids may
 *        be NULL; without it the older back-to-front kernel runs and needs last_ids.
 *   out: v_means3d f32[N,3], v_scales f32[N,3] (w.r.t. the log-scales when scales_are_log), v_quats f32[N,4],
 *        v_opacities f32[N], v_colors f32[N,CDIM] -- all OVERWRITTEN.
 *   bwd_workspace: ms_render_bwd_workspace_bytes(N, CDIM) bytes of scratch.
 *   mid_event: NULL, or a hipEvent_t recorded on `stream` between the two stages (in-situ timing). */
/* Depth cut-offs of ms_render_fwd (DEPTH CUT-OFFS below): mode 0 never / 1 from min_pairs pairs on / 2 whenever possible;
 * a negative argument leaves that setting alone.  Process-wide; the defaults come from MOJOSPLAT_DEPTH_CUT /
 * MOJOSPLAT_DEPTH_CUT_MIN_PAIRS, read once.  (For tests and measurements that switch inside one process.) */
int ms_config_depth_cut(int mode, long long min_pairs);
/* Sort + rasterise in one launch (whole forward frames on plain 32-px bins): mode 0 never / 1 where the rasteriser runs two
 * waves a block by its own rule (default) / 2 on every such frame; < 0 leaves it.  MOJOSPLAT_FUSED_SORT in the environment is
 * read once; this changes the setting in-process.  The image is the same whatever the mode.  Bit 2 of the mode (1 | 4, 2 | 4)
 * keeps the clean-up launch behind such a frame: without it a bin whose sorted front runs out with pixels alive fetches the rest
 * of its list in the same workgroup, nothing is launched behind the rasteriser and bit 49 of word 7 of host_info says so
 * (never on a depth-cut frame, which keeps its clean-up launches). */
int ms_config_fused_sort(int mode);

/* ms_render_bwd in two halves, for a multi-GPU rank's differentiable BAND frame (a 3-channel frame at a tile size that is a
 * multiple of 16, rendered with render_alphas over tile rows [tile_row_begin, tile_row_end) -- or the whole frame: 0, tile_h):
 *   ms_render_bwd_rows  : the backward rasteriser on the band's lists -> rows f32[N][16], the per-Gaussian RAW sums of the
 *                         band's pixels (zeroed by the call).  Sums over disjoint bands ADD: a rank's caller all-reduces
 *                         the rows over the ranks ("per-Gaussian grads need one all-reduce") ...
 *   ms_render_bwd_finish: ... and the backward projection turns the summed rows into the gradients, identically on every rank.
 * ms_render_bwd == rows(0, tile_h) + finish.  redo_counts_host (nullable): pinned HOST i32[2] that a lazily sorted frame's
 * redo launch fills with the frame's clean-up counts (as ms_render_redo_counts would, without a copy of its own; valid once an
 * event recorded behind the call has completed; untouched for a fully sorted frame).
 * Round 6: the workspace of ms_render_fwd ends with a region of ms_render_bwd_rows_bytes(N) bytes (at
 * ms_render_workspace_bytes(N, tile_w, tile_h) - ms_render_bwd_rows_bytes(N)) that a differentiable 3-channel frame's
 * rasteriser zeroes on its way (bit 15 of host_info[7] says it did): handed exactly that address as `rows`, the call skips its
 * own memset; any other buffer is zeroed by the call as before.
 * No reference counterpart (render.py:11; README.md:145). */
size_t ms_render_bwd_rows_bytes(int64_t N);
int ms_render_bwd_rows(int64_t N, int CDIM, int W, int H, int tile_size, int tile_row_begin, int tile_row_end,
                       const float *backgrounds, const void *workspace, size_t workspace_bytes, const void *isect_buf,
                       size_t isect_bytes, const int64_t *host_info, const float *render_colors, const float *render_alphas,
                       const float *v_render_colors, const float *v_render_alphas, float *rows, int32_t *redo_counts_host,
                       void *stream);
int ms_render_bwd_finish(int64_t N, const float *means3d, const float *scales, int scales_are_log, const float *quats,
                         const float *opacities, int CDIM, const float *viewmat, float fx, float fy, float cx, float cy,
                         int W, int H, float eps2d, const float *rows, float *v_means3d, float *v_scales, float *v_quats,
                         float *v_opacities, float *v_colors, void *stream);

/* 3DGS densification statistics (adaptive density control: Kerbl et al. 2023; gsplat's default strategy), accumulated
 * over the views of a training step into three caller-owned buffers f32[N] (non-null, 4-byte aligned, not zeroed by the
 * library).  For every Gaussian i ALIVE in the view -- radii > 0 under the frame's own projection
 * (ms_project_gaussians_fwd with the opacities, near_plane / far_plane, eps2d and radius_clip 0) -- with g = dL/dmeans2d
 * of the view in pixels:
 *   count[i]     += 1
 *   grad2d[i]    += sqrt((g.x * W / 2)^2 + (g.y * H / 2)^2)          (the gradient in NDC units)
 *   max_radii[i]  = max(max_radii[i], max(radius.x, radius.y) / max(W, H))
 * A Gaussian alive but never blended counts, with a zero gradient; one that is not alive is left untouched.
 *   ms_render_bwd_finish_densify: ms_render_bwd_finish (same arguments, same gradients bit for bit) that also updates the
 *     statistics of the frame: the backward projection re-projects each Gaussian for the verdict and the radii (a lean
 *     differentiable frame writes no radii) and takes g from the rows it is finishing anyway.  The rows must be the
 *     whole frame's (one rank's band rows summed over the ranks are).
 *   ms_densify_stats_update: the same update for a caller that already holds v_means2d f32[N,2] and the forward's
 *     radii i32[N,2] (both 8-byte aligned) -- the per-stage path.
 * One backward of a view calls either entry point once.  No reference counterpart (render.py:11). */
int ms_render_bwd_finish_densify(int64_t N, const float *means3d, const float *scales, int scales_are_log,
                                 const float *quats, const float *opacities, int CDIM, const float *viewmat, float fx,
                                 float fy, float cx, float cy, int W, int H, float eps2d, const float *rows,
                                 float *v_means3d, float *v_scales, float *v_quats, float *v_opacities, float *v_colors,
                                 float near_plane, float far_plane, float *grad2d, float *count, float *max_radii,
                                 void *stream);
int ms_densify_stats_update(int64_t N, int W, int H, const int32_t *radii, const float *v_means2d, float *grad2d,
                            float *count, float *max_radii, void *stream);

/* Bins the clean-up pass of a finished ms_render_fwd frame had to redo (lazily sorted fronts that ran out with pixels
 * alive): host_counts i32[2] = {all redone bins, those redone for their depth cut-off}, copied asynchronously on `stream`
 * from the frame's `workspace` (host_counts: pinned HOST memory; valid once an event recorded behind the call has
 * completed).  Frames on cached scratch learn the same number from the NEXT frame's host_info[5]; a differentiable frame
 * owns fresh scratch, so its caller asks here (behind ms_render_bwd) and chooses MS_RENDER_FRONT_LEVEL / MS_RENDER_FULL_SORT
 * for the next step from it.  No reference counterpart (the reference has no backward: render.py:11). */
int ms_render_redo_counts(const void *workspace, size_t workspace_bytes, int64_t N, int tile_w, int tile_h,
                          int32_t *host_counts, void *stream);

size_t ms_render_bwd_workspace_bytes(int64_t N, int CDIM);
int ms_render_bwd(int64_t N, const float *means3d, const float *scales, int scales_are_log, const float *quats,
                  const float *opacities, const float *colors, int CDIM, const float *viewmat, float fx, float fy,
                  float cx, float cy, int W, int H, float eps2d, int tile_size, const float *backgrounds,
                  const void *workspace, size_t workspace_bytes, const void *isect_buf, size_t isect_bytes,
                  const int64_t *host_info, const float *render_colors, const float *render_alphas,
                  const int32_t *last_ids, const float *v_render_colors, const float *v_render_alphas, float *v_means3d,
                  float *v_scales, float *v_quats, float *v_opacities, float *v_colors, void *bwd_workspace,
                  size_t bwd_workspace_bytes, void *mid_event, void *stream);

/* ---------------------------------------------------------------------------------------
 * Gradients w.r.t. the camera pose (pose refinement, SLAM-style tracking, bundle-adjusting 3DGS; gsplat's v_viewmats).
 * Each entry point below is its namesake above with three more arguments before `stream`, and computes exactly what its
 * namesake computes -- every other output bit for bit, the densification statistics included -- plus:
 *   v_viewmat f32[16] (ms_project_gaussians_bwd_pose, ms_render_bwd_finish_pose, ms_render_bwd_finish_densify_pose,
 *     ms_render_bwd_pose): dL/d(viewmat), the row-major world->camera [R | t; 0 0 0 1] the call was given -- through the
 *     camera-space means (p_c = R p + t) and covariances (R Sigma R^T) of the Gaussians the backward differentiates;
 *     OVERWRITTEN, bottom row 0.
 *   v_campos f32[3] (ms_spherical_harmonics_bwd_pose): dL/d(cam_x, cam_y, cam_z) through the viewing directions;
 *     OVERWRITTEN.  (The camera centre is -R^T t; the caller chains it into the view matrix.)
 *   pose_scratch: ms_pose_scratch_bytes(N) bytes, 16-byte aligned, caller-owned: one 64-byte partial sum per workgroup
 *     of 256 Gaussians, written by the backward kernel and summed by a one-workgroup launch behind it (no atomics).
 *     Its contents are garbage before and after the call.
 * The sum runs in an order that depends on N alone: the result is bitwise reproducible from run to run.
 * v_viewmat / v_campos NULL: exactly the namesake's work (the scratch is not touched and may be NULL).  N == 0 or an
 * empty frame: zeros.  No reference counterpart (the reference is forward-only: render.py:11). */
size_t ms_pose_scratch_bytes(int64_t N);
int ms_project_gaussians_bwd_pose(int64_t N, const float *means3d, const float *scales, int scales_are_log,
                                  const float *quats, const float *viewmat, float fx, float fy, float cx, float cy, int W,
                                  int H, float eps2d, const int32_t *radii, const float *v_means2d, const float *v_conics,
                                  const float *v_depths, float *v_means3d, float *v_scales, float *v_quats,
                                  float *v_viewmat, void *pose_scratch, size_t pose_scratch_bytes, void *stream);
int ms_render_bwd_finish_pose(int64_t N, const float *means3d, const float *scales, int scales_are_log, const float *quats,
                              const float *opacities, int CDIM, const float *viewmat, float fx, float fy, float cx, float cy,
                              int W, int H, float eps2d, const float *rows, float *v_means3d, float *v_scales, float *v_quats,
                              float *v_opacities, float *v_colors, float *v_viewmat, void *pose_scratch,
                              size_t pose_scratch_bytes, void *stream);
int ms_render_bwd_finish_densify_pose(int64_t N, const float *means3d, const float *scales, int scales_are_log,
                                      const float *quats, const float *opacities, int CDIM, const float *viewmat, float fx,
                                      float fy, float cx, float cy, int W, int H, float eps2d, const float *rows,
                                      float *v_means3d, float *v_scales, float *v_quats, float *v_opacities,
                                      float *v_colors, float near_plane, float far_plane, float *grad2d, float *count,
                                      float *max_radii, float *v_viewmat, void *pose_scratch, size_t pose_scratch_bytes,
                                      void *stream);
int ms_render_bwd_pose(int64_t N, const float *means3d, const float *scales, int scales_are_log, const float *quats,
                       const float *opacities, const float *colors, int CDIM, const float *viewmat, float fx, float fy,
                       float cx, float cy, int W, int H, float eps2d, int tile_size, const float *backgrounds,
                       const void *workspace, size_t workspace_bytes, const void *isect_buf, size_t isect_bytes,
                       const int64_t *host_info, const float *render_colors, const float *render_alphas,
                       const int32_t *last_ids, const float *v_render_colors, const float *v_render_alphas,
                       float *v_means3d, float *v_scales, float *v_quats, float *v_opacities, float *v_colors,
                       void *bwd_workspace, size_t bwd_workspace_bytes, void *mid_event, float *v_viewmat,
                       void *pose_scratch, size_t pose_scratch_bytes, void *stream);
int ms_spherical_harmonics_bwd_pose(int64_t N, int K, int degree, const float *means3d, float cam_x, float cam_y,
                                    float cam_z, const float *coeffs, const int32_t *radii, int add_half_and_clamp,
                                    const float *colors_fwd, const float *v_colors, float *v_coeffs, float *v_means3d,
                                    float *v_campos, void *pose_scratch, size_t pose_scratch_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Spherical-harmonic colours (view dependent).  The reference leaves SH evaluation as a TODO
 * that only slices channels (mojosplat/render.py:82-87); this is the operator that belongs
 * there, in gsplat's convention (spherical_harmonics + the "+0.5, clamp at 0" of its
 * rasterization()): real SH of degree <= 4, 3DGS signs, coefficient index l*(l+1)+m.
 *   in : means3d f32[N,3]; camera position (world) cam_x/y/z; coeffs f32[N,K,3] with
 *        K >= (degree+1)^2 (only the first (degree+1)^2 are read); radii i32[N,2] or NULL:
 *        Gaussians with a zero radius are skipped (colour 0, zero gradients);
 *        add_half_and_clamp: colour = max(sum + 0.5, 0) when non-zero, the raw sum otherwise.
 *   out: colors f32|f16[N,3].
 * Backward: v_colors f32[N,3] -> v_coeffs f32[N,K,3] (overwritten; zeros beyond the degree) and
 * / or v_means3d f32[N,3] (overwritten); either may be NULL.  colors_fwd (f32, the forward
 * output) is required with add_half_and_clamp.
 * ------------------------------------------------------------------------------------- */
int ms_spherical_harmonics_fwd(int64_t N, int K, int degree, const float *means3d, float cam_x,
                               float cam_y, float cam_z, const float *coeffs, const int32_t *radii,
                               int add_half_and_clamp, int color_dtype, void *colors, void *stream);
int ms_spherical_harmonics_bwd(int64_t N, int K, int degree, const float *means3d, float cam_x,
                               float cam_y, float cam_z, const float *coeffs, const int32_t *radii,
                               int add_half_and_clamp, const float *colors_fwd, const float *v_colors,
                               float *v_coeffs, float *v_means3d, void *stream);

/* ---------------------------------------------------------------------------------------
 * Whole forward path in one call: replaces the three stage calls that
 * render_gaussians makes (mojosplat/render.py:63-101) when the caller does not need the
 * intermediates.  Projection outputs, tile ranges and the sorted list live in caller-owned
 * scratch:
 *   workspace  : ms_render_workspace_bytes(N, tile_w, tile_h) bytes, fixed per (N, image);
 *   isect_buf  : ms_render_isect_bytes(M, merge) bytes, data dependent (M = host_info[0]; a split
 *                frame -- tile_size 16, plain forward, see below -- counts the entries of its 32-px
 *                bins and needs 28 bytes for each: keys, list words, 4 block lists).  If it is too small
 *                the call returns MS_ERR_WORKSPACE with host_info[5] = bytes needed and all
 *                M-independent work done; grow the buffer and call again with resume = 1.
 *   host_info  : HOST memory (pinned), i64[8]; receives isect_info (see
 *                ms_isect_tiles_count).  This is the only entry point that waits on the
 *                device: with sync_event == NULL one hipStreamSynchronize between count and
 *                emit; with a hipEvent_t in sync_event and an isect_buf sized by an earlier
 *                frame, emit + rasterise are enqueued speculatively against the buffer's
 *                capacity BEFORE the wait, so the GPU never idles (an overflowing frame is
 *                detected and redone on the exact path).
 *   resume     : which half of the frame to run (enum below).  MS_RENDER_WHOLE = everything;
 *                MS_RENDER_RESUME = the redo after MS_ERR_WORKSPACE; MS_RENDER_BEGIN enqueues
 *                the frame (speculatively where it can) and returns WITHOUT waiting, and a
 *                later MS_RENDER_FINISH call with the same arguments does the wait, the check
 *                and, if needed, the exact redo -- so a host that renders independent frames
 *                (several views, or consecutive frames of a pipeline) can enqueue frame k+1
 *                before it waits for frame k's size record.  Every frame in flight needs its
 *                own workspace, isect_buf, host_info and sync_event; host_info[7] is the
 *                library's own slot between BEGIN and FINISH.
 *                The record a frame leaves in host_info is also the NEXT frame's hint when the same
 *                host_info is passed again (what a caller that renders frame after frame does): its M
 *                sizes nothing but launch shapes, and a previous frame without any list beyond the
 *                small sort class (1024 entries) makes the library bet that this one has none either
 *                and launch the short sorts alone -- a lost bet is read off this frame's own record
 *                and the frame redone on the exact path, like an overflowing one.  Pass a zeroed
 *                record to start afresh.
 *   stage_events: NULL, or 4 hipEvent_t recorded on `stream` at: start, after projection,
 *                after binning, after rasterisation (for in-situ kernel timing).
 * LEAN FRAMES.  A plain forward frame with CDIM == 3 keeps NO projected arrays in `workspace`: its rasteriser reads
 * the 48-byte records the count kernel leaves per Gaussian, its scatter kernel a 12-byte (tile box, depth bits, reach
 * mask) record; means2d / conics / depths / radii are only written for frames that are asked for render_alphas or
 * last_ids (what the older backward rasteriser needs) and for other channel counts.
 * DEPTH CUT-OFFS.  A lean sync-free frame on plain bins (tile_size 32 / 64, up to 255 bins a side) -- the whole grid or,
 * since round 4, a band of it (a rank's share of a frame: pre-culled or not, MS_RENDER_ROWS16 or not) --
 * whose predecessor ON THE SAME host_info / workspace / grid / band was such a frame too, and held at least 6 M pairs
 * (MOJOSPLAT_DEPTH_CUT_MIN_PAIRS; a band: that number scaled by its share of the rows), takes that predecessor's per-bin
 * depth cut-offs -- the depth at which each bin's
 * lazily sorted front ended, plus 1/16 octave -- and neither counts into the lists, scatters, sorts nor writes records
 * for the (Gaussian, bin) pairs behind them: host_info[0] still counts every pair (the buffer keeps room for them),
 * the lists hold the near ones.  The frame is exact whatever the cut-offs are: a bin whose pixels outlive its list
 * gets its dropped pairs -- and their Gaussians' records -- back in the clean-up launches (which project the
 * Gaussians again), and its cut-off is lifted for the next frame.  host_info[5] of the next record reports such bins in its
 * high 32 bits (the low 32: bins whose sorted FRONT was too short, as before); bits 6-8 and 16-47 of host_info[7]
 * are the library's bookkeeping for it (this frame took the cut; it left cut-offs, in which of two buffers, for which
 * grid and band).  MOJOSPLAT_DEPTH_CUT=0 in the environment (read once; ms_config_depth_cut changes it in-process) switches it off, =2 takes the cut whatever the
 * previous frame held.  A frame that fails its speculation is started over without the cut.
 * SPLIT FRAMES.  A plain forward frame (no render_alphas / last_ids, CDIM <= 4) at tile_size 16 over the
 * whole image or a band of >= 16 tile rows is binned on 32-px bins with block masks (see `tight`), and
 * the sort kernels cut every bin's sorted list into the lists of its four 16x16 blocks, which is what
 * the rasteriser walks: 40 % fewer (Gaussian, bin) pairs to scatter and sort, the same pairs to
 * rasterise, the same frame bit for bit.  MOJOSPLAT_SPLIT=0 in the environment bins such frames on
 * 16-px tiles directly.
 * [tile_row_begin, tile_row_end) restricts binning and rasterisation to a band of tile rows
 * (0, tile_h = whole image); render_colors always addresses the FULL image.
 * Whole-image calls: no bounding box on the grid yields a ZERO image (reference render.py:73-76),
 * otherwise render_colors f32[H,W,CDIM] = composited colours + T * background.  render_alphas
 * f32[H,W] and last_ids i32[H,W] (both nullable) are the per-pixel records the backward
 * rasteriser needs (see ms_rasterize_to_pixels_3dgs_fwd).
 * ------------------------------------------------------------------------------------- */
enum { MS_RENDER_WHOLE = 0, MS_RENDER_RESUME = 1, MS_RENDER_BEGIN = 2, MS_RENDER_FINISH = 3,
       MS_RENDER_FULL_SORT = 0x100, /* or-ed into `resume`: no lazy sorting for this frame */
       MS_RENDER_FRONT_LEVEL = 0x200, /* x 0..3, or-ed into `resume`: lazily sorted fronts 2^level times as deep
                                        (a caller whose previous frame needed the clean-up pass, host_info[5] > 0) */
       MS_RENDER_ROWS16 = 0x800, /* or-ed into `resume`: [tile_row_begin, tile_row_end) counts rows of 16 pixels whatever
                                   tile_size (a multiple of 16) is: the band is binned on the tile rows that cover
                                   it and rasterised on exactly those 16-px rows -- a multi-GPU rank keeps its band
                                   while the bin size follows the scene (32- / 64-px bins for dense scenes) */
       MS_RENDER_DEFER_CLEANUP = 0x1000 /* ms_band_frame.flags only (ms_render_fwd ignores it): the band's clean-up launches --
                                   up to four, empty on almost every frame -- are not enqueued behind the rasteriser;
                                   ms_render_band_finish waits for the END of the band instead of its size record, reads the
                                   rasteriser's verdict from word 8 of the lane's pinned record (host_info must then be
                                   i64[16]) and enqueues them only when a bin asked for them.  For bands in flight behind
                                   each other on two lanes: the GPU has the other band to run while the host waits. */ };
size_t ms_render_workspace_bytes(int64_t N, int tile_w, int tile_h);
size_t ms_render_isect_bytes(int64_t M, int with_merge_scratch);
int ms_render_fwd(int64_t N, const float *means3d, const float *scales, int scales_are_log,
                  const float *quats, const float *opacities, const void *colors, int color_dtype,
                  int CDIM, const float *viewmat, float fx, float fy, float cx, float cy, int W,
                  int H, float eps2d, float near_plane, float far_plane, int tile_size,
                  int tile_row_begin, int tile_row_end, const float *backgrounds, void *workspace,
                  size_t workspace_bytes,
                  void *isect_buf, size_t isect_bytes, int64_t *host_info, int resume,
                  float *render_colors, float *render_alphas, int32_t *last_ids,
                  void **stage_events, void *sync_event, void *stream);

/* ---------------------------------------------------------------------------------------
 * Camera batch: the same Gaussians from C cameras in one call -> render_colors f32[C,H,W,CDIM].
 * The reference's kernels carry a camera dimension (kernels/projection.mojo:32-37,
 * kernels/rasterization.mojo:66) that every wrapper pins to 1 (projection.py:431,
 * rasterization.py:175); this is the entry point with C > 1.  View v equals what ms_render_fwd
 * renders for camera v, bit for bit (incl. the zeros image for a view with nothing on the grid).
 * MI355X mapping: a frame is a VALU-bound rasteriser behind latency-bound binning kernels and one
 * host wait for its size record, so the batch keeps n_lanes (1..4, normally 2) views IN FLIGHT on
 * as many streams: view v+1's projection / binning overlaps view v's rasteriser and is enqueued
 * (MS_RENDER_BEGIN) before the host waits for view v's record (MS_RENDER_FINISH).  A pass over
 * (camera, Gaussian) in one kernel would save nothing: the projection is VALU bound, not
 * bandwidth bound.
 *   viewmats   : DEVICE f32[C,16], row-major world->camera;  intrinsics: HOST f32[C,4] = fx fy cx cy
 *   lanes      : HOST array of n_lanes scratch sets, each as ms_render_fwd wants them (workspace of
 *                ms_render_workspace_bytes, isect_buf, pinned host_info i64[8], a hipEvent_t, a
 *                hipStream_t).  The caller orders the lanes' streams after its inputs and itself after
 *                the lanes' streams.
 *   flags      : MS_RENDER_FULL_SORT / MS_RENDER_FRONT_LEVEL bits applied to every view (0 = defaults)
 *   counts     : HOST i64[C] or NULL: intersections of each view
 *   views_done : HOST, in: first view to render (0); out: views completed.  On MS_ERR_WORKSPACE the
 *                isect_buf of lane *need_lane is too small for view *views_done (*need_isect_bytes
 *                needed): nothing is in flight any more; grow it and call again with the same arrays.
 * ------------------------------------------------------------------------------------- */
typedef struct ms_view_lane {
    void *workspace;
    size_t workspace_bytes;
    void *isect_buf;
    size_t isect_bytes;
    int64_t *host_info;
    void *sync_event;
    void *stream;
} ms_view_lane;
int ms_render_fwd_batch(int C, int64_t N, const float *means3d, const float *scales, int scales_are_log,
                        const float *quats, const float *opacities, const void *colors, int color_dtype,
                        int CDIM, const float *viewmats, const float *intrinsics, int W, int H, float eps2d,
                        float near_plane, float far_plane, int tile_size, const float *backgrounds, int n_lanes,
                        const ms_view_lane *lanes, int flags, float *render_colors, int64_t *counts,
                        int *views_done, size_t *need_isect_bytes, int *need_lane);

/* ---------------------------------------------------------------------------------------
 * A multi-GPU rank's BAND of a frame, in two calls (round 5).  No reference counterpart: the reference has no distributed
 * path (mojosplat/binning.py:83 is a dead comment); what a band bins is what mojosplat/binning.py:73-84 bins, restricted
 * to the band's tile rows.
 *
 * ms_scene: the Gaussians as ms_render_fwd takes them one by one, built ONCE per scene by the caller -- plus, for a
 * PREPARED scene, the bounds of every block of block_size consecutive Gaussians (ms_scene_prepare): when the Gaussians are
 * stored in a spatially coherent order (the caller sorts them once, e.g. along a Morton curve of the means) those boxes
 * are small, the band pre-cull skips every block that cannot reach the band without reading it, and the count kernel's
 * gathers through the band's candidate list coalesce.  block_bounds == NULL: any order, no bounds (as ms_render_fwd).
 * The bounds must describe the arrays AS THEY ARE: recompute them after the means or scales change.
 *   block_bounds: the buffer ms_scene_prepare fills (ms_scene_block_bounds_bytes of it): f32[n_blocks][8] = {min x, min y, min z
 *   of the block's means, its largest LINEAR scale, max x, max y, max z, 0}, then f32[N][4] = every Gaussian's mean and largest
 *   linear scale -- the band pre-cull's own 16-byte record (one load instead of 24 bytes in two)
 *
 * ms_band_lane: one scratch set (as ms_render_fwd wants it: workspace, isect_buf, pinned host_info i64[8], sync_event) with the
 * hipStream_t the band runs on and two hipEvent_t for the ordering around it; built once per lane, isect_buf / isect_bytes
 * updated when the buffer grows.  One frame at a time per lane; frames on different lanes overlap.
 *
 * ms_render_band_begin : caller_stream -> lane (in_event), then the whole band enqueued on lane->stream (MS_RENDER_BEGIN:
 *                        speculatively, no host wait).
 * ms_render_band_finish: waits for the band's size record, checks it, redoes the band on the exact path if the speculation
 *                        did not hold (MS_ERR_WORKSPACE as ms_render_fwd: grow isect_buf to lane->host_info[5] bytes and call
 *                        again with resume = 1), then lane -> caller_stream (out_event); status i64[4] (HOST) = {Gaussians on
 *                        the grid -- of a pre-culled band: of its candidates --, 1 if the library pre-culled the band, pairs
 *                        in the band, the frame's flag word (host_info[7])}.
 * flags: MS_RENDER_ROWS16 / MS_RENDER_FULL_SORT / MS_RENDER_FRONT_LEVEL bits, as ms_render_fwd's `resume`; MS_RENDER_DEFER_CLEANUP
 *        (the lane's host_info is then i64[16]; when the verdict is clean the finishing half enqueues NOTHING: the host has
 *        seen the band end, so whatever it enqueues on caller_stream afterwards is behind it).
 * render_colors addresses image row 0 (rows outside the band are never touched), as for ms_render_fwd.
 * ------------------------------------------------------------------------------------- */
typedef struct ms_scene {
    int64_t N;
    const float *means3d, *scales;
    int scales_are_log;
    const float *quats, *opacities;
    const void *colors;
    int color_dtype, CDIM;
    const float *block_bounds;   /* NULL: not a prepared scene */
    int block_size;              /* Gaussians per block: a power of two >= 64 */
    int64_t n_blocks;
} ms_scene;
typedef struct ms_band_lane {
    void *workspace;
    size_t workspace_bytes;
    void *isect_buf;
    size_t isect_bytes;
    int64_t *host_info;
    void *sync_event, *stream, *in_event, *out_event;
} ms_band_lane;
typedef struct ms_band_frame {
    const ms_scene *scene;
    const float *viewmat;        /* DEVICE f32[16] */
    float fx, fy, cx, cy;
    int W, H;
    float eps2d, near_plane, far_plane;
    int tile_size, row_begin, row_end, flags;
    const float *backgrounds;
    float *render_colors;
    void **stage_events;         /* NULL, or 4 hipEvent_t as ms_render_fwd's (in-situ kernel timing) */
} ms_band_frame;
size_t ms_scene_block_bounds_bytes(int64_t N, int block_size);
int ms_scene_prepare(int64_t N, const float *means3d, const float *scales, int scales_are_log, int block_size,
                     float *block_bounds, void *stream);
int ms_render_band_begin(const ms_band_frame *frame, const ms_band_lane *lane, void *caller_stream);
int ms_render_band_finish(const ms_band_frame *frame, const ms_band_lane *lane, void *caller_stream, int resume,
                          int64_t *status);

/* Where ms_render_fwd keeps its intermediates inside `workspace` (byte offsets), for callers that
 * go on to differentiate the frame: offsets[0..4] = means2d f32[N,2], conics f32[N,3],
 * depths f32[N], radii i32[N,2], tile_ranges i32[tile_h,tile_w,2]; offsets[5] = total bytes.
 * The sorted Gaussian ids are the i32 array at byte offset align256(8 * capacity) of isect_buf on a
 * frame that ran sync-free (capacity = (isect_bytes - 512) / 12 entries), and at
 * align256(8 * M) * (1 + merge) on one that took the exact path (host_info[7] & 4 after the call;
 * merge = host_info[4] > 0).
 * A differentiable frame (render_alphas given, three channels, tiles of 16 or 32 px) also leaves, behind those ids, the
 * lists of its 8x8 quads for ms_render_bwd (host_info[7] & 8192): q = 4 or 16 quads a tile, 4 q more bytes per entry --
 * capacity = (isect_bytes - 768) / (12 + 4 q) on the sync-free path, + align256(4 q M) bytes on the exact one (the size
 * ms_render_fwd asks for in host_info[5] includes them). */
int ms_render_workspace_layout(int64_t N, int tile_w, int tile_h, size_t *offsets);
/* Byte offset, in a frame's workspace, of its per-tile front counts (tile_w * tile_h int32: how many entries of a list
 * beyond 1024 are sorted; undefined for shorter lists).  For tests and measurements. */
int ms_render_front_count_offset(int64_t N, int tile_w, int tile_h, size_t *offset);

/* ms_isect_tiles_emit without the host knowing M: `isect_info_dev` is the DEVICE record written
 * by ms_isect_tiles_count, `capacity` the number of entries sort_keys / flatten_ids can hold.
 * Every kernel clamps to the capacity; the caller must afterwards check (from its own copy of
 * the record) that M <= capacity and that no tile is in the merge-fallback class, and redo the
 * frame with ms_isect_tiles_emit otherwise.  prev_info_host (HOST, nullable) is the record of
 * the previous frame: when its large-class count is 0 the large-class sort is not launched, and
 * the caller must also redo the frame if this frame's large-class count turns out non-zero.
 * Used by ms_render_fwd for sync-free frames. */
int ms_isect_tiles_emit_speculative(int64_t N, const float *means2d, const int32_t *radii,
                                    const float *depths, int tile_size, int tile_w, int tile_h,
                                    int row_begin, int row_end, void *workspace,
                                    size_t workspace_bytes, const int32_t *tile_ranges,
                                    const int64_t *isect_info_dev, int64_t capacity,
                                    const int64_t *prev_info_host, int tight, int lazy,
                                    float depth_near, float depth_far, uint64_t *sort_keys,
                                    int32_t *flatten_ids, void *stream);

/* ---------------------------------------------------------------------------------------
 * Photometric loss of 3DGS training (csrc/loss.hip; the definition: mojosplat_amd/loss.py, photometric_loss_torch):
 *   loss = (1 - lambda_dssim) * mean|img - target| + lambda_dssim * (1 - mean SSIM(img, target)),
 * SSIM per channel under the 11x11 Gaussian window (sigma 1.5) with 5 pixels of zero padding, C1 = 0.01^2, C2 = 0.03^2.
 * Replaces nothing in the reference (it is forward-only, README.md:145); the CUDA stack's fused-ssim extension.
 *   img, target : f32[B,H,W,C], channel innermost -- the tensor ms_render_fwd writes (B = 1); C in 1..4.
 *   workspace   : ms_photometric_loss_workspace_bytes(B, H, W, C, keep_for_backward) bytes (0: bad sizes).  With
 *                 keep_for_backward != 0 the forward leaves three derivative planes there (12 bytes per image element) and
 *                 the SAME workspace, untouched, goes to ms_photometric_loss_bwd; with 0 it holds partial sums only.
 *   out3        : f32[3] (DEVICE) = {loss, l1, ssim}, overwritten.
 *   v_loss      : f32[1] (DEVICE): dL/dloss, read by the kernel -- never brought to the host.
 *   v_img       : f32[B,H,W,C] = dL/dimg, overwritten (target is data: no gradient).
 * Two launches forward, one backward, on `stream`; no host synchronisation, no allocation, no float atomics: the same
 * inputs give the same bits on every run.  B*H*W*C above 2^31 - 1 is refused (MS_ERR_TOO_LARGE); null pointers, sizes
 * <= 0, C outside 1..4, lambda_dssim outside [0, 1] -> MS_ERR_INVALID_ARG, a short workspace -> MS_ERR_WORKSPACE, all
 * before any device work.
 * ------------------------------------------------------------------------------------- */
size_t ms_photometric_loss_workspace_bytes(int B, int H, int W, int C, int keep_for_backward);
int ms_photometric_loss_fwd(int B, int H, int W, int C, const float *img, const float *target, float lambda_dssim,
                            void *workspace, size_t workspace_bytes, int keep_for_backward, float *out3, void *stream);
int ms_photometric_loss_bwd(int B, int H, int W, int C, const float *img, const float *target, float lambda_dssim,
                            const void *workspace, size_t workspace_bytes, const float *v_loss, float *v_img,
                            void *stream);

/* ---------------------------------------------------------------------------------------
 * Optimiser step of 3DGS training (csrc/adam.hip; the definition: mojosplat_amd/optim.py, GaussianAdam with
 * backend="torch"): Adam, per element and in float32,
 *   m' = beta1 m + (1 - beta1) g,  v' = beta2 v + (1 - beta2) g g,
 *   p' = p - (lr / bias_correction1) m' / (sqrt(v') / bias_correction2_sqrt + eps)
 * -- torch.optim.Adam without amsgrad, weight decay or maximize -- for n_tensors (1..MS_ADAM_MAX_TENSORS) parameter tensors
 * in ONE launch whose workgroups are shared among the tensors in proportion to their sizes.
 * Replaces nothing in the reference (it is forward-only and updates no parameter); the CUDA stack's
 * torch.optim.Adam(fused=True) and, with a mask, gsplat's SelectiveAdam.
 *   tensors     : HOST array of n_tensors records, read during the call (the kernel receives what it needs by value):
 *                   param, exp_avg, exp_avg_sq : f32[rows, width], contiguous, updated in place
 *                   grad                       : f32[rows, width], contiguous, read
 *                   rows, width                : > 0, rows * width < 2^31; width = elements per row (3 for means, 1 for
 *                                                opacities, 48 for SH degree 3 ...)
 *                   lr, beta1, beta2, eps      : lr >= 0 and finite, betas in [0, 1), eps > 0
 *                   bias_correction1           : 1 - beta1^t,        in (0, 1] | computed by the caller in double from ITS
 *                   bias_correction2_sqrt      : sqrt(1 - beta2^t),  in (0, 1] | step count t: the device keeps no count
 *                 16-byte aligned pointers get 16-byte loads and stores; others are served element by element.
 *   visible     : u8[visible_rows] or NULL.  A row (of every tensor) whose byte is 0 is neither read nor written: its param
 *                 and moments stay bit for bit.  Rows with a non-zero byte get exactly the bits the NULL call gives them.
 *                 With a mask every tensor must have rows == visible_rows; without one visible_rows is ignored.
 * One launch on `stream` (a hipStream_t), no host synchronisation, no allocation, no atomics: the same inputs give the same
 * bits on every run.  IEEE sqrt and division, no contraction.  n_tensors outside 1..8, a null pointer, rows or width <= 0,
 * a negative or non-finite lr, a beta outside [0, 1), eps <= 0 or NaN, a bias correction outside (0, 1], a row count that
 * differs from the mask's -> MS_ERR_INVALID_ARG; a tensor of 2^31 elements or more -> MS_ERR_TOO_LARGE; all before any
 * device work.
 * ------------------------------------------------------------------------------------- */
#define MS_ADAM_MAX_TENSORS 8
typedef struct ms_adam_tensor {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t rows, width;
    double lr, beta1, beta2, eps;
    double bias_correction1, bias_correction2_sqrt;
} ms_adam_tensor;
int ms_adam_step(int n_tensors, const ms_adam_tensor *tensors, const uint8_t *visible, int64_t visible_rows, void *stream);

/* ---------------------------------------------------------------------------------------
 * The densification step of 3DGS training: clone, split and prune (csrc/densify.hip; the definition:
 * mojosplat_amd/refine.py, densify_and_prune_torch).  Replaces nothing in the reference (it is forward-only); the CUDA
 * stack's gsplat DefaultStrategy (duplicate, split, remove).  Two calls with the caller's ONE host read between them,
 * because the outputs have to be allocated:
 *
 * ms_densify_classify  decides every Gaussian in float32 (IEEE division, no contraction, scale tests in log space) and
 *                      scans the per-workgroup counts.  With g = grad2d / max(count, 1), smax = max(scales row):
 *                        high  = g > grow_grad2d          small    = smax <= log_grow
 *                        clone = high & small             split    = (high & !small) | (max_radii > grow_radius)
 *                        lowop = opacity < thr_opa        big      = (smax > log_big) | (max_radii > prune_radius)
 *                                                         childbig = (smax - float32(log 1.6) > log_big) | (max_radii > prune_radius)
 *                      flag bit 0: an original stays (!split & !lowop & !big); bit 1: a clone appears (clone & !lowop & !big);
 *                      bit 2: two children appear (split & !lowop & !childbig).
 *   grad2d, count, max_radii, opacities : f32[N];  scales : f32[N, 3], log space
 *   rules      : HOST, the thresholds, each rounded to float32 once by the caller; +inf switches a rule off; none is NaN
 *   workspace  : ms_densify_workspace_bytes(N) bytes, 16-byte aligned: the flag bytes and the scanned counts; it is what
 *                ms_densify_move reads
 *   totals     : i64[4], out: originals kept, clones, split rows (each leaves two children), source rows that leave nothing
 * ms_densify_move      writes the output rows -- [kept originals | clones | first children | second children], each
 *                      segment in ascending source row -- of up to MS_DENSIFY_MAX_TENSORS tensors per call (more: call
 *                      again with the next records) in one launch.
 *   n_kept, n_cloned, n_split : totals[0..2] of the classify call on the same workspace
 *   tensors    : HOST array of n_tensors records: src f32[N, width] -> dst f32[n_kept + n_cloned + 2 n_split, width], and kind:
 *                  MS_DENSIFY_COPY   every output row is a bit copy of its source row
 *                  MS_DENSIFY_MEAN   (width 3) originals and clones copied; the children's rows are the row outputs' below
 *                  MS_DENSIFY_SCALE  (width 3) children get src - float32(log 1.6), one float32 subtraction
 *                  MS_DENSIFY_MOMENT originals copied; clones' and children's rows are written as ZEROS
 *                16-byte loads and stores when width is a multiple of 4 and both pointers are 16-byte aligned, dwords otherwise.
 *   means3d, scales, quats (f32[N,3], [N,3], [N,4] wxyz), noise (f32[2, N, 3]), out_means3d (the MEAN record's dst), source
 *   (i64[rows out], each output row's source row): the row outputs, all six or all NULL.  Given, the call also writes `source`
 *   and both children's means, mean + R(q / |q|) (exp(scales) * noise[c]), c = 0 / 1; noise is read for split rows only.
 * No atomics, order-preserving, the same inputs give the same bits on every run; no host synchronisation, no allocation.
 * N = 0 (and, for the move, no output row) is a no-op.  A negative size, a null pointer, a NaN threshold, a kind out of range,
 * a MEAN or SCALE record whose width is not 3 -> MS_ERR_INVALID_ARG; a short workspace -> MS_ERR_WORKSPACE; a tensor of
 * 2^31 elements or more before or after -> MS_ERR_TOO_LARGE; all before any device work.
 * ------------------------------------------------------------------------------------- */
#define MS_DENSIFY_ROWS 256          /* Gaussians per workgroup of the classify and move kernels */
#define MS_DENSIFY_SCAN_SPAN 512     /* workgroup counts the scan kernel takes in one pass of its lanes */
#define MS_DENSIFY_MAX_TENSORS 16
typedef enum ms_densify_kind { MS_DENSIFY_COPY = 0, MS_DENSIFY_MEAN = 1, MS_DENSIFY_SCALE = 2, MS_DENSIFY_MOMENT = 3 } ms_densify_kind;
typedef struct ms_densify_rules {
    float grow_grad2d, log_grow, grow_radius, thr_opa, log_big, prune_radius;
} ms_densify_rules;
typedef struct ms_densify_tensor {
    const float *src;
    float *dst;
    int64_t width;
    int kind;
} ms_densify_tensor;
size_t ms_densify_workspace_bytes(int64_t N);
int ms_densify_classify(int64_t N, const float *grad2d, const float *count, const float *max_radii, const float *scales,
                        const float *opacities, const ms_densify_rules *rules, void *workspace, size_t workspace_bytes,
                        int64_t *totals, void *stream);
int ms_densify_move(int64_t N, int64_t n_kept, int64_t n_cloned, int64_t n_split, const void *workspace, size_t workspace_bytes,
                    int n_tensors, const ms_densify_tensor *tensors, const float *means3d, const float *scales,
                    const float *quats, const float *noise, float *out_means3d, int64_t *source, void *stream);

/* ---------------------------------------------------------------------------------------
 * The 3DGS-MCMC strategy (csrc/mcmc.hip; the definition: mojosplat_amd/mcmc.py, relocate_dead_torch, grow_torch,
 * inject_noise_torch).  Replaces nothing in the reference (it is forward-only); the CUDA stack's gsplat MCMCStrategy.
 * Every call enqueues on `stream` and returns: no host synchronisation, no allocation.  The only atomics are integer ones
 * (the draws of each source are counted; a count does not depend on the order), so the same inputs give the same bits.
 *
 * ms_mcmc_sample   classifies, weighs, scans and draws.  A row is dead when !(opacities[i] > thr) on the STORED value (a NaN
 *                  is dead); its weight is 0, a live row's is round(o 2^24) with o = opacities[i] (logit = 0) or its sigmoid
 *                  (logit = 1).  cum = the inclusive int64 scan, total = cum[N - 1].  Draw j: t = min(floor(draws[j] * total),
 *                  total - 1) in double, sampled[j] = the first row with cum > t (never a zero-weight row); with sampled_in
 *                  the draw is sampled_in[j] instead.  A draw whose source is out of range or dead is NOT applied:
 *                  sampled[j] = -1.
 *   grow = 0 (relocation): n_draws == N; the dead rows in ascending order are targets[0 .. n), n = their number (0 when
 *                  total == 0); sampled and targets hold -1 from n on; *n_out = n (device, may be NULL).
 *   grow = 1     : every one of the n_draws draws is made, targets[j] = N + j, *n_out = n_draws; with total == 0 no draw is
 *                  applied.
 *   opacities : f32[N];  thr : the threshold, rounded to float32 once by the caller (its logit with logit = 1)
 *   draws     : f64[n_draws], uniform in [0, 1), or NULL when sampled_in i64[n_draws] is given
 *   workspace : ms_mcmc_workspace_bytes(N) bytes, 16-byte aligned; it is what ms_mcmc_apply reads
 *   sampled, targets : i64[n_draws], out
 * ms_mcmc_apply    moves.  With values given (opacities, scales, binom: all or none -- the FIRST call after a sample), every
 *                  row's new stored opacity and scales are first computed from the old ones into the workspace, before any
 *                  row is written: a row drawn c > 0 times, n = min(c + 1, MS_MCMC_MAX_RATIO), gets
 *                    o' = -expm1(log1p(-o) / n),  D = sum_b binom[n - 1][b] o'^(b + 1),  scales += log(o / D),
 *                    opacity = clamp(o', min_opacity, 1 - 1e-7) (stored as its logit with logit = 1)
 *                  evaluated in double; a row nobody drew keeps its values.  Then, for every applied draw and every record,
 *                  in place: MS_MCMC_COPY row target <- row source; MS_MCMC_OPACITY (width 1) and MS_MCMC_SCALE (width 3)
 *                  source and target <- the new values; MS_MCMC_MOMENT source and target <- 0.  With grow = 1 the target of a
 *                  draw that was not applied becomes a copy of row 0 (and a MOMENT row of zeros).  Up to
 *                  MS_MCMC_MAX_TENSORS records per call (more: call again with the next records and no values).
 *   n_rows    : rows of every tensor: N, or N + n_draws after a grow (rows [0, N) filled by the caller)
 *   binom     : f32[51 * 51], binom[n - 1][b] = (-1)^b C(n, b + 1) / sqrt(b + 1) (0 for b >= n), formed in double and rounded
 *               once by the caller
 *   tensors   : HOST array of n_tensors records: base f32[n_rows, width] and kind.  16-byte accesses when width is a multiple
 *               of 4 and base is 16-byte aligned, dwords otherwise.
 * ms_mcmc_noise    means3d += R (exp(2 scales) * (R^T v)) = Sigma v with R = R(quats / |quats|) (wxyz),
 *                  v = noise * gate * step, gate = 1 / (1 + exp(-k ((1 - o) - x0))), o as above; float32, IEEE division and
 *                  sqrt, no contraction.  means3d, scales, noise : f32[N,3]; quats : f32[N,4]; opacities : f32[N].
 * N = 0 (and, for sample and apply, n_draws = 0) is a no-op.  A null pointer, a negative size, a misaligned pointer (float: 4
 * bytes, double and int64: 8, workspace: 16), a NaN threshold or step, a kind out of range, an OPACITY or SCALE record of
 * another width, min_opacity outside (0, 1) -> MS_ERR_INVALID_ARG; a short workspace -> MS_ERR_WORKSPACE; a tensor of 2^31
 * elements or more -> MS_ERR_TOO_LARGE; all before any device work.
 * ------------------------------------------------------------------------------------- */
#define MS_MCMC_ROWS 256             /* Gaussians (or draws) per workgroup */
#define MS_MCMC_MAX_RATIO 51         /* the relocation formula's largest n; the binomial table's side */
#define MS_MCMC_MAX_TENSORS 16
typedef enum ms_mcmc_kind { MS_MCMC_COPY = 0, MS_MCMC_OPACITY = 1, MS_MCMC_SCALE = 2, MS_MCMC_MOMENT = 3 } ms_mcmc_kind;
typedef struct ms_mcmc_tensor {
    float *base;
    int64_t width;
    int kind;
} ms_mcmc_tensor;
size_t ms_mcmc_workspace_bytes(int64_t N);
int ms_mcmc_sample(int64_t N, const float *opacities, int logit, float thr, int64_t n_draws, int grow, const double *draws,
                   const int64_t *sampled_in, void *workspace, size_t workspace_bytes, int64_t *sampled, int64_t *targets,
                   int64_t *n_out, void *stream);
int ms_mcmc_apply(int64_t N, int64_t n_draws, int64_t n_rows, int grow, void *workspace, size_t workspace_bytes,
                  const int64_t *sampled, const int64_t *targets, int n_tensors, const ms_mcmc_tensor *tensors,
                  const float *opacities, const float *scales, const float *binom, int logit, double min_opacity, void *stream);
int ms_mcmc_noise(int64_t N, float *means3d, const float *scales, const float *quats, const float *opacities,
                  const float *noise, int logit, float step, float k, float x0, void *stream);

/* ---------------------------------------------------------------------------------------
 * Exact k nearest neighbours of every point of a cloud (csrc/knn.hip; the definition: mojosplat_amd/knn.py, knn_torch).
 * Replaces nothing in the reference (it has no training); the CUDA stack's simple-knn (distCUDA2), which 3DGS sets its
 * initial scales from.  Enqueues two launches on `stream` and returns: no host synchronisation, no allocation, no atomics,
 * so the same inputs give the same bits.
 *
 * For query i and candidate j != i (self is excluded by ROW, equal points are neighbours at distance 0), in float32 with
 * every operation rounded on its own:  dx = x_i - x_j, dy, dz likewise, d_ij = ((dx dx) + (dy dy)) + (dz dz).  The candidates
 * of a query are ordered by (d_ij, j); the first k are its result, in the caller's row order:
 *   dist2 : f32[N,k]  ascending;   idx : i64[N,k] the neighbours' rows, or NULL (not wanted)
 *   points: f32[N,3]  finite, |coordinate| <= 1e18 (a square that overflows is the caller's problem)
 *   order : i32[N]    a permutation of the rows that makes the points spatially coherent (a Morton order), or NULL: as
 *                     stored.  Blocks of MS_KNN_BLOCK consecutive points of that order are pruned by their bounding boxes, so
 *                     the order buys speed only: every permutation gives the same, exact result.  An entry outside [0, N) is
 *                     not dereferenced (the results are then wrong, nothing is accessed out of bounds).
 *   workspace : ms_knn_workspace_bytes(N, k) bytes, 16-byte aligned (16 N of sorted points, 32 per block of boxes; 0 for
 *               arguments ms_knn refuses)
 * k outside [1, MS_KNN_MAX_K], N <= k, a null pointer (points, dist2, workspace), a misaligned pointer (float and int32: 4
 * bytes, int64: 8, workspace: 16) -> MS_ERR_INVALID_ARG; N >= 2^31 -> MS_ERR_TOO_LARGE; all before any device work.
 * ------------------------------------------------------------------------------------- */
#define MS_KNN_BLOCK 64              /* points per bounding box = queries per wave */
#define MS_KNN_MAX_K 8
size_t ms_knn_workspace_bytes(int64_t N, int k);
int ms_knn(int64_t N, const float *points, const int32_t *order, int k, float *dist2, int64_t *idx, void *workspace,
           void *stream);

/* ---------------------------------------------------------------------------------------
 * Scene files: the row move between the five parameter tensors of a scene and the float32 rows of a 3DGS PLY body
 * (csrc/sceneio.hip; the file layout and the definition: mojosplat_amd/sceneio.py, pack_ply_rows_torch /
 * unpack_ply_rows_torch).  Replaces nothing in the reference (it reads and writes no scene); the CUDA stack's save_ply /
 * load_ply of 3DGS and gsplat's export_splats, which compose the rows from torch ops (permute, reshape, cat).
 * One launch on `stream` per call: no host synchronisation, no allocation, no workspace, no atomics.  The kernels move BITS:
 * no value passes through a float operation (NaN payloads and -0.0 survive).
 *
 *   tensors : HOST array of MS_PLY_TENSORS device pointers, tensor k f32[N, widths[k]] (the package's order: means3d, scales,
 *             quats, opacities, features as [N, 3 K])
 *   widths  : HOST array of their row widths in floats, each in [1, MS_PLY_MAX_COLUMNS], at most MS_PLY_MAX_COLUMNS together
 *   columns : HOST array of F table entries, F in [1, MS_PLY_MAX_COLUMNS].  An entry ties the file column `column` to float
 *             `offset` of the row of tensor `tensor`, or to no tensor (tensor = MS_PLY_NONE; offset is then ignored).
 *   rows    : pack   f32[N, F], out.  Entry by entry rows[n][column] = tensor[n][offset], +0.0 for an entry of no tensor;
 *                    every column of [0, F) must be named exactly once (every element of rows is written).
 *             unpack f32[N, S], in, S in [F, MS_PLY_MAX_STRIDE] the file's floats per row.  Entry by entry
 *                    tensor[n][offset] = rows[n][column], column in [0, S); an entry of no tensor is skipped, as is a column no
 *                    entry names; every float of every tensor's row must be named exactly once (every element of every
 *                    tensor is written).
 * A workgroup moves MS_PLY_ROWS consecutive rows through LDS; 16-byte accesses on every array whose base is 16-byte aligned,
 * dwords otherwise; every element index is 64-bit.  N = 0 is a no-op.  N < 0, a null or misaligned (4 bytes) pointer, F, S or a
 * width out of range, a table entry whose tensor, offset or column is out of range, a column (pack) or a tensor float
 * (unpack) named twice or (unpack) not at all -> MS_ERR_INVALID_ARG; more than (2^31 - 1) MS_PLY_ROWS rows ->
 * MS_ERR_TOO_LARGE; all before any device work.
 * ------------------------------------------------------------------------------------- */
#define MS_PLY_ROWS 64               /* rows per workgroup */
#define MS_PLY_TENSORS 5
#define MS_PLY_MAX_COLUMNS 128       /* table entries, and floats of the five tensors' rows together */
#define MS_PLY_MAX_STRIDE 192        /* floats per row of the rows ms_ply_unpack reads (64 rows of them are staged in LDS) */
#define MS_PLY_NONE (-1)
typedef struct ms_ply_column {
    int32_t tensor, offset, column;
} ms_ply_column;
int ms_ply_pack(int64_t N, int F, const float *const *tensors, const int32_t *widths, const ms_ply_column *columns, float *rows,
                void *stream);
int ms_ply_unpack(int64_t N, int F, int S, const float *rows, float *const *tensors, const int32_t *widths,
                  const ms_ply_column *columns, void *stream);

/* ---------------------------------------------------------------------------------------
 * Viewer formats: the bit packing of the PlayCanvas / SuperSplat compressed PLY and of the 32-byte .splat row
 * (csrc/splatio.hip; both formats and the definition: mojosplat_amd/splatio.py, backend="torch").  Replaces nothing in the
 * reference (it reads and writes no scene); the CUDA stack's gsplat export_splats(format="ply_compressed" | "splat"), which
 * runs on the host in numpy.  One launch on `stream` per call: no host synchronisation, no allocation, no workspace, no
 * atomics.  The kernels do only what is exact in IEEE float32 (compare, subtract, divide, multiply, add, floor, trunc,
 * sqrt, convert; no contraction, correctly rounded division and square root): the transcendental conversions are the
 * caller's, before ms_splat_compress / ms_splat32_pack and after the other two.  Non-finite inputs are not checked.
 *
 * The PREPARED arrays, rows in file order (C = ceil(N / MS_SPLAT_CHUNK) chunks; R = 3 (K - 1)):
 *   pos   f32[N,3]  the means                       rot   f32[N,4]  the unit quaternion wxyz
 *   lsc   f32[N,3]  log-scales clamped to [-20, 20] rgba  f32[N,4]  f_dc * SH_C0 + 0.5, then the linear opacity
 *   shr   f32[N,R]  the higher-order SH coefficients, channel-major as f_rest_* (K == 1: ignored, may be null)
 * and the file's elements:
 *   chunks   f32[C,18]  min xyz, max xyz, min scale, max scale, min rgb, max rgb over the chunk's rows
 *                       (ms_splat_decompress: f32[C, chunk_floats], chunk_floats 18, or 12 = no colour bounds: 0 and 1)
 *   vertices u32[N,4]   packed_position (11-10-11 bits), packed_rotation (2 + 3 x 10), packed_scale, packed_color (4 x 8)
 *   sh       u8[N,R]    a byte per higher-order coefficient (K == 1: ignored, may be null)
 * ms_splat_compress   reads the prepared arrays, writes every element of chunks, vertices and sh: a workgroup per chunk,
 *                     min / max by DPP steps over rows of 16 lanes and 16 x 18 LDS words.
 * ms_splat_decompress reads the file's elements, writes every element of the prepared arrays (rot: the dropped component
 *                     rebuilt as sqrt(max(0, 1 - a^2 - b^2 - c^2)); rgba's fourth: the opacity byte / 255).
 * ms_splat32_pack     rows u8[N,32] = pos | scale_lin f32[N,3] (exp of the log-scales) | trunc(255 rgba) | trunc(128 rot + 128),
 *                     bytes clamped to [0, 255]; ms_splat32_unpack is its inverse (byte / 255, (byte - 128) / 128).
 * rot, rgba, vertices and rows are accessed 16 bytes at a time and must be 16-byte aligned; every row index is 64-bit.
 * N = 0 is a no-op.  N < 0, a null or misaligned pointer, K outside [1, MS_SPLAT_MAX_K], chunk_floats neither 12 nor 18 ->
 * MS_ERR_INVALID_ARG; more than (2^31 - 1) MS_SPLAT_CHUNK rows -> MS_ERR_TOO_LARGE; all before any device work.
 * ------------------------------------------------------------------------------------- */
#define MS_SPLAT_CHUNK 256           /* Gaussians per chunk of a compressed PLY = rows per workgroup */
#define MS_SPLAT_MAX_K 25            /* SH coefficients per channel (degree 4) */
int ms_splat_compress(int64_t N, int K, const float *pos, const float *rot, const float *lsc, const float *rgba,
                      const float *shr, float *chunks, uint32_t *vertices, uint8_t *sh, void *stream);
int ms_splat_decompress(int64_t N, int K, int chunk_floats, const float *chunks, const uint32_t *vertices, const uint8_t *sh,
                        float *pos, float *rot, float *lsc, float *rgba, float *shr, void *stream);
int ms_splat32_pack(int64_t N, const float *pos, const float *scale_lin, const float *rgba, const float *rot, uint8_t *rows,
                    void *stream);
int ms_splat32_unpack(int64_t N, const uint8_t *rows, float *pos, float *scale_lin, float *rgba, float *rot, void *stream);

/* ---------------------------------------------------------------------------------------
 * Scene editing: a similarity transform x' = s R x + t of a whole scene -- means, log-scales, quaternions and the SH
 * coefficients, each band l >= 1 multiplied by the rotation's (2l+1) x (2l+1) real Wigner matrix in this library's SH basis
 * (csrc/transform.hip; the definition, and how the constants are derived: mojosplat_amd/edit.py, transform_scene with
 * backend="torch").  Replaces nothing in the reference (it edits no scene); SuperSplat's and splat-transform's scene
 * transforms, which run on the host.  One launch on `stream`: no host synchronisation, no allocation, no workspace, no atomics.
 * Every operation is a separately rounded float32 multiply or add in the definition's order (no contraction, nothing skipped
 * for a zero matrix entry): the outputs are the definition's bits.
 *
 *   xf : HOST, read before the call returns (it travels to the kernel by value).  All float32:
 *        A   s R, row-major          means'  = ((A[3i] x + A[3i+1] y) + A[3i+2] z) + t[i]
 *        t   the translation
 *        r   R as a unit quaternion wxyz   quats' = r (x) q (Hamilton product, not normalised); a - b c is evaluated as
 *                                          a + (-b) c, so only multiplies and adds occur
 *        l   ln s                    scales' = scales + l
 *        M1 .. M4  the band matrices, row-major: c'[l^2 + m] = sum_j M_l[m][j] c[l^2 + j], j ascending, per channel
 *   K  : SH coefficients per channel, one of 1, 4, 9, 16, 25; the bands above K's degree are not read.  K = 1 copies
 *        `features` ((N, 3) RGB features are passed as K = 1).
 *   means, scales f32[N,3], quats f32[N,4], features f32[N,K,3]: in; out_*: the same shapes, every element written.  No output
 *   may overlap an input.
 * A workgroup moves MS_TRANSFORM_ROWS feature rows through LDS (K = 1: MS_TRANSFORM_ROWS_K1 rows, no LDS): 16-byte accesses on
 * features / out_features and quats / out_quats where their base is 16-byte aligned, dwords otherwise; every row index is
 * 64-bit.  N = 0 is a no-op.  N < 0, a K outside the set, a null or misaligned (4 bytes) pointer, a null xf ->
 * MS_ERR_INVALID_ARG; more than (2^31 - 1) workgroups -> MS_ERR_TOO_LARGE; all before any device work.
 * ------------------------------------------------------------------------------------- */
#define MS_TRANSFORM_ROWS 64         /* Gaussians per workgroup, K > 1 */
#define MS_TRANSFORM_ROWS_K1 256     /* Gaussians per workgroup, K = 1 */
typedef struct ms_transform {
    float A[9], t[3], r[4], l;
    float M1[9], M2[25], M3[49], M4[81];
} ms_transform;
int ms_scene_transform(int64_t N, int K, const float *means, const float *scales, const float *quats, const float *features,
                       const ms_transform *xf, float *out_means, float *out_scales, float *out_quats, float *out_features,
                       void *stream);

/* ---------------------------------------------------------------------------------------
 * Bilateral-grid colour correction (csrc/bilagrid.hip; the definitions: mojosplat_amd/bilagrid.py, bilagrid_slice_torch and
 * bilagrid_tv_loss_torch).  Nothing in the reference; gsplat's use_bilateral_grid, and with L = Gh = Gw = 1 the per-image
 * 3x4 exposure matrix of 3DGS.
 *   grids  : f32[B,12,L,Gh,Gw] (gsplat's layout); coefficient c = 4 i + j is entry (i, j) of the 3x4 matrix, j = 3 the offset.
 *   img    : f32[B,H,W,3], channel innermost -- the tensor ms_render_fwd writes; image b goes through grid b.
 *   out    : f32[B,H,W,3], overwritten: out_i = sum_j A[4 i + j] rgb_j + A[4 i + 3], A interpolated trilinearly at
 *            u = (x + 0.5) / W (Gw - 1), v = (y + 0.5) / H (Gh - 1), z = ((0.299 r + 0.587 g) + 0.114 b) (L - 1) -- products and
 *            sums rounded separately; per axis of size n: vertex 0 if n == 1, else tc = clamp(t, 0, n - 1),
 *            i0 = min(floor(tc), n - 2), weights (1 - (tc - i0), tc - i0) on (i0, i0 + 1).
 *   v_out  : f32[B,H,W,3] = dL/dout.
 *   v_grids: f32[B,12,L,Gh,Gw] = dL/dgrids, EVERY element overwritten (exact zeros where no pixel reaches), or NULL.
 *   v_img  : f32[B,H,W,3] = dL/dimg, overwritten, or NULL: A^T v_out, plus -- where 0 < z < L - 1 only -- the term through
 *            the guidance, (L - 1) dA/df_z . (v_out x (rgb, 1)) times (0.299, 0.587, 0.114).  Nothing flows into u and v.
 *   workspace: ms_bilagrid_slice_workspace_bytes(B, H, W, L, Gh, Gw) bytes (0: bad sizes), needed with v_grids only: the
 *            partial sums [b][vertex][chunk of 32 pixel rows][level][12] of the vertex-centred gather.
 * One launch forward; backward one launch for v_img and two for v_grids; on `stream`, no host synchronisation, no
 * allocation, no float atomics: the same inputs give the same bits on every run.  Pixel offsets are 64-bit.
 *
 * ms_bilagrid_tv_*: gsplat's total_variation_loss -- per grid axis of size n >= 2 the sum of squared differences of
 * neighbours along it over their number in one batch entry (12 x the other two sizes x (n - 1)), the three added, over B; an
 * axis of size 1 contributes 0.
 *   workspace: ms_bilagrid_tv_workspace_bytes(B, L, Gh, Gw) bytes (0: bad sizes): per-workgroup partial sums.
 *   out1   : f32[1] (DEVICE), overwritten.     v_loss : f32[1] (DEVICE), read by the kernel.
 *   v_grids: f32[B,12,L,Gh,Gw] = v_loss * d tv / d grids, overwritten.
 * Two launches forward (partial sums, then one workgroup adding them in a fixed order in double), one backward; 16-byte
 * accesses along Gw where Gw is a multiple of 4 and the bases are 16-byte aligned, dwords otherwise.
 *
 * Sizes <= 0 or a null pointer (v_grids / v_img excepted; a workspace goes with v_grids) -> MS_ERR_INVALID_ARG; a short
 * workspace -> MS_ERR_WORKSPACE; grids of more than 2^31 - 1 elements, an image side above 2^23, more than 65535 tile rows
 * (16 pixels), images, or row chunks of a vertex -> MS_ERR_TOO_LARGE; all before any device work.
 * ------------------------------------------------------------------------------------- */
size_t ms_bilagrid_slice_workspace_bytes(int B, int H, int W, int L, int Gh, int Gw);
int ms_bilagrid_slice_fwd(int B, int H, int W, int L, int Gh, int Gw, const float *grids, const float *img, float *out,
                          void *stream);
int ms_bilagrid_slice_bwd(int B, int H, int W, int L, int Gh, int Gw, const float *grids, const float *img,
                          const float *v_out, void *workspace, size_t workspace_bytes, float *v_grids, float *v_img,
                          void *stream);
size_t ms_bilagrid_tv_workspace_bytes(int B, int L, int Gh, int Gw);
int ms_bilagrid_tv_fwd(int B, int L, int Gh, int Gw, const float *grids, void *workspace, size_t workspace_bytes,
                       float *out1, void *stream);
int ms_bilagrid_tv_bwd(int B, int L, int Gh, int Gw, const float *grids, const float *v_loss, float *v_grids, void *stream);

/* ---------------------------------------------------------------------------------------
 * Per-Gaussian contribution statistics of one view (csrc/contrib.hip; the definition: mojosplat_amd/contrib.py,
 * contributions_from_lists_torch).  Nothing in the reference; the scores that RadSplat (max blend weight over the training
 * rays) and LightGaussian (summed blend weight) prune by, and the sum that lifts an image mask to Gaussians.
 * Every pixel walks its tile's list front to back with ms_rasterize_to_pixels_3dgs_fwd's rules: sigma = 0.5 (a dx^2 + c dy^2)
 * + b dx dy at the pixel centre, alpha = min(0.999, o exp(-sigma)); an entry is skipped when sigma < 0 or alpha < 1/255; the
 * pixel stops BEFORE adding an entry when T (1 - alpha) <= 1e-4.  An entry that is added is blended, with w = alpha T_before.
 *   means2d f32[N,2], conics f32[N,3], opacities f32[N] (activated), tile_ranges i32[th,tw,2], flatten_ids i32[M]: the
 *            per-stage lists (ms_project_gaussians_fwd, ms_isect_tiles_*), tile_size 16 or 32, th = ceil(H / tile_size).
 *            A range is clamped to [0, M]; an id outside [0, N) blends nothing.
 *   weights: f32[H,W] or NULL; read clamped to [0, 1], NaN as 0.
 *   pixels : i64[N], += the number of pixels that blended the Gaussian.
 *   max_weight: f32[N], = max(itself, the largest w); updated as a 32-bit unsigned maximum on the bit pattern, so it must
 *            hold non-negative floats (zeros at first).
 *   sum_q  : i64[N], += sum w in units of 2^-30 (MS_CONTRIB_FIXED_ONE): the float32 partial sum of a (16x16 pixel block,
 *            Gaussian) -- a wave's 64 pixels in pixel order, the four waves in order -- is rounded to the nearest unit
 *            (ties to even) and added as an integer, so the result does not depend on the order of workgroups or calls.
 *   wsum_q : i64[N] or NULL with weights == NULL (then untouched), += the same sum with every term times its pixel's weight.
 * One launch on `stream`: a workgroup per 16x16 pixel block (a 32-pixel tile is walked by four), entries staged through LDS
 * 64 at a time (a wave walks only those that can reach its pixels: a conservative test, the result is that of walking all), the reduction over pixels through LDS in a fixed order; the only traffic between workgroups is integer
 * atomics (64-bit add, 32-bit unsigned max), none for a (block, Gaussian) that blended no pixel.  No workspace, no host
 * synchronisation, bitwise reproducible.  Bytes: 4 + 24 per list entry read (per block), up to four atomics per blended
 * (block, entry).  N == 0 or M == 0 returns at once, buffers untouched.
 * Sizes < 0, W or H <= 0, another tile_size, a null or misaligned pointer -> MS_ERR_INVALID_ARG; N or M above 2^31 - 1 or more
 * pixel blocks than a launch has workgroups -> MS_ERR_TOO_LARGE; all before any device work.
 * ------------------------------------------------------------------------------------- */
#define MS_CONTRIB_FIXED_ONE 1073741824 /* 2^30 */
int ms_contrib_accumulate(int64_t N, int64_t M, const float *means2d, const float *conics, const float *opacities,
                          const int32_t *tile_ranges, const int32_t *flatten_ids, const float *weights, int W, int H,
                          int tile_size, int64_t *pixels, float *max_weight, int64_t *sum_q, int64_t *wsum_q, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MOJOSPLAT_HIP_H */
