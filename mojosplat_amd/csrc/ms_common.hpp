// Shared host-side plumbing for libmojosplat_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mojosplat_hip.h"

namespace ms {

void set_error(const char *fmt, ...);

#define MS_REQUIRE(cond, code, ...)  \
    do {                             \
        if (!(cond)) {               \
            ms::set_error(__VA_ARGS__); \
            return (code);           \
        }                            \
    } while (0)

#define MS_HIP(expr)                                                                   \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) {                                                        \
            ms::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                          __LINE__);                                                   \
            return MS_ERR_HIP;                                                         \
        }                                                                              \
    } while (0)

// after a kernel launch: catches bad launch configurations without synchronising
#define MS_LAUNCH_CHECK() MS_HIP(hipGetLastError())

constexpr float kAlphaThreshold = 1.0f / 255.0f;
constexpr float kMaxAlpha = 0.999f;
constexpr float kTransmittanceStop = 1e-4f;
// The forward rasteriser's select without a compare (rasterize.hip is compiled with fp32 denormals flushed):
// kFlushK = 255 * 2^-126 is the smallest float k with fl(1/255) * k >= 2^-126, so alpha * k is a normal number
// iff alpha >= fl(1/255) and +0 otherwise.
constexpr float kFlushK = 0x1.fep-119f;
// alpha * kFlushK is never scaled back: the rasteriser carries the transmittance as S = T * kTScale, so that
// (alpha kFlushK) S = 255 alpha T, and divides by 255 (kInv255 = fl(1/255)) where it needs alpha T itself.
constexpr float kTScale = 0x1p+126f, kTUnscale = 0x1p-126f, kInv255 = kAlphaThreshold;
constexpr float kAlphaOfV = 0x1.010102p+118f;   // 2^126 / 255: alpha S from v = 255 alpha T
static_assert((double)kAlphaThreshold * (double)kFlushK >= 0x1p-126 &&
                  (double)(kAlphaThreshold * (1.0f - 0x1p-24f)) * (double)kFlushK < 0x1p-126,
              "flush select: the threshold must sit exactly on the smallest normal number");

// The rasteriser's staged record of one Gaussian (3 channels), as the fused frame's projection kernel
// writes it once per Gaussian and as the rasteriser's own staging computes it from the per-stage arrays:
//   a = (mean.x, mean.y, a', b')   a' = -log2(e)/2 * conic.a, b' = -log2(e) * conic.b
//   b = (c', log2(opacity), r, g)  c' = -log2(e)/2 * conic.c
//   c = (b, s, n_c, n_a)           s = log2(255 o) with slack (+inf: no bound, evaluate everywhere and take the
//                                  generic blend loop; -inf: opacity < 1/255, reaches nothing),
//                                  n_c = -conic.b / conic.c, n_a = -conic.b / conic.a
// log2(alpha)(d) = a' dx^2 + b' dx dy + c' dy^2 + log2(o); a quad can blend the Gaussian iff the minimum of
// -(a' dx^2 + b' dx dy + c' dy^2) over its pixel-centre rectangle is <= s.
struct RasterRecord {
    float4 a, b, c;
};
#ifdef __HIPCC__
__device__ __forceinline__ RasterRecord make_raster_record(float mx, float my, float ca, float cb, float cc,
                                                           float op, float r, float g, float b) {
    constexpr float kLog2e = 1.4426950408889634f;
    RasterRecord o;
    o.a = make_float4(mx, my, -0.5f * kLog2e * ca, -kLog2e * cb);
    o.b = make_float4(-0.5f * kLog2e * cc, __log2f(op), r, g);
    const float det = ca * cc - cb * cb;
    const bool bounded = det > 0.f && ca > 0.f && cc > 0.f && op <= kMaxAlpha;
    // (approximate reciprocals / log: their 1e-7 relative error is far inside the slack)
    // opacity below 1/255 can never blend: -inf, no quad is reached
    const float s = !(op >= kAlphaThreshold) ? -__builtin_huge_valf()
                    : bounded ? (__log2f(op * 255.0f) * 1.0001f + 1.5e-4f) : __builtin_huge_valf();
    o.c = make_float4(b, s, bounded ? -cb * __builtin_amdgcn_rcpf(cc) : 0.f, bounded ? -cb * __builtin_amdgcn_rcpf(ca) : 0.f);
    return o;
}
#endif

// What every entry point is handed, packed ONCE at the C ABI boundary (each extern "C" function fills them at its top, in
// the header's own argument order) and passed down by const reference: below that line no function takes a scalar scene or
// camera parameter, so two floats of a camera cannot change places on the way to a kernel.
struct Gaussians {
    int64_t N;
    const float *means3d, *scales;
    int scales_are_log;
    const float *quats, *opacities;
    const void *colors;   // (an entry point without colours: null, 0, 0)
    int color_dtype, CDIM;
};
struct View {
    const float *viewmat;
    float fx, fy, cx, cy;
    int W, H;
    float eps2d, near_plane, far_plane;   // (an entry point without planes: 0, 0 -- nothing downstream of one reads them)
};

// The frame's SIZE RECORD (ms_render_fwd's host_info: i64 words in pinned memory, written by the scans' total pass and --
// word 7, between the two halves of a frame -- by the library's host side).  The values are ABI: the header documents some,
// the Python layer tests others by value (the static_asserts below); only C++ uses the names.
enum InfoWord {
    kInfoPairs = 0,      // (Gaussian, tile) pairs in the band: M
    kInfoMaxCount = 1,   // the longest tile list (binning.hip, count_tail: sizes the exact path's sort classes)
    kInfoMedium = 2, kInfoLarge = 3, kInfoXL = 4,   // tiles in the medium / large / extra-large sort class
    kInfoNeed = 5,       // from the device: the PREVIOUS frame's redo counts; after MS_ERR_WORKSPACE: bytes of isect_buf needed
    kInfoOnGrid = 6,     // Gaussians whose box touches the grid (a pre-culled band: of its candidates)
    kInfoFlags = 7,
    kInfoVerdict = 8,    // a deferred clean-up: the rasteriser stores 1 here when a bin asks for the launches (LazyLists::verdict)
};
// word 7: the library's own between the two halves of a frame, and what the backward and the caller learn about the frame
constexpr int64_t
    kFrameSpeculated = 1,    // emit + rasterise were enqueued before the size record was known: the finishing half checks it
    kFrameLargeSorted = 2,   // ... with the large sort class among the launches (a frame that has such tiles needs it)
    kFrameExact = 4,         // redone on the exact path: the lists the caller reads back are laid out by M, not by capacity
    kFrameSplit = 8,         // 32-px bins cut into block lists: ids are not Gaussian indices, no backward can walk them
    kFrameNoSplit = 16,      // restarted without the split (4 M block-list slots overflowed int32): a resumed call must agree
    kFrameLightBet = 32,     // only the short sorts were launched, on the bet that no tile is heavy: holds iff heavy() == 0
    kFrameDepthCut = 64,     // pairs behind the bins' cut-offs were never written: the exact path cannot finish such a frame
    kFrameCutoffs = 128,     // the sort launch left cut-offs for the next frame on this record ...
    kFrameCutoffsBuf = 256,  // ... in this one of the workspace's two buffers (bit 8)
    kFrameFronts = 512,      // the rasteriser was given lazily sorted fronts: front counts and redo flags are this frame's
    kFrameLazy = 1024,       // a lazily sorted frame: no merge scratch between keys and ids in the exact layout
    kFrameBandCulled = 2048, // the band was pre-culled: word 6 counts its candidates, ids are positions in their list
    kFrameCleanupDeferred = 4096,   // the clean-up launches were left to the finishing half (word 8 says if they are needed)
    kFrameQuadLists = 8192,  // a differentiable frame's per-quad lists sit behind the ids (4 bytes per pair and quad of a tile)
    kFrameClaimed = 16384,   // the histogram rows are per-XCD claims: every emit of the frame must read them that way
    kFrameRowsZeroed = 32768,   // the rasteriser zeroed the backward's rows of raw sums in the workspace: no memset is owed
    // bits 16-31: the grid the cut-offs belong to (the record may have served another since); bits 32-47: the band's
    // signature (a rank's share keeps cut-offs for its own rows and clip only)
    kFrameCutSigMask = 0xffffffffll << 16,
    // bit 48: the frame's sort launch rode in its rasteriser (rasterize.hip, k_sort_rasterize): one workgroup per 32-px bin sorted
    // the bin's list and rasterised its four blocks.  Nothing downstream reads the lists differently -- the bit exists so that a
    // test or a measurement can tell that a frame really took that path (_fused.FRAME_STATS: fused_sort)
    kFrameFusedSort = 1ll << 48,
    // bit 49 (only beside bit 48): this frame's bins finish their own short fronts -- a workgroup of the fused kernel whose
    // sorted front ran out with pixels alive fetched the rest of its list itself; no clean-up launch was enqueued
    // (_fused.FRAME_STATS: cleanup_in_kernel)
    kFrameCleanupInKernel = 1ll << 49;
constexpr int kFrameCutGridShift = 16, kFrameBandSigShift = 32, kFrameCutoffsBufShift = 8;
static_assert(kInfoPairs == 0 && kInfoXL == 4 && kInfoNeed == 5 && kInfoOnGrid == 6 && kInfoFlags == 7 && kInfoVerdict == 8,
              "size record: the header and the Python layer index these words by number");
static_assert(kFrameSpeculated == 1 && kFrameExact == 4 && kFrameSplit == 8 && kFrameLightBet == 32 && kFrameDepthCut == 64 &&
                  kFrameFronts == 512 && kFrameBandCulled == 2048 && kFrameCleanupDeferred == 4096 && kFrameQuadLists == 8192 &&
                  kFrameRowsZeroed == 32768,
              "flag word: mojosplat_hip.h documents bits 2, 13 and 15, mojosplat_amd/*.py tests the others by value");
static_assert(kFrameFusedSort == 281474976710656ll && (kFrameFusedSort & (kFrameCutSigMask | 0xffffll)) == 0,
              "flag word: bit 48 lies above the cut-offs' signature; _fused.py counts fused_sort frames by this value");
static_assert(kFrameCleanupInKernel == 562949953421312ll && (kFrameCleanupInKernel & (kFrameFusedSort | kFrameCutSigMask | 0xffffll)) == 0,
              "flag word: bit 49, next to the fused sort's; _fused.py counts cleanup_in_kernel frames by this value");
static_assert(((kFrameDepthCut | kFrameCutoffs | kFrameCutoffsBuf | kFrameCutSigMask) & 0x3f) == 0,
              "flag word: _fused.py withdraws the record's word for the cut-offs by keeping bits 0-5 alone");
// word 5 as the device leaves it: bins the previous frame's clean-up redid because their sorted front was too short ...
static inline int64_t front_redos(const int64_t *info) { return info[kInfoNeed] & 0xffffffffll; }
// ... and because their depth cut-off was stale (bits 32-61; bit 62: the regeneration disagreed with the count kernel)
static inline int64_t cut_redos(const int64_t *info) { return (info[kInfoNeed] >> 32) & 0x3fffffffll; }
static inline int64_t heavy(const int64_t *info) { return info[kInfoMedium] + info[kInfoLarge] + info[kInfoXL]; }

// HOW a frame is binned and sorted.  The C ABI's `tight` and `lazy` words end at the entry points: each decodes its masked
// word once (decode_tight / decode_lazy, the only places that know a bit's value) and nothing below takes an int of flags.
// ms_render_fwd fills the structs field by field -- the fields behind the first comment line of each are its alone.
struct BinMode {
    bool reach_masks, band_only, block_masks;   // bits 0-2 of `tight` (mojosplat_hip.h, ms_project_isect_count)
    bool odd_cols, odd_rows;   // bits 3-4: the half-tile grid of a block-mask frame has 2 tile_w - 1 columns / 2 tile_h - 1 rows
    bool band_cull;            // bit 5: the band is a rank's share of a frame -- its Gaussians are pre-culled (k_band_precull)
    // ms_render_fwd only:
    bool lean;          // the frame keeps LeanRecs instead of the projected arrays (the caller vouches that nobody reads those)
    bool keep_arrays;   // ... and writes the projected arrays too (a frame that hands out last_ids)
    bool defer_total;   // sync-free frames: the scans' total pass rides in the scatter launch
    bool claimed;       // the count pass claims its rows (k_project_hist's tile_total); every emit of the frame must carry it too
    int cut_in;         // a depth-cut frame: which of the two cut-off buffers it reads
};
struct SortMode {
    bool on;            // `lazy` != 0: lazily sorted fronts
    int front_level;    // bits 1-2: fronts 2^level times as deep
    bool light_bet;     // bit 3, speculative emit: the caller expects no tile beyond the small sort class
    // ms_render_fwd only: the merged sort launch leaves the NEXT frame's cut-offs (a depth-cut frame reads its own from the other buffer)
    bool write_cutoffs;
    int cut_out;        // ... in this one of the two buffers
};
constexpr BinMode decode_tight(int tight) {
    return BinMode{(tight & 1) != 0, (tight & 2) != 0, (tight & 4) != 0, (tight & 8) != 0, (tight & 16) != 0, (tight & 32) != 0,
                   false, false, false, false, 0};
}
constexpr SortMode decode_lazy(int lazy) { return SortMode{(lazy & 15) != 0, (lazy >> 1) & 3, (lazy & 8) != 0, false, 0}; }
static_assert(decode_tight(1).reach_masks && decode_tight(2).band_only && decode_tight(4).block_masks && decode_tight(8).odd_cols &&
                  decode_tight(16).odd_rows && decode_tight(32).band_cull && !decode_tight(~1).reach_masks && !decode_tight(~32).band_cull,
              "tight: the bits mojosplat_hip.h documents, one field each");
static_assert(!decode_lazy(0).on && decode_lazy(1).on && decode_lazy(1).front_level == 0 && decode_lazy(2).front_level == 1 &&
                  decode_lazy(6).front_level == 3 && !decode_lazy(7).light_bet && decode_lazy(8).light_bet && decode_lazy(8).on,
              "lazy: mojosplat_hip.h documents != 0, bits 1-2 (front level) and bit 3 (light bet)");
static_assert(!decode_tight(~0).lean && !decode_tight(~0).keep_arrays && !decode_tight(~0).defer_total && !decode_tight(~0).claimed &&
                  decode_tight(~0).cut_in == 0 && !decode_lazy(~0).write_cutoffs && decode_lazy(~0).cut_out == 0,
              "no bit of a caller's word reaches what only ms_render_fwd may ask for");

// WHERE: a band of tile rows of one binning grid, and the isect workspace (ms_isect_workspace_bytes(N, tw, th)) that serves it.
// ms_render_fwd builds one per frame (one more for the 32-px bin grid of a split frame, in the same workspace).
struct Band {
    int64_t N;   // the scene the workspace is carved up for
    int tile_size, tw, th, row_begin, row_end;
    void *ws;
    size_t ws_bytes;
};
// ... and how the count / scatter kernels walk the scene for it (binning.hip, make_schedule): G workgroups of `chunk` Gaussians
struct Schedule {
    int G;
    int64_t chunk;
    int64_t near_cap;   // depth-cut frames: the stride of a count workgroup's compacted records (>= what any workgroup walks, band candidates included)
    int T_local;        // the band's tiles
    size_t lds_bytes;   // their counters (+ the on-grid counter of the count kernels)
};

// binning.hip: ms_project_isect_count that also writes the rasteriser's records (raster_records: N x 48 B, or null;
// they take g.colors: the frame's colours, 3 channels, f32 or f16)
int project_isect_count(const Gaussians &g, const View &v, float radius_clip, const Band &band, BinMode mode, float *means2d,
                        float *conics, float *depths, int32_t *radii, int32_t *tile_ranges, int64_t *isect_info,
                        int64_t *isect_info_mirror, void *raster_records, void *stream, uint32_t cut_stamp = 0,
                        // a PREPARED scene (ms_scene_prepare): bounds of every block of block_size Gaussians, for the band pre-cull
                        const float *block_bounds = nullptr, int block_size = 0,
                        Schedule *launched = nullptr);   // out: the count launch's schedule (CutInputs::count)

// Lazy sorting (binning.hip): tiles longer than front_threshold have only front_count[tile] sorted
// entries; the rasteriser appends a tile to redo_list when pixels are still alive at the end of it.
// what a depth-cut frame's clean-up launches need to bring a dropped Gaussian's record back (host-side: far_regen)
struct CutInputs {
    Gaussians g;   // (by value: a deferred clean-up keeps the whole struct beyond the enqueuing call -- rasterize.hip, CleanupMemo)
    View v;
    void *records;
    // the frame's band and -- pre-culled (band_cull) -- the schedule of its count launch, which left the band's candidate
    // list in the workspace (project_isect_count: `launched`)
    Band band;
    Schedule count;
    int band_cull;
};
struct LazyLists {
    const int32_t *front_count;
    int32_t *redo_flag, *redo_list, *redo_count;
    int front_threshold;
    const uint64_t *keys;   // the scatter's unsorted (depth_bits << 32 | id) keys, for the clean-up pass
    // split frames (rasterize_fwd_split): the lists above belong to 32-px bins; the rasteriser walks
    // per-block lists cut from them and flags the BIN (bin_more: its list was longer than its front)
    const int32_t *bin_more;
    int bin_w;
    int packed;             // key / list words are id << 4 | block bits
    int row_lo, row_hi;     // split frames: the band in 16-px block rows (the clean-up leaves other rows alone)
    int redo_grid;          // workgroups of the clean-up launch (256: an empty launch costs the frame the same whatever their number)
    int redo_sort;          // != 0: the clean-up takes two launches (rasterize.hip, k_redo_sort): stranded bins sorted whole, then a workgroup per block
    // depth-cut frame (cut_stamp != 0): the tiles marked has_far[tile] == cut_stamp own pairs that were never written
    // (depth bits > tau[tile]); the clean-up launches regenerate them for the tiles on the redo list from the frame's
    // 12-byte box records (`lean`, n_lean of them) into the free tail of the key array behind the cut_words[0] entries
    // of the lists, one segment per tile: far_cnt[tile] keys from far_start[tile] on (far_cur: the scatter's cursors).
    uint32_t cut_stamp;
    const uint32_t *tau;    // this frame's cut-offs (isect_lazy_arrays: buffer 0 of the two, T words each)
    uint32_t *tau_next;     // the next frame's, as the sort launch left them: the clean-up launch resets the tiles it redoes
    const uint32_t *has_far;
    const void *lean;
    int64_t n_lean;
    int64_t *cut_words;     // the device record's words 8.. : near pairs, far pairs, log cursor
    uint64_t *log_keys;     // == keys, writable
    uint32_t *far_cnt, *far_cur, *far_start;
    const CutInputs *cut_inputs;   // (a HOST pointer, read when the clean-up launches are enqueued)
    // DEFERRED clean-up (a band frame in flight behind another: ms_render_band_begin / _finish, pipeline.hip): non-null = a
    // device-visible address of a word of the lane's pinned record.  The rasteriser stores 1 there when it puts a bin on the
    // redo list, its launch is NOT followed by the clean-up launches, and the finishing half -- which has waited for the
    // rasteriser -- enqueues them only if the word is set (rasterize_deferred_cleanup).
    int32_t *verdict;
};
// lazily sorted fronts: depth (entries) of a front, LDS room for it, depth buckets from the camera planes
struct FrontParams {
    uint32_t fixed_min;
    int fixed_shift, front_k, front_cap;
};
// The sort of a frame whose rasteriser does it itself (rasterize.hip, k_sort_rasterize): what the merged sort launch
// (binning.hip, k_tile_front<false, true>) would have been handed.  isect_emit_speculative fills it and launches the scatter
// alone (taken = 1) when it would have launched the merged sort on 32-px bins at the default front depth; rasterize_fwd
// then launches the fused kernel in place of its own.
// What the workgroup at position p of the heaviest-first order needs to begin: its bin and the bin's list, in ONE load.  The
// pass that builds the order writes it (binning.hip, deferred_total) beside order[] and tile_ranges[], which stay as they are.
struct alignas(16) OrderRec {
    int32_t tile, start, n, pad;
};
struct FusedSort {
    int taken;              // out: the sort launch was left to the rasteriser
    FrontParams fp;
    const uint32_t *wg_depth;   // the scatter's per-workgroup depth ranges, n_wg pairs (8-byte aligned)
    int n_wg;
    // in: n_order OrderRecs of the caller's own scratch (null: the frame is not fused); the scatter launch of a fused frame
    // fills all of them, every frame
    OrderRec *order_recs;
    int n_order;            // the band's bins, heaviest first: one workgroup each
    uint32_t *tau_out;      // the next frame's cut-offs (or null), this frame's, the marks of its cut bins and their stamp
    const uint32_t *tau_now, *has_far;
    uint32_t cut_stamp;
    int64_t cap;            // entries the key / id buffers hold (a bin beyond it: speculative overflow, left unsorted)
    const uint64_t *keys;
    int32_t *flatten_ids, *front_count;
    int finish_short;       // (set by the frame's caller behind `taken`) a bin whose front is shorter than its list walks on by
                            // itself and rasterize_fwd enqueues no clean-up launch: never on a depth-cut frame (cut_stamp != 0)
};
// rasterize.hip: the clean-up launches a frame enqueued with lazy.verdict set left out, on `stream`; `key` = that pointer
int rasterize_deferred_cleanup(const void *key, void *stream);
int far_regen(const LazyLists &lazy, int tw, int n_tiles, int64_t cap, void *stream);
// project_bwd.hip: ms_project_gaussians_bwd_pose behind its checks of the pose output (v_viewmat, or null, as below)
int project_bwd(const Gaussians &g, const View &v, const int32_t *radii, const float *v_means2d, const float *v_conics,
                const float *v_depths, float *v_means3d, float *v_scales, float *v_quats, float *v_viewmat, void *pose_scratch,
                void *stream);
// project_bwd.hip: the backward projection straight from the backward rasteriser's packed gradient rows
int project_bwd_from_rows(const Gaussians &g, const View &v, const int32_t *radii, const float *rows, float *v_means3d,
                          float *v_scales, float *v_quats, float *v_colors, float *v_opacities, void *stream,
                          bool raw_rows = false,    // rasterize_bwdq.hip's raw sums, finished with g.opacities (radii may be null)
                          // non-null: dL/dviewmat f32[16] (overwritten, bottom row 0) through ms_pose_scratch_bytes(N) of scratch
                          float *v_viewmat = nullptr, void *pose_scratch = nullptr);
// project_bwd.hip: the checks of a pose-gradient entry point's output and scratch (ms_pose_scratch_bytes)
int check_pose_out(int64_t N, const float *out, const void *scratch, size_t scratch_bytes, const char *who);
LazyLists isect_lazy_arrays(const Band &band);
bool depth_cut_fits(const Band &band);
FrontParams front_params(int tile_size, const SortMode &sort, float depth_near, float depth_far, bool merged, bool split);
const int32_t *isect_order_array(const Band &band);

// rasterize.hip: ms_rasterize_to_pixels_3dgs_fwd with a separate density hint (ms_render_fwd's
// sync-free frames pass the buffer capacity as M and the previous frame's M as the hint).
// records: N ready-made RasterRecords (3 channels) or null; order: the band's tiles of the BINNING grid,
// heaviest list first (isect_order_array; for a split frame these are its 32-px bins), or null;
// clip_row16_begin / _end: only the 16x16 blocks of these 16-px rows are rasterised (-1: all of the band's tiles)
int rasterize_fwd(int64_t N, int64_t M, int64_t density_hint, const float *means2d, const float *conics,
                  const void *colors, int color_dtype, int CDIM, const float *opacities, const float *backgrounds,
                  int W, int H, int tile_size, int tile_row_begin, int tile_row_end, const int32_t *tile_ranges,
                  const int32_t *flatten_ids, float *render_colors, float *render_alphas, int32_t *last_ids,
                  const LazyLists *lazy, const void *records, const int32_t *order, int clip_row16_begin,
                  int clip_row16_end, void *after_raster_event, void *stream,
                  // a differentiable frame: every 8x8 quad leaves the Gaussians that passed its reach test, in list order, for the
                  // backward rasteriser -- quad_lists i32[M * quads per tile], quad_counts i32[tiles * quads per tile] (or null)
                  int32_t *quad_lists = nullptr, int32_t *quad_counts = nullptr,
                  // round 6: zero_bytes of memory every wave of the launch zeroes a slice of on its way (a differentiable frame's
                  // rows of raw gradient sums: the kernel is issue-bound and moves 70 MB in 90 us -- the 64 N bytes ride along
                  // instead of costing the backward a 10-us memset); null: nothing
                  void *zero_mem = nullptr, size_t zero_bytes = 0,
                  // non-null (taken != 0): the frame's sort launch was left to this call -- the fused kernel, k_sort_rasterize
                  const FusedSort *fused = nullptr);
// rasterize.hip: would rasterize_fwd take the frame's sort (the plain 3-channel kernel on ready-made records over a whole grid
// of 32-px bins, two waves a block by its own rule -- or, `force`, whatever the rule says: tests on small images)?
bool rasterize_takes_sort(int64_t density_hint, int CDIM, int W, int H, int tile_size, int tile_row_begin, int tile_row_end,
                          const void *records, const int32_t *order, bool force);

// rasterize_bwd.hip: ms_rasterize_to_pixels_3dgs_bwd with the forward frame's ready-made records (or null) and its
// heaviest-first order of the image's tiles (16-px tiles only; or null: the kernel's own counting sort)
int rasterize_bwd(int64_t N, int64_t M, const float *means2d, const float *conics, const float *colors, int CDIM,
                  const float *opacities, const float *backgrounds, int W, int H, int tile_size,
                  const int32_t *tile_ranges, const int32_t *flatten_ids, const float *render_alphas,
                  const int32_t *last_ids, const float *v_render_colors, const float *v_render_alphas, float *v_means2d,
                  float *v_conics, float *v_colors, float *v_opacities, void *workspace, size_t workspace_bytes,
                  int overwrite, const void *records, const int32_t *block_order, void *stream);

// rasterize_bwdq.hip: the backward rasteriser of a 3-channel differentiable frame -- one wave per 8x8 quad walking the
// frame's own lists front to back (fully sorted, or lazily sorted fronts: front_count / front_threshold as the forward
// took them), per-entry sums on the matrix pipe, raw sums into 64-byte rows (zeroed by the caller; finished by
// project_bwd_from_rows with raw_rows_opacities).  ids: Gaussian index per entry, id_stride ints apart; skip_flag: tiles
// to leave alone (or null); order: the binning grid's tiles heaviest first (or null).
int rasterize_bwd_quads(int64_t N, int64_t M, const void *records, const float *backgrounds, int W, int H, int tile_size,
                        const int32_t *tile_ranges, const int32_t *ids, int id_stride, const int32_t *front_count,
                        int front_threshold, const int32_t *skip_flag, const float *render_colors,
                        const float *render_alphas, const float *v_render_colors, const float *v_render_alphas,
                        float *packed_rows, const int32_t *order, void *stream,
                        int tile_row_begin = 0, int tile_row_end = -1,
                        const int32_t *quad_lists = nullptr, const int32_t *quad_counts = nullptr);   // (a band of tile rows; -1: to the last row | the forward's per-quad lists: rasterize_fwd)

// ... and its launch for the tiles the forward's clean-up pass redid (their sorted front ran out with pixels alive): a wave
// per (tile, block, quad) walks the whole-tile sorted ids the forward's k_redo_sort left (redo_flag[tile] == 2); a tile that
// was not sorted that way gets its keys sorted in place by one workgroup first.  Empty on almost every frame.
int rasterize_bwd_redo(int64_t N, int64_t M, const void *records, const float *backgrounds, int W, int H, int tile_size,
                       const int32_t *tile_ranges, uint64_t *keys, const int32_t *ids, const int32_t *redo_list,
                       const int32_t *redo_count, const int32_t *redo_flag, const float *render_colors,
                       const float *render_alphas, const float *v_render_colors, const float *v_render_alphas,
                       float *packed_rows, void *stream, int32_t *count_mirror = nullptr);

// Block lists of a split frame (ms_render_fwd): what the sort kernels of 32-px bins write instead of
// flatten_ids.  Bin `b` with list [start, start + n) owns block_ids[4 start, 4 (start + n)): its block q
// (2x2 per bin, q = 2 dy + dx) gets [4 start + q n, ... + count_q), and block_ranges holds that pair for
// every 16x16 block of the image; bin_more[b] = the list was longer than its sorted front.
struct BlockLists {
    int32_t *block_ranges, *block_ids, *bin_more;
    int tw16, th16;
};
// Sync-free frames (ms_render_fwd): the scans' total pass -- tile_ranges, work lists, launch order, the size record --
// rides in the scatter launch instead of being a serial pass of its own (binning.hip, deferred_total), and the
// caller's hand-off event is recorded right behind that launch.
struct DeferredTotal {
    int band_only;
    int64_t *info, *info_mirror;
    void *sync_event;
    uint32_t cut_stamp;   // != 0: a depth-cut frame; the value its tiles with dropped pairs are marked with (unique per frame)
};
// DEPTH CUT (sync-free lean frames on plain bins; binning.hip, k_project_hist): pairs behind their tile's cut-off
// are counted but never written; a tile that outlives its list gets them back from the clean-up launch.
// (project_isect_count: cut_stamp; the emit and the rasteriser: DeferredTotal::cut_stamp / LazyLists::cut_stamp)
// binning.hip: what ms_isect_tiles_emit_speculative / ms_isect_tiles_emit forward to, and ms_render_fwd with its own modes
int isect_emit_speculative(const Band &band, const float *means2d, const int32_t *radii, const float *depths, const int32_t *tile_ranges, const int64_t *isect_info_dev,
                           int64_t capacity, const int64_t *prev_info_host, const BinMode &bin, const SortMode &sort,
                           float depth_near, float depth_far, uint64_t *sort_keys, int32_t *flatten_ids,
                           const DeferredTotal *defer, void *stream,
                           // non-null: the caller's rasteriser can sort the bins itself (FusedSort: filled, taken = 1 if left to it)
                           FusedSort *fuse = nullptr);
int isect_emit_exact(const Band &band, const float *means2d, const int32_t *radii, const float *depths, const int32_t *tile_ranges, const int64_t *host_info,
                     const BinMode &bin, const SortMode &sort, float depth_near, float depth_far, uint64_t *sort_keys,
                     uint64_t *sort_tmp, int32_t *flatten_ids, void *stream,
                     int64_t *isect_ids = nullptr);   // (the C entry point's: gsplat's 64-bit ids, fully sorted lists only)

// binning.hip: scatter + sorts on the bin grid, writing block lists (info_dev != null: sync-free frame
// against `cap` entries, host_info = the previous frame's record or null)
int isect_emit_bins(const Band &bins, const float *means2d, const int32_t *radii, const float *depths, const int32_t *bin_ranges, const int64_t *host_info,
                    const int64_t *info_dev, int64_t cap, const BinMode &bin, const SortMode &sort, float depth_near,
                    float depth_far, uint64_t *sort_keys, const BlockLists *out, const DeferredTotal *defer, void *stream);

// Split frame: the block lists cut from 32-px bins are rasterised per 16x16 block and cleaned up per
// bin.  Rows are BLOCK rows.
int rasterize_fwd_split(int64_t N, int64_t cap, int64_t density_hint, const float *means2d, const float *conics,
                        const void *colors, int color_dtype, int CDIM, const float *opacities,
                        const float *backgrounds, int W, int H, int block_row_begin, int block_row_end,
                        const int32_t *bin_ranges, const BlockLists *lists, float *render_colors,
                        const LazyLists *lazy, const void *records, const int32_t *order, void *after_raster_event,
                        void *stream);

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace ms
