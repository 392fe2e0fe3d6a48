"""A multi-GPU rank's band frame through the library's two-call pair (ms_render_band_begin / ms_render_band_finish,
include/mojosplat_hip.h) -- the host side of distributed.py's HIP path since round 5.

Round 4's asynchronous band frame cost ~100-130 us of host time (Python marshalling of five tensors and a camera per frame,
four event operations, record_stream on every tensor that crosses to the lane, a frame object, the plan's bookkeeping) around
18-45 us of library enqueue -- level with the GPU time of a config-5 band at 8 ranks.  Here everything that does not change
from frame to frame is built ONCE and cached:

  * the scene (ms_scene: five device pointers, sizes, a prepared scene's block bounds) per set of tensors, keyed by their
    data pointers and version counters -- the tensors themselves are kept alive by the entry, so the caching allocator
    cannot recycle them under a lane's kernels and nothing needs record_stream;
  * the lane (ms_band_lane: scratch, pinned size record, stream, the two events that order the lane against the caller's
    stream) per (device, lane) -- the same scratch sets _fused.py's other lane users take;
  * the frame struct per lane, mutated in place (a lane runs one frame at a time).

A frame is then two ctypes calls; the caller -> lane -> caller stream ordering happens inside them (the output buffer is
allocated on the caller's stream, first touched on the lane after the lane has waited for the caller, and handed back
only after the caller's stream has waited for the lane: no record_stream for it either).

The reference has no counterpart (no distributed code: mojosplat/binning.py:83 is a dead comment).
"""
import ctypes
import math

import torch

from . import _fused, _hip
from .projection import EPS2D
from .utils import getenv

_scenes = {}    # key -> (Scene struct, tensors kept alive)
_SCENE_CAP = 16


def _tkey(t):
    # (round 6, advisor: a view such as means3d[:k] shares its base's data pointer AND version counter -- the extent is part
    # of what a cached ms_scene describes, so shape, strides and dtype are part of the key)
    return (t.data_ptr(), t._version, tuple(t.shape), t.stride(), t.dtype)


def _lane_fence(dev):
    """Make the caller's current stream wait for everything enqueued on the band lanes of `dev` so far: tensors the lanes may
    still be reading or writing are about to go back to the caching allocator, which only knows the caller's stream."""
    from ._fused import _lane_streams_if_any
    lanes = _lane_streams_if_any(dev)
    if not lanes:   # (no frame ever ran on a lane of this device: nothing to wait for -- and no CUDA call for CPU tensors)
        return
    cur = torch.cuda.current_stream(dev)
    for s in lanes:
        ev = torch.cuda.Event()
        ev.record(s)
        cur.wait_event(ev)


def clear_scenes():
    """Drop every cached ms_scene (release_scratch; the caller has synchronised the devices)."""
    global _last
    with _fused._frame_lock:
        _scenes.clear()
        _last = None


_last = None   # (the five tensor OBJECTS of the previous call, what _sig saw of them, the struct, its key): a render loop's fast path


def _sig(a, b, c, d, e):
    """What a cached ms_scene depends on, of the very same five tensor objects: where they point, their versions, extents,
    strides and types (_tkey's fields) -- ``t.data = other`` keeps the object AND its version counter and changes the rest
    (``t.data = t.data[:k]``: the extent alone; a transposed alias of the same memory: the strides alone).  One flat tuple
    of attribute reads: this runs on every band frame."""
    return (a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), e.data_ptr(),
            a._version, b._version, c._version, d._version, e._version,
            a.shape, b.shape, c.shape, d.shape, e.shape, a.stride(), b.stride(), c.stride(), d.stride(), e.stride(),
            a.dtype, b.dtype, c.dtype, d.dtype, e.dtype)


def scene_struct(means3d, scales, quats, opacities, colors):
    """-> the ms_scene ctypes struct for these tensors as they are now (cached)."""
    global _last
    with _fused._frame_lock:
        L = _last
        # the very same tensor objects, unmodified since (a view such as means3d[:k] is a NEW object each time: slow path) and
        # still on the same storage
        if (L is not None and L[0] is means3d and L[1] is scales and L[2] is quats and L[3] is opacities and L[4] is colors and
                L[5] == _sig(means3d, scales, quats, opacities, colors) and L[7] in _scenes):
            return L[6]
        S = _scene_struct(means3d, scales, quats, opacities, colors)
        _last = (means3d, scales, quats, opacities, colors, _sig(means3d, scales, quats, opacities, colors), S, S._key)
        return S


def _scene_struct(means3d, scales, quats, opacities, colors):
    key = _tkey(means3d) + _tkey(scales) + _tkey(quats) + _tkey(opacities) + _tkey(colors)
    hit = _scenes.get(key)
    if hit is not None:
        # (belt and braces: the struct's N is what band_begin sizes the workspace from)
        if hit[0].N != means3d.shape[0]:
            raise RuntimeError("cached ms_scene does not describe these tensors")
        hit[0]._key = key
        return hit[0]
    from .scene_order import prepared_bounds
    N = means3d.shape[0]
    m, sc, q = _hip.f32c(means3d), _hip.f32c(scales), _hip.f32c(quats)
    op = _hip.f32c(opacities.reshape(-1))
    if colors.dtype == torch.float16:
        cdt, col = 1, colors.contiguous()
    else:
        cdt, col = 0, _hip.f32c(colors)
    C = col.shape[1]
    assert m.shape == (N, 3) and sc.shape == (N, 3) and q.shape == (N, 4) and op.shape == (N,) and col.shape == (N, C)
    pb = prepared_bounds(means3d, scales) if (m is means3d and sc is scales) else None
    S = _hip.Scene(N, m.data_ptr() if N else None, sc.data_ptr() if N else None, 1, q.data_ptr() if N else None,
                   op.data_ptr() if N else None, col.data_ptr() if N else None, cdt, C,
                   pb[0].data_ptr() if pb else None, pb[1] if pb else 0, pb[0].shape[0] if pb else 0)
    # an earlier VERSION of these very tensors (updated in place since: an animated or a training scene) is stale for good --
    # and may hold marshalled copies (float64 / strided inputs): drop it instead of waiting for sixteen newer scenes
    evicted = [k_ for k_, v_ in _scenes.items() if v_[1][0] is means3d]
    if len(_scenes) - len(evicted) >= _SCENE_CAP:
        evicted.append(next(k_ for k_ in _scenes if k_ not in evicted))
    if evicted:
        # (round 6, advisor: an evicted entry may own marshalled copies that a begun band on a lane stream still reads; the
        # allocator re-issues them on the caller's stream, so that stream first waits for the lanes)
        _lane_fence(means3d.device)
        for k_old in evicted:
            _scenes.pop(k_old)
    # (the originals too: a marshalled copy's source must not change under the key's version check unnoticed)
    S._keep = (means3d, scales, quats, opacities, colors, m, sc, q, op, col, pb[0] if pb else None)
    S._key = key
    _scenes[key] = (S, S._keep)
    return S


class _LaneRec:
    """The cached ms_band_lane / ms_band_frame pair of one (device, lane slot)."""

    def __init__(self, dev, slot):
        self.dev, self.slot = dev, slot
        self.st = _fused._dev_state(dev, slot)
        self.ev_in, self.ev_out = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.device(dev):
            self.ev_in.record()
            self.ev_out.record()    # (materialises the hipEvent_t handles)
        st = self.st
        self.lane = _hip.BandLane(None, 0, None, 0, st["host"].data_ptr(), st["ev"].cuda_event, None, self.ev_in.cuda_event,
                                  self.ev_out.cuda_event)
        self.frame = _hip.BandFrame()
        self.status = (ctypes.c_int64 * 4)()
        self.ws_id = self.isect_id = None
        self.ws_key, self.ws_need = None, 0


_lane_recs = {}


def _lane_rec(dev, slot):
    # (lane slot 0 is per host thread in _fused -- its record lives with that thread's state)
    st = _fused._dev_state(dev, slot)
    rec = st.get("band_rec")
    if rec is None:
        rec = st["band_rec"] = _LaneRec(dev, slot)
    return rec


def _defer_enabled():
    return getenv(b"MOJOSPLAT_DEFER_CLEANUP", "1") != "0"


class BandHandle:
    __slots__ = ("rec", "shape", "level", "mode", "keep", "channels", "done")


def band_begin(means3d, scales, quats, opacities, colors, camera, bg, tile_size, band, out, out_y0, rows16, slot, lane_stream,
               caller_stream, stage_events=None):
    """Enqueue rows `band` of the frame on lane `slot` (its stream: the raw handle `lane_stream`; None = the caller's own
    stream, the blocking path).  `out`: the framebuffer (image row 0 at its start) or, with out_y0, a slab whose first row
    is image row out_y0.  -> a BandHandle for band_finish."""
    L = _hip.lib()
    dev = means3d.device
    S = scene_struct(means3d, scales, quats, opacities, colors)
    N, C = S.N, S.CDIM
    H, W = camera.H, camera.W
    th, tw = -(-H // tile_size), -(-W // tile_size)
    rec = _lane_rec(dev, slot)
    st = rec.st
    assert not st.get("busy"), "a begun frame still occupies this lane: finish it first"
    if rec.ws_key != (N, tw, th):
        rec.ws_key, rec.ws_need = (N, tw, th), L.ms_render_workspace_bytes(N, tw, th)
    ws = _fused._grow(st, "ws", rec.ws_need, dev)
    lane = rec.lane
    if rec.ws_id != ws.data_ptr():
        lane.workspace, lane.workspace_bytes = ws.data_ptr(), ws.numel()
        rec.ws_id = ws.data_ptr()
    isect = st["isect"]
    iid = None if isect is None else isect.data_ptr()
    if rec.isect_id != iid:
        lane.isect_buf, lane.isect_bytes = iid, 0 if isect is None else isect.numel()
        rec.isect_id = iid
    lane.sync_event = st["ev"].cuda_event if st.get("speculate", True) else None
    lane.stream = caller_stream if lane_stream is None else lane_stream
    r0, r1 = band
    flags = _fused.ROWS16 if (rows16 and tile_size != 16) else 0
    shape = (round(math.log2(N) * 8) if N > 0 else -1, tw, th, r0, r1)
    level = int(st.get("front_level", 0))
    mode = (_fused.FULL_SORT if st.get("full_sort") else _fused.FRONT_LEVEL * level) | flags
    vm = camera._viewmat_f32()
    if vm.device != dev:
        vm = vm.to(dev)
    bgc = None if bg is None else _hip.f32c(bg.reshape(-1))
    f = rec.frame
    f.scene = ctypes.pointer(S)
    f.viewmat = vm.data_ptr()
    f.fx, f.fy, f.cx, f.cy = camera.fx, camera.fy, camera.cx, camera.cy
    f.W, f.H = W, H
    f.eps2d, f.near_plane, f.far_plane = EPS2D, camera.near, camera.far
    # a band on a lane of its own (frames in flight behind each other): the clean-up launches wait for the rasteriser's verdict
    # (MS_RENDER_DEFER_CLEANUP; MOJOSPLAT_DEFER_CLEANUP=0: enqueued behind every band as on the blocking path)
    defer = _fused.DEFER_CLEANUP if (lane_stream is not None and _defer_enabled()) else 0
    f.tile_size, f.row_begin, f.row_end, f.flags = tile_size, r0, r1, mode | defer
    f.backgrounds = None if bgc is None else bgc.data_ptr()
    if out_y0 is not None:
        px = tile_size if not flags else 16
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape[1:]) == (W, C)
        assert out.shape[0] >= min(r1 * px, H) - min(r0 * px, H) and out_y0 == min(r0 * px, H)
        f.render_colors = out.data_ptr() - out_y0 * W * C * 4
    else:
        assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] >= H and tuple(out.shape[1:]) == (W, C)
        f.render_colors = out.data_ptr()
    evs = None
    if stage_events is not None:   # (bench.py's in-situ timing: 4 recorded-once torch events, entries may be None)
        evs = (ctypes.c_void_p * 4)(*[None if e is None else ctypes.c_void_p(e.cuda_event) for e in stage_events])
    f.stage_events = None if evs is None else ctypes.cast(evs, ctypes.c_void_p)
    with _hip.on_device(dev):
        _hip.check(L.ms_render_band_begin(ctypes.byref(f), ctypes.byref(lane), caller_stream), "ms_render_band_begin")
    st["busy"] = True
    h = BandHandle()
    h.rec, h.shape, h.level, h.mode, h.channels, h.done = rec, shape, level, mode, C, False
    # alive until the frame is finished (the scene's tensors and marshalled copies too: the cache may evict the entry)
    h.keep = (S, S._keep, vm, bgc, out, evs)
    return h


class _StatsFrame:   # (what _fused._count_frame wants to know of a frame)
    own = False

    def __init__(self, st):
        self.st = st


def band_finish(h, caller_stream):
    """Wait for the band's size record, redo the band exactly if its speculation did not hold, order the caller's stream
    behind the lane.  -> (Gaussians on the grid, pre-culled by the library, pairs in the band, the frame's flag word)."""
    L = _hip.lib()
    rec = h.rec
    st, lane, f = rec.st, rec.lane, rec.frame
    host = st["host_np"]
    grew = False
    try:
        with _hip.on_device(rec.dev):
            rc = L.ms_render_band_finish(ctypes.byref(f), ctypes.byref(lane), caller_stream, 0, rec.status)
            if rc == 2:   # MS_ERR_WORKSPACE: the intersection buffer is too small for this band's pairs
                need = int(host[5])
                grew = need > 0
                if need > 0:
                    # (round 6, advisor: ALWAYS resume against the state's current buffer -- the lane struct may have been
                    # built against an older, smaller one while st["isect"] is already large enough)
                    isect = st["isect"]
                    if isect is None or isect.numel() < need:
                        isect = _fused._grow(st, "isect", need, rec.dev, slack=1.25)
                    lane.isect_buf, lane.isect_bytes = isect.data_ptr(), isect.numel()
                    rec.isect_id = isect.data_ptr()
                    rc = L.ms_render_band_finish(ctypes.byref(f), ctypes.byref(lane), caller_stream, 1, rec.status)
            _hip.check(rc, "ms_render_band_finish")
    finally:
        st["busy"] = False
        h.done = True
    _fused._after_frame(st, host, rc, grew, shape=h.shape, level=h.level, mode=h.mode, own=False, channels=h.channels,
                        frame=_StatsFrame(st))
    s = rec.status
    return int(s[0]), bool(s[1]), int(s[2]), int(s[3])
