"""Multi-GPU rendering of ONE frame: image tile-row bands over the ranks of a node, one RCCL
all-gather of the framebuffer over xGMI (BASELINE config 5).

The reference has no distributed path at all (no torch.distributed / NCCL call site anywhere),
so this is new design, MI355X-first:
  * every rank holds the full Gaussian set and projects it redundantly -- 76 B/Gaussian of HBM
    streaming is cheaper than moving 32 B/Gaussian of projected data across xGMI;
  * rank r bins, sorts and rasterises only tile rows [r*rows, (r+1)*rows) (one ms_render_fwd
    call with a row band): its pixels are one contiguous slab of the HWC framebuffer, so the
    exchange is a single equal-sized all_gather_into_tensor whose input slab aliases its slot of
    the output (in-place form, no staging copy).  Slabs are padded to `rows` tile rows; rows
    below H are never read;
  * the "no intersections anywhere -> zeros image" rule of the reference (render.py:73-76)
    needs a frame-level fact.  A HIP band frame pre-culls the Gaussians that cannot reach its band
    (csrc/binning.hip, k_band_precull) and reports how many of the REST touch the full grid, so the
    fact is the OR over the ranks: one 4-byte all-reduce(MAX) enqueued beside the framebuffer gather;
    only a rank whose own band holds nothing waits for its result.  (Injected CPU stages count over
    all Gaussians and need no exchange.)
  * frames are independent, so the gather of frame k can overlap the render of frame k+1:
    `async_op=True` hands back a PendingFrame right after the all-gather is enqueued on RCCL's
    stream; the caller's stream only waits for it in `.wait()`.

  * LOAD BALANCE (round 3).  Equal bands are not equal work: a centre-heavy scene gives the middle ranks twice the
    pairs of the edge ranks (config 5 cut 8 ways: 157-323 us per band).  Every frame's 16-byte status record (the
    on-grid flag and the band's pair count, all-gathered beside the framebuffer in place of round 2's 4-byte
    all-reduce) lets all ranks recompute the SAME band boundaries from the same numbers every few frames: cost of a
    band = half its share of the pairs + half its share of the rows, boundaries moved 70 % of the way to the equal-
    cost cut, until the spread is under 8 %.  Bands are then ragged, and the exchange is either the padded in-place
    all-gather plus one compaction copy, or (MOJOSPLAT_GATHER=direct) grouped point-to-point sends / receives
    straight into the image's rows -- xGMI is point to point, every GPU has a link to every other, and ragged
    bands need no padding there.  MOJOSPLAT_BALANCE=0 keeps equal bands.

One process per GPU; backend "nccl" is RCCL on ROCm.  `stages` makes the orchestration testable
on CPU with gloo (tests inject CPU stage functions); without it the HIP library renders the band.
"""
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import torch
import torch.distributed as dist

from .utils import Camera, getenv as _getenv


def band_plan(tile_rows: int, world: int) -> Tuple[int, list]:
    """rows per rank (equal, padded) and the [r0, r1) tile-row band of every rank."""
    rows = -(-tile_rows // world)
    bands = [(min(r * rows, tile_rows), min((r + 1) * rows, tile_rows)) for r in range(world)]
    return rows, bands


def rebalance(bounds, pairs, damping: float = 0.7, min_rows: int = 1):
    """New band boundaries (tile rows, len world + 1) from the weights the ranks reported for the current ones (the
    Gaussians that reach a pre-culled band, or a band's pairs).
    Cost of a band = 0.5 * its share of the weights + 0.5 * its share of the rows (the binning side of a band frame
    follows the Gaussians / pairs, the rasteriser of a dense scene the pixels); weights are taken as uniform inside a band.  The
    boundaries move `damping` of the way to the equal-cost cut.  Pure integer / float arithmetic on numbers every
    rank holds identically -> every rank gets the same answer.  -> (bounds, spread = max cost / mean cost BEFORE)."""
    world = len(bounds) - 1
    th = bounds[-1]
    total = float(sum(pairs))
    rows = [bounds[r + 1] - bounds[r] for r in range(world)]
    if total <= 0 or th <= 0:
        return list(bounds), 1.0
    cost = [0.5 * pairs[r] / total + 0.5 * rows[r] / th for r in range(world)]
    spread = max(cost) * world          # (the costs sum to 1: mean = 1 / world)
    # cumulative cost at every row boundary, piecewise linear inside a band
    dens = [(cost[r] / rows[r]) if rows[r] > 0 else 0.0 for r in range(world)]
    new = [0]
    r, acc = 0, 0.0                      # acc = cumulative cost at the start of band r
    for k in range(1, world):
        want = k / world
        while r < world - 1 and acc + cost[r] < want:
            acc += cost[r]
            r += 1
        inside = (want - acc) / dens[r] if dens[r] > 0 else 0.0
        target = bounds[r] + inside
        b = bounds[k] + damping * (target - bounds[k])
        new.append(int(round(b)))
    new.append(th)
    # monotone, every band at least min_rows (as far as the image allows)
    for k in range(1, world):
        new[k] = max(new[k], new[k - 1] + min_rows)
    for k in range(world - 1, 0, -1):
        new[k] = min(new[k], new[k + 1] - min_rows)
    for k in range(1, world):
        new[k] = min(max(new[k], 0), th)
        new[k] = max(new[k], new[k - 1])
    return new, spread


def _gather_mode():
    v = _getenv(b"MOJOSPLAT_GATHER", "allgather")
    if v not in ("allgather", "ring", "direct"):
        raise ValueError("MOJOSPLAT_GATHER must be 'allgather' or 'direct'")
    return "direct" if v == "direct" else "allgather"


def _balance_enabled():
    return _getenv(b"MOJOSPLAT_BALANCE", "1") != "0"


def _force_exchange():
    """MOJOSPLAT_FORCE_EXCHANGE=1: a group of ONE rank still runs the exchange step -- the status all-gather and the
    in-place all_gather_into_tensor of the framebuffer onto itself.  For the world-1 RCCL test (tests/test_hip_rccl.py):
    one GPU is all a test box has, RCCL refuses two ranks per device, and this way its collectives, their stream
    semantics and the in-place aliasing run on hardware."""
    return _getenv(b"MOJOSPLAT_FORCE_EXCHANGE", "0") == "1"


def balance_weights(records):
    """The weights `rebalance` runs on, from the ranks' gathered status records (on_grid, Gaussians that reach the band if the
    LIBRARY pre-culled it else -1, pairs in the band, stamp): ONE unit for all ranks -- Gaussians only if every band was
    pre-culled, else pairs (round 3 let each rank pick its unit from a local guess: ragged bands could make one rank
    report Gaussians and another pairs, and the plan oscillated).  -> (weights, by_gaussians)."""
    by_gaussians = all(int(r[1]) >= 0 for r in records)
    return [int(r[1] if by_gaussians else r[2]) for r in records], by_gaussians


_plans = {}   # plan key -> dict(bounds, frame): the bands of the next frame of that scene, identical on every rank
_CHECK_EVERY, _CHECK_SETTLED, _SPREAD_OK = 8, 64, 1.08


def _plan_key(means3d, camera, tile_size, world, group=None):
    """(round 4: the GROUP is part of the key -- a rank that sits in two groups of one size keeps a plan and a frame
    counter per group, so that the ranks of either group count the same frames)"""
    import math
    n = means3d.shape[0]
    return (means3d.device, round(math.log2(n) * 8) if n > 0 else -1, camera.W, camera.H, tile_size, world,
            None if group is None else id(group))


def _bounds_hash(bounds):
    h = 1469598103934665603
    for b in bounds:
        h = ((h ^ int(b)) * 1099511628211) & 0x7fffffff
    return h


def band_bounds(means3d, camera, tile_size, world, group=None):
    """The band boundaries (tile rows) the next sharded frame of this scene uses -- equal bands until the ranks'
    pair counts say otherwise."""
    th = -(-camera.H // tile_size)
    p = _plans.get(_plan_key(means3d, camera, tile_size, world, group))
    if p is not None:
        return list(p["bounds"])
    rows, bands = band_plan(th, world)
    return [b[0] for b in bands] + [th]


@dataclass
class Stages:
    """Per-stage callables (CPU tests inject these).
    project(means3d, scales, quats, opacities, camera) -> means2d, conics, depths, radii
    bin(means2d, radii, depths, tile_size, tw, th, row_range) -> ids, tile_ranges
    raster(means2d, conics, colors, opacities, bg, ranges, ids, camera, tile_size, row_range, out)"""
    project: Callable
    bin: Callable
    raster: Callable


def _on_grid_count(means2d, radii, tile_size, tw, th) -> int:
    """Gaussians whose gsplat tile box (floor/ceil, exclusive max, clamped) is non-empty on the
    full grid -- the torch restatement of isect_info[6] for the injected-stage path."""
    r = radii.to(torch.float32) / tile_size
    t = means2d.to(torch.float32) / tile_size
    x0 = torch.floor(t[:, 0] - r[:, 0]).clamp(0, tw)
    x1 = torch.ceil(t[:, 0] + r[:, 0]).clamp(0, tw)
    y0 = torch.floor(t[:, 1] - r[:, 1]).clamp(0, th)
    y1 = torch.ceil(t[:, 1] + r[:, 1]).clamp(0, th)
    ok = (radii[:, 0] > 0) & (radii[:, 1] > 0) & (x1 > x0) & (y1 > y0)
    return int(ok.sum())


def _band_of(band, th):
    # an empty band (more ranks than tile rows) still runs the count pass: its verdict on the
    # frame must match the other ranks'
    return (min(band[0], th), min(max(band[1], band[0]), th))


# Bin size of a rank's band frames (16 = the library's default for 16-px tiles, 32 / 64 = plain coarse bins under a
# band that keeps its 16-px rows, MS_RENDER_ROWS16): the same rule as render_gaussians (render.bin_rule) applied to
# the band's own size record -- pairs on its bin rows, its (pre-culled) Gaussians on the grid -- one frame behind.
# The pixels do not depend on it (tests/test_hip_fused.py); ranks need not agree.
def _band_key(means3d, camera, band, tile_size):
    import math
    n = means3d.shape[0]
    return ("band", means3d.device, round(math.log2(n) * 8) if n > 0 else -1, camera.W, camera.H, tuple(band), tile_size)


def _band_bin(means3d, camera, band, tile_size):
    """-> (key, bin px) for this band's next frame."""
    from . import render as R
    if tile_size != 16:
        return None, tile_size
    forced = R._env_bin_px()
    if forced is not None:
        return None, forced
    key = _band_key(means3d, camera, band, tile_size)
    with R._bin_lock:
        return key, R._bin_mode.get(key, 16)


_learnt = {}   # band key -> the last size record the rule was applied to (a static scene repeats it frame after frame)


def _band_learn(key, mode, m, info, camera, band):
    if key is None:
        return
    from . import render as R
    rec = (mode, m, info["on_grid"], info["flags"])
    with R._bin_lock:
        if _learnt.get(key) == rec:
            return       # same record as the previous frame: the rule's answer stands
        if len(_learnt) > 256:
            _learnt.clear()
        _learnt[key] = rec
    # (a frame at mode 16 is a split frame -- 32-px bins, flag bit 3 -- unless the band is too thin for that)
    grid = (32 if info["flags"] & 8 else 16) if mode == 16 else mode
    band_px = max(16, (band[1] - band[0]) * 16)
    nxt = R.bin_rule(mode, m, info["on_grid"], camera.W, band_px, band=True, grid_px=grid)
    if nxt == 64 and band_px < 256:
        # a band under four rows of 64-px bins: the coarse grid's saving in pairs does not make up for the bin rows
        # that stick out of the band (config 3 cut 8 ways, 144-px bands: 98 / 102 / 113 us at 16 / 32 / 64 px on the
        # edge bands whose large near-camera footprints the rule sends to 64)
        nxt = 32
    R._settle(key, mode, nxt)


def _render_band(stages, means3d, scales, quats, opacities, features, camera, bg, tile_size, band, out, out_y0=None):
    """Render tile rows `band` into `out` (the full framebuffer, or -- out_y0 given -- a slab whose first row is image
    row out_y0); -> (Gaussians touching the full grid (0 = empty frame), pairs in the band, whether the library
    pre-culled the band -- the first number then counts the Gaussians that reach THIS band)."""
    r0, r1 = band
    H, W = camera.H, camera.W
    th, tw = -(-H // tile_size), -(-W // tile_size)
    if stages is None:
        from . import _band, _hip
        b = _band_of(band, th)
        key, mode = _band_bin(means3d, camera, b, tile_size)
        # (rows16: the band stays in 16-px rows while the BINS follow the rule -- only when the caller's tiles are the
        # 16-px ones; an explicit tile_size of 32 / 48 / 64 keeps band_plan's units, tile rows of that size)
        # (round 5: the library's band pair on the CALLER's stream -- lane slot 0, the calling thread's own scratch)
        cur = _hip._raw_stream(means3d.device.index) if _hip._raw_stream is not None else torch.cuda.current_stream(means3d.device).cuda_stream
        h = _band.band_begin(means3d, scales, quats, opacities, features, camera, bg, mode, b, out, out_y0, tile_size == 16, 0, None, cur)
        on_grid, culled, m, flags = _band.band_finish(h, cur)
        _band_learn(key, mode, m, {"on_grid": on_grid, "flags": flags}, camera, b)
        return on_grid, m, culled
    means2d, conics, depths, radii = stages.project(means3d, scales, quats, opacities, camera)
    ids, ranges = stages.bin(means2d, radii, depths, tile_size, tw, th, band)
    if r1 > r0:
        stages.raster(means2d, conics, features, opacities, bg, ranges, ids, camera, tile_size, band, out)
    return _on_grid_count(means2d, radii, tile_size, tw, th), int(ids.numel()), False


class PendingFrame:
    """A sharded frame in flight.  `.wait()` completes it on the host side (size-record check,
    framebuffer all-gather enqueued on the collective's stream) and makes the CURRENT stream wait
    for the gather; -> the full (H, W, C) image."""

    def __init__(self, image=None, finalize=None, on_drop=None):
        self._image, self._finalize, self._on_drop = image, finalize, on_drop

    def wait(self) -> torch.Tensor:
        if self._finalize is not None:
            fin, self._finalize = self._finalize, None
            self._image = fin()
        return self._image

    def __del__(self):
        # dropped without wait(): release what the frame holds (its lane)
        if getattr(self, "_finalize", None) is not None and getattr(self, "_on_drop", None) is not None:
            try:
                self._on_drop()
            except Exception:   # noqa: BLE001  (interpreter shutdown)
                pass


_turn = {}  # device -> which of the two lanes the next asynchronous frame takes
_events = {}  # (device, lane) -> (event the lane waits for before a band, event the caller waits for after it)


_streams = {}  # (device index, raw handle) -> torch Stream object of that handle


def _current_stream(dev):
    """torch.cuda.current_stream(dev) without its ~5 us of Python per call: the raw handle of the current stream
    is one C call, and the Stream object for a handle never changes."""
    from . import _hip
    if _hip._raw_stream is None:
        return torch.cuda.current_stream(dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    raw = _hip._raw_stream(idx)
    st = _streams.get((idx, raw))
    if st is None:
        st = torch.cuda.current_stream(dev)
        _streams[(idx, raw)] = st
    return st


def _lane_events(dev, lane):
    e = _events.get((dev, lane))
    if e is None:
        e = (torch.cuda.Event(), torch.cuda.Event())
        _events[(dev, lane)] = e
    return e


@torch.no_grad()
def render_gaussians_sharded(means3d, scales, quats, opacities, features, camera: Camera,
                             background_color: Optional[torch.Tensor] = None, tile_size: int = 16,
                             group=None, stages: Optional[Stages] = None, async_op: bool = False,
                             rehearse: Optional[Tuple[int, int]] = None, bounds: Optional[list] = None,
                             exchange_dtype: Optional[torch.dtype] = None):
    """Every rank returns the full (H, W, C) image.  Inputs must be identical on all ranks.
    exchange_dtype: None -- the bands travel as they are rendered, float32, and the image is the single-GPU frame bit for bit --
    or torch.float16 / torch.bfloat16: every rank rounds ITS band to that type (one cast of 1 / world of the frame) before
    the exchange and every rank returns the image IN that type.  Half the bytes over xGMI: the exchange is what bounds the
    8-GPU frame rate of a large frame (config 5: 87 MB per GPU in float32, at least 81 us over 7 x 153 GB/s against a
    ~118 us band), and a frame that goes to a display or an 8-bit encoder loses nothing to float16.
    rehearse=(rank, world) acts as that rank WITHOUT a process group and without the exchange
    (only its own slab of the image is rendered): single-GPU timing of one rank's share.
    bounds: the world + 1 band boundaries in tile rows (rehearsals, tests); default: the scene's current plan --
    equal bands, then what `rebalance` makes of the ranks' pair counts.

    async_op=True returns a PendingFrame (call .wait() for the image) and is meant to be used one
    frame ahead: `nxt = render(..., async_op=True); img = cur.wait(); cur = nxt`.  The band is
    enqueued on one of two lane streams without any host wait; .wait() then checks the frame and
    starts its gather, which overlaps the band render of the frame begun before it.  At most two
    frames may be pending."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    if rehearse is not None:
        rank, world = rehearse
    dev = means3d.device
    C = features.shape[-1]
    H, W = camera.H, camera.W
    th = -(-H // tile_size)
    # the background takes the colours' dtype first, as in render_gaussians (reference render.py:55): with
    # fp16 colours 0.1 is 0.09998 on every path
    if background_color is None:
        bg = torch.zeros(C, device=dev, dtype=torch.float32)
    elif isinstance(background_color, torch.Tensor):
        from .render import _background_as
        bg = _background_as(background_color, dev, features.dtype, True)   # (kept per tensor: no conversion kernels per frame)
    else:
        bg = torch.as_tensor(background_color, device=dev).to(features.dtype).to(torch.float32)
    if bg.shape[0] != C:
        raise ValueError(f"Background color channels ({bg.shape[0]}) must match gaussian color channels ({C})")
    if exchange_dtype not in (None, torch.float32, torch.float16, torch.bfloat16):
        raise ValueError("exchange_dtype must be None, torch.float32, torch.float16 or torch.bfloat16")
    xdt = torch.float32 if exchange_dtype is None else exchange_dtype
    x16 = xdt != torch.float32

    # ---- this frame's bands: equal until the ranks' pair counts say otherwise (rebalance, module docstring)
    live = (world > 1 or (_force_exchange() and dist.is_initialized())) and rehearse is None   # a real process group: status records are exchanged
    pkey = _plan_key(means3d, camera, tile_size, world, group)
    if bounds is None:
        bounds = band_bounds(means3d, camera, tile_size, world, group)
    assert len(bounds) == world + 1 and bounds[0] == 0 and bounds[-1] == th and all(a <= b for a, b in zip(bounds, bounds[1:]))
    bands = [(bounds[r], bounds[r + 1]) for r in range(world)]
    rows_max = max(b - a for a, b in bands)
    equal = all(a == min(r * rows_max, th) and b == min((r + 1) * rows_max, th) for r, (a, b) in enumerate(bands))
    mode = _gather_mode()
    slab = rows_max * tile_size
    y0s = [min(a * tile_size, H) for a, _ in bands]
    y1s = [min(b * tile_size, H) for _, b in bands]
    # Framebuffer: equal bands render straight into their slot of the padded image (in-place all-gather, as round
    # 2); "direct" renders into the image and exchanges rows point to point; ragged bands under the all-gather go
    # through a (world, slab) buffer, each rank's band at the start of its slot, and ONE compaction copy.
    padded = live and mode == "allgather" and not equal
    H_pad = max(world * slab, H) if (equal or not live) else H

    # A HIP band frame reports how many of ITS Gaussians touch the full grid: the library pre-culls what cannot
    # reach the band (csrc/binning.hip, k_band_precull), so the frame-level "nothing on the grid -> zeros image"
    # rule (render.py:73-76) needs the OR over the ranks.  Every frame of a live group therefore all-gathers a
    # 16-byte status record per rank -- (Gaussians on the grid, pairs in the band) -- beside the framebuffer; every
    # rank always takes part in both collectives.  (Injected CPU stages count the on-grid Gaussians over ALL of
    # them, but exchange the record all the same: the pair counts steer the band boundaries.)
    def exchange(buf, on_grid, m_band, culled=False):
        """-> (image or a callable that yields it, [works]): the exchange step, or the frame-level zeros rule."""
        if not live:
            if rehearse is not None and stages is None and world > 1:
                # a rehearsed rank of the HIP path: its on-grid count is the count AFTER the band pre-cull, so an
                # empty band of a non-empty frame also reports 0 -- the frame-level zeros rule cannot be decided
                # locally; the band (background where nothing reaches it) is what this rank contributes
                return buf[:H], []
            if on_grid == 0:
                return torch.zeros(H, W, C, device=dev, dtype=xdt), []   # zeros, not background (render.py:73-76)
            return buf[:H], []
        # The status record, 32 bytes per rank: Gaussians on the grid (the zeros-image rule's OR); the Gaussians that reach
        # the band if the LIBRARY pre-culled it (it says so in the size record's flag word: bit 11), else -1; the band's
        # pairs; and this rank's frame counter of the plan with a hash of the bounds it rendered with.  Round 3 sent one
        # weight whose unit each rank chose from a Python copy of the library's pre-cull test: ragged bands could make one
        # rank report Gaussians and another pairs, and the plan oscillated.  Now the unit is chosen from what ALL ranks
        # report (Gaussians only if every band was pre-culled).  The plans and their counters are kept per GROUP (a rank in
        # two groups of one size counted both groups' frames on one counter and re-planned on other frames than its
        # peers); the stamps are compared on the frames that re-plan and a mismatch raises instead of drifting on.
        plan = _plans.setdefault(pkey, dict(bounds=list(bounds), frame=0))
        plan["frame"] += 1
        stamp = (plan["frame"] << 32) | _bounds_hash(bounds)
        status = torch.tensor([on_grid, on_grid if culled else -1, m_band, stamp], dtype=torch.int64, device=dev)
        status_all = torch.empty((world, 4), dtype=torch.int64, device=dev)
        works = [dist.all_gather_into_tensor(status_all.view(-1), status, group=group, async_op=True)]
        if mode == "direct":
            ops = []
            for peer in range(world):
                if peer == rank:
                    continue
                if y1s[rank] > y0s[rank]:
                    ops.append(dist.P2POp(dist.isend, buf[y0s[rank]:y1s[rank]], peer, group))
                if y1s[peer] > y0s[peer]:
                    ops.append(dist.P2POp(dist.irecv, buf[y0s[peer]:y1s[peer]], peer, group))
            if ops:
                works += dist.batch_isend_irecv(ops)
        elif padded:
            works.append(dist.all_gather_into_tensor(buf.view(-1), buf[rank].reshape(-1), group=group, async_op=True))
        else:
            works.append(dist.all_gather_into_tensor(buf[:world * slab], buf[rank * slab:(rank + 1) * slab],
                                                     group=group, async_op=True))
        check = _balance_enabled() and plan["bounds"] == list(bounds) and \
            plan["frame"] % (_CHECK_SETTLED if plan.get("settled") else _CHECK_EVERY) == 0

        def image():
            # the OR over the ranks is at least this rank's own bit: only a rank whose band holds nothing has to READ
            # the records (a device-to-host read, i.e. a host stall), and every rank on the frames that re-plan
            frame = torch.cat([buf[r, :y1s[r] - y0s[r]] for r in range(world)]) if padded else buf[:H]
            if on_grid > 0 and not check:
                return frame
            rec = status_all.cpu()
            if check:
                stamps = [int(v) for v in rec[:, 3]]
                if any(v != stamps[0] for v in stamps):
                    # (cannot happen while every rank of the group makes the same sequence of sharded calls -- the plans
                    # and their frame counters are kept per group -- so this is a caller's bug, and silence would end in
                    # collectives of different sizes)
                    raise RuntimeError(f"render_gaussians_sharded: the ranks of this group lost step (frame counter / "
                                       f"band bounds stamps {stamps}); every rank must make the same sharded calls")
                # identical numbers on every rank -> identical new bounds on every rank, from the next frame on
                weights, _ = balance_weights(rec.tolist())
                nb, spread = rebalance(list(bounds), weights)
                plan["settled"] = spread <= _SPREAD_OK
                if not plan["settled"]:
                    plan["bounds"] = nb
            if int(rec[:, 0].max()) == 0:
                return torch.zeros(H, W, C, device=dev, dtype=xdt)
            return frame
        return image, works

    def resolve(img, works):
        for w_ in works:
            w_.wait()
        return img() if callable(img) else img

    def framebuffer():
        # fresh per frame (caching allocator: no hipMalloc), handed out as a view; in the exchange's type
        if padded:
            return torch.empty((world, slab, W, C), dtype=xdt, device=dev)
        return torch.empty((H_pad, W, C), dtype=xdt, device=dev)

    n_own = y1s[rank] - y0s[rank]

    def own_slot(buf):
        return buf[rank, :n_own] if padded else buf[y0s[rank]:y1s[rank]]

    if stages is not None or not async_op:
        buf = framebuffer()
        if stages is not None and (padded or x16):
            tmp = torch.empty((H, W, C), dtype=torch.float32, device=dev)     # (CPU test stages address the full image)
            on_grid, m_band, culled = _render_band(stages, means3d, scales, quats, opacities, features, camera, bg, tile_size,
                                                   bands[rank], tmp)
            own_slot(buf).copy_(tmp[y0s[rank]:y1s[rank]])
        elif x16:
            # a 16-bit exchange: the band in float32 into a slab of its own, ONE rounding pass into its slot of the framebuffer
            own = torch.empty((max(n_own, 1), W, C), dtype=torch.float32, device=dev)
            on_grid, m_band, culled = _render_band(stages, means3d, scales, quats, opacities, features, camera, bg, tile_size,
                                                   bands[rank], own, y0s[rank])
            own_slot(buf).copy_(own[:n_own])
        else:
            on_grid, m_band, culled = _render_band(stages, means3d, scales, quats, opacities, features, camera, bg, tile_size,
                                                   bands[rank], buf[rank] if padded else buf, y0s[rank] if padded else None)
        img, works = exchange(buf, on_grid, m_band, culled)
        if not async_op:
            return resolve(img, works)
        return PendingFrame(finalize=lambda: resolve(img, works))

    # asynchronous HIP path: the band on a lane stream, begun without any host wait (ms_render_band_begin); torch's current
    # stream is never switched.  Round 5: the library's two-call pair does the marshalling-free enqueue and the stream ordering
    # around the lane (_band.py: scene / lane / frame structs cached, no record_stream -- the scene's tensors are kept alive
    # by the cache, the framebuffer is first touched on the lane after the lane has waited for the caller's stream and
    # handed out after the caller's stream has waited for the lane).
    from . import _band, _hip
    from ._fused import _frame_lock, _lane_streams
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    raw = _hip._raw_stream(idx) if _hip._raw_stream is not None else torch.cuda.current_stream(dev).cuda_stream
    lanes = _lane_streams(dev)
    buf = framebuffer()
    own = torch.empty((max(n_own, 1), W, C), dtype=torch.float32, device=dev) if x16 else None   # (see the blocking path)
    my_band = _band_of(bands[rank], th)
    bkey, bmode = _band_bin(means3d, camera, my_band, tile_size)
    with _frame_lock:   # (the shared lanes are one thread at a time: the lane pick and the frame's claim on it)
        lane = _turn.get(dev, 0)
        _turn[dev] = 1 - lane
        from . import render as _render   # bench.py's in-situ kernel timing hook (None otherwise)
        h = _band.band_begin(means3d, scales, quats, opacities, features, camera, bg, bmode, my_band,
                             own if x16 else (buf[rank] if padded else buf),
                             y0s[rank] if (padded or x16) else None, tile_size == 16, 1 + lane, lanes[lane].cuda_stream, raw,
                             _render._STAGE_HOOK() if _render._STAGE_HOOK is not None else None)

    def finalize():
        now = _hip._raw_stream(idx) if _hip._raw_stream is not None else torch.cuda.current_stream(dev).cuda_stream
        on_grid, culled, m, flags = _band.band_finish(h, now)   # size-record check (+ exact redo on the lane); lane -> `now`
        _band_learn(bkey, bmode, m, {"on_grid": on_grid, "flags": flags}, camera, my_band)
        if x16:
            own_slot(buf).copy_(own[:n_own])                    # (on `now`, which band_finish has ordered behind the lane)
        img, works = exchange(buf, on_grid, m, culled)          # the collectives' stream waits for `now`
        return resolve(img, works)                              # ... and `now` for the exchange
    def on_drop(st=h.rec.st, lane_stream=lanes[lane]):
        # (round 6, advisor) dropped without wait(): the lane's kernels may still be writing the framebuffer / slab, which the
        # closure above is about to hand back to the caching allocator -- an allocator that only knows the caller's stream.
        # record_stream defers their re-issue until the lane has passed this point.  (The scene's tensors and marshalled
        # copies stay alive through the handle and the scene cache, whose eviction fences the lanes itself: _band.py.)
        for t in (buf, own):
            if t is not None:
                t.record_stream(lane_stream)
        st["busy"] = False
    return PendingFrame(finalize=finalize, on_drop=on_drop)


@torch.no_grad()
def render_gaussians_batch_sharded(means3d, scales, quats, opacities, features, cameras,
                                   background_color: Optional[torch.Tensor] = None, tile_size: int = 16, group=None,
                                   async_op: bool = False, exchange_dtype: Optional[torch.dtype] = None):
    """Multi-view rendering sharded by VIEW instead of by tile row -- the second sharding axis SURVEY.md section 8(f)
    row 4 names: the same Gaussians from C cameras, every rank returns all C views, (C, H, W, channels) f32.

    Rank r renders the contiguous run of views [r * per, (r + 1) * per), per = ceil(C / world), with the multi-view
    entry point (render_gaussians_batch: one library call, two views in flight) straight into its slab of a
    (world * per, H, W, channels) buffer, and ONE in-place all_gather_into_tensor over RCCL completes it on every
    rank.  Whole frames shard without any per-frame fixed cost growing with the rank count, which is what bounds the
    tile-row bands of a small frame: the price is that the views must be known together, and the
    exchange moves the same bytes per view as the band gather does.  The zeros-image rule is per view and local
    (every rank renders whole frames).  Inputs must be identical on all ranks.
    async_op=True returns a PendingFrame right after the gather is enqueued on the collective's stream: `.wait()`
    makes the current stream wait for it and hands out the views, so the next call's rendering overlaps this call's
    exchange (use it one call ahead, as with render_gaussians_sharded).
    exchange_dtype: as render_gaussians_sharded's -- torch.float16 / torch.bfloat16 halve the bytes of the exchange; the views
    are then returned in that type (a world of one included, so that a caller sees one type whatever the group)."""
    from .render import render_gaussians_batch
    if exchange_dtype not in (None, torch.float32, torch.float16, torch.bfloat16):
        raise ValueError("exchange_dtype must be None, torch.float32, torch.float16 or torch.bfloat16")
    xdt = torch.float32 if exchange_dtype is None else exchange_dtype
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    cams = list(cameras)
    C = len(cams)
    dev = means3d.device
    ch = features.shape[-1]
    if C == 0:
        return torch.empty((0, 0, 0, ch), dtype=torch.float32, device=dev)
    H, W = cams[0].H, cams[0].W
    if world == 1 and not (_force_exchange() and dist.is_initialized()):
        out = render_gaussians_batch(means3d, scales, quats, opacities, features, cams,
                                     background_color=background_color, tile_size=tile_size)
        out = out if xdt == torch.float32 else out.to(xdt)
        return PendingFrame(image=out) if async_op else out
    per = -(-C // world)
    full = torch.empty((world * per, H, W, ch), dtype=xdt, device=dev)
    mine = cams[rank * per:(rank + 1) * per]
    if mine and xdt == torch.float32:
        render_gaussians_batch(means3d, scales, quats, opacities, features, mine, background_color=background_color,
                               tile_size=tile_size, out=full[rank * per:rank * per + len(mine)])
    elif mine:
        part = render_gaussians_batch(means3d, scales, quats, opacities, features, mine, background_color=background_color,
                                      tile_size=tile_size)
        full[rank * per:rank * per + len(mine)].copy_(part)   # (the one rounding pass, over this rank's views)
    # in place, as the band gather
    work = dist.all_gather_into_tensor(full, full[rank * per:(rank + 1) * per], group=group, async_op=True)

    def done():
        work.wait()
        return full[:C]
    return PendingFrame(finalize=done) if async_op else done()


# ---- sharded TRAINING step ("per-Gaussian grads need one all-reduce") -----------------------------
class _ReduceGrad(torch.autograd.Function):
    """Identity forward; the gradient is summed over the ranks on its way back (injected-stage path: each rank's autograd
    yields the gradient of ITS band's pixels only)."""

    @staticmethod
    def forward(ctx, x, group):
        ctx.group = group
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        dist.all_reduce(g, op=dist.ReduceOp.SUM, group=ctx.group)
        return g, None


class _GatherBands(torch.autograd.Function):
    """Forward: this rank's band rows [y0, y1) of `full_like` come from `band_img`, the others' from an all-gather of the
    padded slabs; backward: the band's rows of dL/dimage (every rank computes the same loss on the same full image)."""

    @staticmethod
    def forward(ctx, band_img, H, slab, rank, world, group):
        W, C = band_img.shape[1], band_img.shape[2]
        buf = torch.zeros((world * slab, W, C), dtype=band_img.dtype, device=band_img.device)
        y0 = min(rank * slab, H)
        y1 = min(y0 + slab, H)
        buf[y0:y1] = band_img[y0:y1]
        dist.all_gather_into_tensor(buf.view(-1), buf[rank * slab:(rank + 1) * slab].reshape(-1).clone(), group=group)
        ctx.rows = (y0, y1, band_img.shape[0])
        return buf[:H].clone()

    @staticmethod
    def backward(ctx, v):
        y0, y1, Hb = ctx.rows
        g = torch.zeros((Hb,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
        g[y0:y1] = v[y0:y1]
        return g, None, None, None, None, None


class _RenderBandHip(torch.autograd.Function):
    """A rank's differentiable band frame on the HIP path: ms_render_fwd with render_alphas over the band's tile rows (own
    scratch, lazily sorted fronts, the inference frame's binning), the framebuffer all-gather; backward: the band's
    backward rasteriser into the packed per-Gaussian rows (ms_render_bwd_rows), ONE all_reduce of the rows over the
    ranks, the backward projection on the summed rows (ms_render_bwd_finish) -- identical gradients on every rank."""

    @staticmethod
    def forward(ctx, means3d, scales, quats, opacities, colors, background, camera, tile_size, rank, world, group, live=True):
        import numpy as np
        from ._fused import WHOLE, _Frame
        H, W = camera.H, camera.W
        th = -(-H // tile_size)
        rows, bands = band_plan(th, world)
        band = _band_of(bands[rank], th)
        slab = rows * tile_size
        dev = means3d.device
        buf = torch.empty((max(world * slab, H), W, 3), dtype=torch.float32, device=dev)
        frame = _Frame(means3d.detach(), scales.detach(), quats.detach(), opacities.detach(), colors.detach(), camera, background,
                       tile_size, None, band, buf, 0, own=True, own_last=False)
        info = {}
        _, M = frame.finish(WHOLE, info)
        if world > 1 and live:
            dist.all_gather_into_tensor(buf[:world * slab], buf[rank * slab:(rank + 1) * slab], group=group)
        elif world > 1:
            buf[:min(rank * slab, H)].zero_()      # (a rehearsed rank: the other ranks' rows are never rendered)
            buf[min((rank + 1) * slab, H):H].zero_()
        img = buf[:H]
        ctx.empty = info["on_grid"] == 0   # (a differentiable frame is never pre-culled: the count is the whole frame's, the same on every rank)
        ctx.camera, ctx.tile_size, ctx.band, ctx.group, ctx.world = camera, tile_size, band, group, (world if live else 1)
        m3, sc, qu, op, col, bg = frame.keep[:6]
        ctx.scratch = (frame.ws, frame.isect, np.array(frame.st["host_np"], dtype=np.int64, copy=True))
        ctx.save_for_backward(m3, sc, qu, op, col, bg, frame.alphas, img)
        if ctx.empty:
            return torch.zeros_like(img)   # zeros, not the background (reference render.py:73-76)
        return img

    @staticmethod
    def backward(ctx, v_img):
        from . import _hip
        from .projection import EPS2D
        m3, sc, qu, op, col, bg, alphas, img = ctx.saved_tensors
        cam, ts, (r0, r1) = ctx.camera, ctx.tile_size, ctx.band
        ws, isect, host = ctx.scratch
        L = _hip.lib()
        N = m3.shape[0]
        dev = m3.device
        z = lambda *s_: torch.empty(*s_, dtype=torch.float32, device=dev)
        v_means3d, v_scales, v_quats, v_opac, v_colors = z(N, 3), z(N, 3), z(N, 4), z(N), z(N, 3)
        if ctx.empty or N == 0:
            return (torch.zeros_like(m3), torch.zeros_like(sc), torch.zeros_like(qu), torch.zeros_like(op), torch.zeros_like(col),
                    None if bg is None else torch.zeros_like(bg), None, None, None, None, None, None)
        v_img = _hip.f32c(v_img)
        rows = torch.empty(L.ms_render_bwd_rows_bytes(N) // 4, dtype=torch.float32, device=dev)
        vm = cam._viewmat_f32().to(dev)
        with _hip.on_device(dev):
            _hip.check(L.ms_render_bwd_rows(N, 3, cam.W, cam.H, ts, r0, r1, _hip.ptr(bg), _hip.ptr(ws), ws.numel(), _hip.ptr(isect),
                                            0 if isect is None else isect.numel(), host.ctypes.data, _hip.ptr(img), _hip.ptr(alphas),
                                            _hip.ptr(v_img), None, _hip.ptr(rows), None, _hip.stream(dev)), "ms_render_bwd_rows")
            if ctx.world > 1:
                dist.all_reduce(rows, op=dist.ReduceOp.SUM, group=ctx.group)   # 64 bytes per Gaussian: the one exchange of the step
            _hip.check(L.ms_render_bwd_finish(N, _hip.ptr(m3), _hip.ptr(sc), 1, _hip.ptr(qu), _hip.ptr(op), 3, _hip.ptr(vm), cam.fx,
                                              cam.fy, cam.cx, cam.cy, cam.W, cam.H, EPS2D, _hip.ptr(rows), _hip.ptr(v_means3d),
                                              _hip.ptr(v_scales), _hip.ptr(v_quats), _hip.ptr(v_opac), _hip.ptr(v_colors),
                                              _hip.stream(dev)), "ms_render_bwd_finish")
        v_bg = None
        if bg is not None and ctx.needs_input_grad[5]:
            y0, y1 = min(r0 * ts, cam.H), min(r1 * ts, cam.H)
            v_bg = ((1.0 - alphas[y0:y1])[..., None] * v_img[y0:y1]).sum(dim=(0, 1))
            if ctx.world > 1:
                dist.all_reduce(v_bg, op=dist.ReduceOp.SUM, group=ctx.group)
        return v_means3d, v_scales, v_quats, v_opac, v_colors, v_bg, None, None, None, None, None, None


def render_gaussians_trainable_sharded(means3d, scales, quats, opacities, features, camera: Camera, background_color=None,
                                       tile_size: int = 16, group=None, stages=None, rehearse: Optional[Tuple[int, int]] = None):
    """The differentiable twin of render_gaussians_sharded: every rank returns the full (H, W, 3) image and, after
    backward(), the FULL gradients of its (identical) inputs -- the training step of one frame cut into tile-row bands.
    Rank r renders and differentiates only its band; the exchanges are the framebuffer all-gather of the forward and ONE
    all-reduce of the per-Gaussian gradient rows in the backward.  Inputs, camera and the loss
    must be identical on all ranks.  Bands are equal tile-row bands at the given tile size (which is also the binning
    grid here: a differentiable band keeps whole tile rows).

    `stages`: CPU tests inject differentiable torch stage functions (oracle/torch_oracle.py) --
        project(means3d, scales, quats, opacities, camera) -> means2d, conics, depths, radii (radii / ids non-differentiable)
        bin(means2d, radii, depths, tile_size, tw, th) -> ids, tile_ranges
        raster(means2d, conics, colors, opacities, bg, ranges, ids, camera, tile_size) -> (H, W, C) image
    rehearse=(rank, world) (HIP path): that rank's share of the step WITHOUT a process group and without the two exchanges --
    its band's forward and backward, gradients of its band's pixels only: single-GPU timing of one rank (scripts/band_train_bench.py).
    The reference has no counterpart (no backward: render.py:11; no distributed path).
    A camera whose view_matrix requires grad is refused (ValueError): the pose gradient would need an all-reduce of its own
    over the ranks, which this path does not do -- render_gaussians_trainable differentiates the pose on one GPU."""
    if camera.view_matrix is not None and camera.view_matrix.requires_grad:
        raise ValueError("render_gaussians_trainable_sharded: no gradient w.r.t. the camera pose (view_matrix requires grad); "
                         "use render_gaussians_trainable")
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    if rehearse is not None:
        if stages is not None:
            raise ValueError("rehearse= is for the HIP path")
        rank, world = rehearse
    dev = means3d.device
    C = features.shape[-1]
    H, W = camera.H, camera.W
    th = -(-H // tile_size)
    bg = torch.zeros(C, device=dev) if background_color is None else torch.as_tensor(background_color, dtype=torch.float32, device=dev)
    if stages is None:
        from . import _hip
        _hip.require_cuda(means3d, scales, quats, opacities, features, what="gaussian tensor")
        if C != 3 or features.dtype != torch.float32 or tile_size % 16 != 0:
            raise ValueError("render_gaussians_trainable_sharded: the HIP path takes three float32 channels and a tile size that is a multiple of 16")
        return _RenderBandHip.apply(means3d, scales, quats, opacities.reshape(-1), features, bg, camera, tile_size, rank, world, group,
                                    rehearse is None)
    rows, bands = band_plan(th, world)
    slab = rows * tile_size
    if world > 1:
        means3d, scales, quats, opacities, features = (_ReduceGrad.apply(t, group) for t in (means3d, scales, quats, opacities, features))
    means2d, conics, depths, radii = stages.project(means3d, scales, quats, opacities, camera)
    tw = -(-W // tile_size)
    with torch.no_grad():
        ids, ranges = stages.bin(means2d.detach(), radii, depths.detach(), tile_size, tw, th)
    if ids.numel() == 0:
        return (means3d.sum() + features.sum()) * 0 + torch.zeros(H, W, C, dtype=features.dtype, device=dev)
    img = stages.raster(means2d, conics, features, opacities, bg.to(features.dtype), ranges, ids, camera, tile_size)
    if world == 1:
        return img
    return _GatherBands.apply(img, H, slab, rank, world, group)
