"""Export a scene for viewers, and read such files back: the PlayCanvas / SuperSplat COMPRESSED PLY (16 bytes per Gaussian, one
byte per higher-order SH coefficient, 72 bytes per chunk of 256 Gaussians) and the 32-byte-per-Gaussian ``.splat`` -- with
sceneio's ``save_ply`` the three targets of gsplat's ``export_splats(format="ply" | "ply_compressed" | "splat")``::

    save_compressed_ply("scene.compressed.ply", params)            # the dict save_ply takes; Morton order, spatially tight chunks
    save_splat("scene.splat", params)                              # degree 0 only, the most important Gaussians first
    params = load_compressed_ply("scene.compressed.ply")           # float32, contiguous leaf tensors, features (N, K, 3)

``params``: as ``sceneio.save_ply`` takes it, with the same checks and the same ValueErrors ("means3d" (N, 3); "scales" (N, 3),
log space; "quats" (N, 4), wxyz; "opacities" (N,), a logit or -- ``opacity_space="linear"`` -- the opacity itself; "features"
(N, K, 3) SH coefficients or (N, 3) RGB).  Both formats are LOSSY.  NON-FINITE INPUTS AND ZERO QUATERNIONS ARE UNDEFINED
BEHAVIOUR of the formats and are not checked (a check would cost a host wait); so is a chunk column that holds both -0.0 and
+0.0 as its extreme (which zero the chunk stores is unspecified).

THE SPLIT BETWEEN TORCH AND THE KERNEL (sceneio's convention).  Transcendental and normalising conversions are plain torch
ops, THE SAME OPS FOR BOTH BACKENDS, before the kernel when saving and after it when loading.  ``backend="torch"`` is the
definition of the rest; ``backend="hip"`` (csrc/splatio.hip: ``ms_splat_compress``, ``ms_splat_decompress``,
``ms_splat32_pack``, ``ms_splat32_unpack``, one launch each, no atomics, no workspace, no host wait, no fallback) does only work
that is exact in IEEE float32 -- compare, subtract, divide, multiply, add, floor, trunc, sqrt, convert, each rounded on its
own, in the definition's order -- and gives the definition's bits.

The PREPARED inputs of the packing, in torch, in file order (after ``index_select`` by ``perm``):
``pos`` (N, 3) the means; ``rot`` (N, 4) ``quats / quats.norm(dim=1, keepdim=True)``; ``lsc`` (N, 3) ``scales.clamp(-20, 20)``;
``rgba`` (N, 4) ``features[:, 0, :] * SH_C0 + 0.5`` and then ``sigmoid(logit)`` (the opacity itself for "linear"); ``shr``
(N, 3 (K - 1)) the higher-order coefficients CHANNEL-major exactly as ``f_rest_*`` (none when K == 1).

COMPRESSED PLY: THE DEFINITION (written from the PlayCanvas engine's reader and splat-transform's writer; this text decides).
Header: ``ply`` / ``format binary_little_endian 1.0``, then three elements in this order (``compressed_ply_header(N, K)``
returns the exact bytes): ``element chunk C``, C = ceil(N / 256), 18 ``property float``: ``min_x min_y min_z max_x max_y max_z
min_scale_x min_scale_y min_scale_z max_scale_x max_scale_y max_scale_z min_r min_g min_b max_r max_g max_b``; ``element
vertex N`` with ``property uint`` ``packed_position packed_rotation packed_scale packed_color``; ``element sh N``, only if
K > 1, with ``property uchar f_rest_0 .. f_rest_{3 (K - 1) - 1}``.  The body follows ``end_header``: the chunk rows, the vertex
rows, the sh rows.
  Chunks.  Chunk c covers file rows [256 c, min(256 c + 256, N)); its mins and maxes are over the rows it has, of ``pos``,
  ``lsc`` and the first three columns of ``rgba``.
  Helpers.  ``norm(v, lo, hi)`` = 0 if v <= lo; 1 if v >= hi; 0 if hi - lo < 1e-5f; otherwise (v - lo) / (hi - lo).
  ``pack(v, b)``, t = float(2^b - 1): uint(min(t, max(0, floor(v * t + 0.5f)))).
  Position and scale.  ``packed_position = pack(nx, 11) << 21 | pack(ny, 10) << 11 | pack(nz, 11)``, n* normalised by the chunk;
  ``packed_scale`` the same on ``lsc``.
  Colour.  ``packed_color = pack(nr, 8) << 24 | pack(ng, 8) << 16 | pack(nb, 8) << 8 | pack(a, 8)``; r g b normalised by the
  chunk, a the opacity, not normalised.
  Rotation.  a[0..3] = rot (w x y z); L = the first index of the largest |a[i]|; if a[L] < 0 negate all four; word = L; for
  i = 0..3 with i != L, in order: ``word = word << 10 | pack(a[i] * 0.70710678f + 0.5f, 10)``.
  SH bytes.  ``uint8(min(255, max(0, trunc((v / 8 + 0.5f) * 256))))``.
  Decoding.  ``u(x, b) = float(x & (2^b - 1)) / float(2^b - 1)``; position, scale and rgb are ``lo * (1 - u) + hi * u``; the
  opacity is ``u(word, 8)``; the three stored rotation components are ``(u - 0.5f) * 1.41421356f`` = a, b, c and
  ``m = sqrt(max(0, ((1 - a a) - b b) - c c))`` (correctly rounded) goes at index L; SH is ``float(byte) * (8.0f / 255.0f) - 4.0f``.
  Torch then does ``f_dc = (rgb - 0.5) / SH_C0`` and, for the logit space, ``log(o) - log1p(-o)`` on ``o.clamp(1/510, 1 - 1/510)``
  (bytes 0 and 255 stay finite).  Scales come back as the decoded log-scales, quats as the decoded unit quaternion.
  Order.  ``order="morton"`` (the default): ``scene_order.morton_permutation(means3d)``, so that chunks are spatially tight;
  ``"keep"``: the identity.  ``CompressedScene.perm[i]`` is the Gaussian of ``params`` that file row i holds.
``load_compressed_ply`` ACCEPTS FOREIGN FILES: chunk properties are found by name, 12 or 18 of them (with 12, colour min / max
are 0 and 1); the four vertex words are found by name; the ``sh`` element is optional, with 3 (K - 1) uchar properties (9, 24,
45; 72 for degree 4); other properties, elements and ``comment`` lines are skipped.  Each a ValueError before anything is
launched: C != ceil(N / 256), N == 0, an ascii or big-endian file, a missing property (or one of another type), a short body.

.SPLAT: THE DEFINITION.  N rows of 32 bytes, no header: ``pos`` 3 x f32; ``exp(scales)`` 3 x f32 (the exp is torch); rgba
4 x u8, ``uint8(min(255, max(0, trunc(v * 255))))`` of the prepared ``rgba``; rot 4 x u8, ``uint8(min(255, max(0, trunc(r * 128 +
128))))`` of the unit quaternion wxyz.  ``order="importance"`` (the default): rows sorted ascending by ``-(exp((s0 + s1) + s2) *
opacity)``, in torch, a stable sort; ``"keep"``: the identity.  Decoding: colour ``byte / 255``, rot ``(byte - 128) / 128``,
scales ``log`` in torch, features (N, 1, 3).  A FILE HOLDS DEGREE 0 ONLY: ``save_splat`` of a scene with K > 1 drops the higher
degrees.  ``load_splat`` raises ValueError for a file size that is not a positive multiple of 32.

Both ``save_*`` write ``path + ".tmp"`` and rename it over ``path``.  For backend="hip" the tensors must be float32, contiguous
CUDA/ROCm tensors (ValueError otherwise; no fallback) and each file costs the device-to-host copies of its elements.

Not covered: ``.spz``, k-means / PNG compression, reading compressed files through ``load_ply``, optimiser moments, the sharded
trainer.
"""
import os
import sys
from typing import NamedTuple, Optional

import numpy as np
import torch

from .knn import SH_C0
from .sceneio import _check_backend, _check_space, _sh_features, _supported_K, _validate_params

CHUNK = 256
CHUNK_PROPERTIES = ("min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "min_scale_x", "min_scale_y", "min_scale_z",
                    "max_scale_x", "max_scale_y", "max_scale_z", "min_r", "min_g", "min_b", "max_r", "max_g", "max_b")
VERTEX_PROPERTIES = ("packed_position", "packed_rotation", "packed_scale", "packed_color")
SPLAT_ROW = 32
# the float32 constants of the definition, as Python floats that ARE float32 values (what the kernel's literals round to)
_EPS = float(np.float32(1e-5))
_SQRT1_2 = float(np.float32(0.70710678))
_SQRT2 = float(np.float32(1.41421356))
_SH_STEP = float(np.float32(8.0) / np.float32(255.0))
_O_MIN = 1.0 / 510.0
_HEADER_LIMIT = 1 << 20
_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2",
          "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4",
          "double": "<f8", "float64": "<f8"}


class CompressedScene(NamedTuple):
    """A scene as a compressed PLY holds it: ``chunks`` float32 (C, 18) (a foreign file's: (C, 12)); ``vertices`` int32 (N, 4),
    the four packed uint32 words as bits; ``sh`` uint8 (N, 3 (K - 1)), or None when K == 1; ``perm`` int64 (N,): row i is
    Gaussian ``perm[i]`` of the params it was made from (None: unknown, a loaded file); ``K``."""
    chunks: torch.Tensor
    vertices: torch.Tensor
    sh: Optional[torch.Tensor]
    perm: Optional[torch.Tensor]
    K: int


# ---------------------------------------------------------------------------------------------------------------------------
# the torch side of both backends: preparing and finishing

def _linear_opacity(o, opacity_space):
    return torch.sigmoid(o) if opacity_space == "logit" else o


def _prepare(t, K, perm, opacity_space):
    """The five validated tensors (features already SH) -> pos, rot, lsc, rgba, shr (or None), float32, contiguous, in file order."""
    means, scales, quats, opac, feats = (x.float().index_select(0, perm) for x in t)
    rot = quats / quats.norm(dim=1, keepdim=True)
    lsc = scales.clamp(-20.0, 20.0)
    rgba = torch.cat([feats[:, 0, :] * SH_C0 + 0.5, _linear_opacity(opac, opacity_space).unsqueeze(1)], 1)
    shr = feats[:, 1:, :].transpose(1, 2).reshape(means.shape[0], 3 * (K - 1)).contiguous() if K > 1 else None
    return means.contiguous(), rot.contiguous(), lsc.contiguous(), rgba.contiguous(), shr


def _finish(pos, rot, scales, rgba, shr, K, opacity_space, requires_grad):
    """Decoded pos, rot, LOG-scales, rgba, shr (or None) -> the params dict."""
    N = pos.shape[0]
    f_dc = (rgba[:, :3] - 0.5) / SH_C0
    if K > 1:
        features = torch.cat([f_dc.unsqueeze(1), shr.reshape(N, 3, K - 1).transpose(1, 2)], 1)
    else:
        features = f_dc.unsqueeze(1)
    o = rgba[:, 3]
    if opacity_space == "logit":
        o = o.clamp(_O_MIN, 1.0 - _O_MIN)
        o = torch.log(o) - torch.log1p(-o)
    out = {"means3d": pos, "scales": scales, "quats": rot, "opacities": o, "features": features}
    return {k: x.detach().contiguous().requires_grad_(bool(requires_grad)) for k, x in out.items()}


def _as_words(w):
    """int64 words in [0, 2^32) -> the same bits as int32."""
    return (w - ((w >> 31) << 32)).to(torch.int32)


def _from_words(v):
    """int32 bits -> int64 words in [0, 2^32)."""
    return v.to(torch.int64) & 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------------
# the definition (module docstring), on any device: every line one float32 operation per element

def _norm(v, lo, hi):
    d = hi - lo
    return torch.where(v <= lo, torch.zeros_like(v),
                       torch.where(v >= hi, torch.ones_like(v), torch.where(d < _EPS, torch.zeros_like(v), (v - lo) / d)))


def _pack(v, bits):
    t = float((1 << bits) - 1)
    return torch.floor(v * t + 0.5).clamp(0.0, t).to(torch.int64)


def _byte(x):
    return torch.trunc(x).clamp(0.0, 255.0).to(torch.uint8)


def _div(x, c):
    """x / c for a constant c, correctly rounded: by a tensor on x's device (on a GPU torch turns a division by a Python
    scalar into a multiplication by the rounded reciprocal, which is another number)."""
    return x / torch.full((), c, dtype=torch.float32, device=x.device)


def _unit(x, bits):
    mask = (1 << bits) - 1
    return _div((x & mask).to(torch.float32), float(mask))


def _mix(lo, hi, u):
    return lo * (1.0 - u) + hi * u


def _rows_of(chunks, N):
    return chunks.repeat_interleave(CHUNK, 0)[:N]


def _compress_torch(pos, rot, lsc, rgba, shr):
    N, dev = pos.shape[0], pos.device
    C = -(-N // CHUNK)
    v9 = torch.cat([pos, lsc, rgba[:, :3]], 1)
    pad = C * CHUNK - N
    inf = torch.full((pad, 9), float("inf"), dtype=torch.float32, device=dev)
    mn = torch.cat([v9, inf], 0).view(C, CHUNK, 9).amin(1)
    mx = torch.cat([v9, -inf], 0).view(C, CHUNK, 9).amax(1)
    chunks = torch.cat([mn[:, 0:3], mx[:, 0:3], mn[:, 3:6], mx[:, 3:6], mn[:, 6:9], mx[:, 6:9]], 1).contiguous()
    per = _rows_of(chunks, N)
    lo = torch.cat([per[:, 0:3], per[:, 6:9], per[:, 12:15]], 1)
    hi = torch.cat([per[:, 3:6], per[:, 9:12], per[:, 15:18]], 1)
    u = _norm(v9, lo, hi)
    position = _pack(u[:, 0], 11) << 21 | _pack(u[:, 1], 10) << 11 | _pack(u[:, 2], 11)
    scale = _pack(u[:, 3], 11) << 21 | _pack(u[:, 4], 10) << 11 | _pack(u[:, 5], 11)
    colour = _pack(u[:, 6], 8) << 24 | _pack(u[:, 7], 8) << 16 | _pack(u[:, 8], 8) << 8 | _pack(rgba[:, 3], 8)
    mag = rot.abs()
    L = torch.zeros(N, dtype=torch.int64, device=dev)
    best = mag[:, 0]
    for i in range(1, 4):
        gt = mag[:, i] > best
        L = torch.where(gt, torch.full_like(L, i), L)
        best = torch.where(gt, mag[:, i], best)
    top = rot.gather(1, L.unsqueeze(1))
    a = torch.where(top < 0, -rot, rot)
    rotation = L
    for i in range(4):
        rotation = torch.where(L != i, rotation << 10 | _pack(a[:, i] * _SQRT1_2 + 0.5, 10), rotation)
    vertices = _as_words(torch.stack([position, rotation, scale, colour], 1)).contiguous()
    sh = _byte((_div(shr, 8.0) + 0.5) * 256.0).contiguous() if shr is not None else None
    return chunks, vertices, sh


def _decompress_torch(chunks, vertices, sh):
    N, dev = vertices.shape[0], vertices.device
    if chunks.shape[1] == 12:
        C = chunks.shape[0]
        chunks = torch.cat([chunks, torch.zeros((C, 3), dtype=torch.float32, device=dev),
                            torch.ones((C, 3), dtype=torch.float32, device=dev)], 1)
    per = _rows_of(chunks, N)
    w = _from_words(vertices)
    p, r, s, c = w[:, 0], w[:, 1], w[:, 2], w[:, 3]
    pos = torch.stack([_mix(per[:, 0], per[:, 3], _unit(p >> 21, 11)), _mix(per[:, 1], per[:, 4], _unit(p >> 11, 10)),
                       _mix(per[:, 2], per[:, 5], _unit(p, 11))], 1)
    lsc = torch.stack([_mix(per[:, 6], per[:, 9], _unit(s >> 21, 11)), _mix(per[:, 7], per[:, 10], _unit(s >> 11, 10)),
                       _mix(per[:, 8], per[:, 11], _unit(s, 11))], 1)
    rgba = torch.stack([_mix(per[:, 12], per[:, 15], _unit(c >> 24, 8)), _mix(per[:, 13], per[:, 16], _unit(c >> 16, 8)),
                        _mix(per[:, 14], per[:, 17], _unit(c >> 8, 8)), _unit(c, 8)], 1)
    L = r >> 30
    a, b, cc = ((_unit(r >> sft, 10) - 0.5) * _SQRT2 for sft in (20, 10, 0))
    # (the correctly rounded float32 square root: taken in float64 and rounded once more, which is exact for a square root of a
    # float32; torch's own float32 sqrt is not correctly rounded on every CPU)
    m = torch.sqrt((((1.0 - a * a) - b * b) - cc * cc).clamp_min(0.0).double()).float()
    rot = torch.stack([torch.where(L == 0, m, a), torch.where(L == 1, m, torch.where(L == 0, a, b)),
                       torch.where(L == 2, m, torch.where(L < 2, b, cc)), torch.where(L == 3, m, cc)], 1)
    shr = sh.to(torch.float32) * _SH_STEP - 4.0 if sh is not None else None
    return pos.contiguous(), rot.contiguous(), lsc.contiguous(), rgba.contiguous(), shr


def _splat32_pack_torch(pos, scale_lin, rgba, rot):
    return torch.cat([pos.contiguous().view(torch.uint8), scale_lin.contiguous().view(torch.uint8), _byte(rgba * 255.0),
                      _byte(rot * 128.0 + 128.0)], 1).contiguous()


def _splat32_unpack_torch(rows):
    pos = rows[:, 0:12].contiguous().view(torch.float32)
    scale_lin = rows[:, 12:24].contiguous().view(torch.float32)
    rgba = _div(rows[:, 24:28].to(torch.float32), 255.0)
    rot = _div(rows[:, 28:32].to(torch.float32) - 128.0, 128.0)
    return pos, scale_lin, rgba.contiguous(), rot.contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels.  ``out``: the tensors to write into (tests: guard-filled, with rows to spare)

def _compress_hip(pos, rot, lsc, rgba, shr, out=None):
    from . import _hip
    L = _hip.lib()
    N, dev = pos.shape[0], pos.device
    K = 1 if shr is None else shr.shape[1] // 3 + 1
    if out is None:
        out = (torch.empty((-(-N // CHUNK), 18), dtype=torch.float32, device=dev),
               torch.empty((N, 4), dtype=torch.int32, device=dev),
               torch.empty((N, 3 * (K - 1)), dtype=torch.uint8, device=dev) if K > 1 else None)
    chunks, vertices, sh = out
    with _hip.on_device(dev):
        _hip.check(L.ms_splat_compress(N, K, _hip.ptr(pos), _hip.ptr(rot), _hip.ptr(lsc), _hip.ptr(rgba), _hip.ptr(shr),
                                       _hip.ptr(chunks), _hip.ptr(vertices), _hip.ptr(sh), _hip.stream(dev)), "ms_splat_compress")
    return chunks, vertices, sh


def _decompress_hip(chunks, vertices, sh, out=None):
    from . import _hip
    L = _hip.lib()
    N, dev = vertices.shape[0], vertices.device
    K = 1 if sh is None else sh.shape[1] // 3 + 1
    if out is None:
        out = tuple(torch.empty((N, w), dtype=torch.float32, device=dev) for w in (3, 4, 3, 4)) + \
            ((torch.empty((N, 3 * (K - 1)), dtype=torch.float32, device=dev),) if K > 1 else (None,))
    pos, rot, lsc, rgba, shr = out
    with _hip.on_device(dev):
        _hip.check(L.ms_splat_decompress(N, K, chunks.shape[1], _hip.ptr(chunks), _hip.ptr(vertices), _hip.ptr(sh), _hip.ptr(pos),
                                         _hip.ptr(rot), _hip.ptr(lsc), _hip.ptr(rgba), _hip.ptr(shr), _hip.stream(dev)),
                   "ms_splat_decompress")
    return pos, rot, lsc, rgba, shr


def _splat32_pack_hip(pos, scale_lin, rgba, rot, out=None):
    from . import _hip
    L = _hip.lib()
    N, dev = pos.shape[0], pos.device
    rows = torch.empty((N, SPLAT_ROW), dtype=torch.uint8, device=dev) if out is None else out
    with _hip.on_device(dev):
        _hip.check(L.ms_splat32_pack(N, _hip.ptr(pos), _hip.ptr(scale_lin), _hip.ptr(rgba), _hip.ptr(rot), _hip.ptr(rows),
                                     _hip.stream(dev)), "ms_splat32_pack")
    return rows


def _splat32_unpack_hip(rows, out=None):
    from . import _hip
    L = _hip.lib()
    N, dev = rows.shape[0], rows.device
    if out is None:
        out = tuple(torch.empty((N, w), dtype=torch.float32, device=dev) for w in (3, 3, 4, 4))
    pos, scale_lin, rgba, rot = out
    with _hip.on_device(dev):
        _hip.check(L.ms_splat32_unpack(N, _hip.ptr(rows), _hip.ptr(pos), _hip.ptr(scale_lin), _hip.ptr(rgba), _hip.ptr(rot),
                                       _hip.stream(dev)), "ms_splat32_unpack")
    return pos, scale_lin, rgba, rot


def _check_hip_tensor(name, x, dtype):
    if not x.is_cuda:
        raise ValueError(f"backend='hip': {name} must be a CUDA/ROCm tensor (there is no fallback)")
    if x.dtype != dtype:
        raise ValueError(f"backend='hip': {name} must be {dtype}, got {x.dtype}")
    if not x.is_contiguous():
        raise ValueError(f"backend='hip': {name} must be contiguous")


# ---------------------------------------------------------------------------------------------------------------------------
# compressed PLY

def _check_order(order, allowed):
    if order not in allowed:
        raise ValueError(f"Invalid order: {order!r} ({' or '.join(repr(a) for a in allowed)})")


@torch.no_grad()
def compress_scene(params, *, opacity_space="logit", order="morton", backend="hip") -> CompressedScene:
    """``params`` -> what a compressed PLY of it holds (module docstring), on params' device.  backend="torch": the
    definition.  backend="hip": ms_splat_compress, one launch on the current stream behind the torch ops that prepare its
    inputs, no host wait; CUDA/ROCm, float32, contiguous tensors; bit for bit the definition; no fallback.  Non-finite values
    and zero quaternions are undefined behaviour and not checked."""
    _check_space(opacity_space)
    _check_order(order, ("morton", "keep"))
    N, K, t = _validate_params(params, backend)
    t[4] = _sh_features(t[4], K)
    K = K or 1
    if order == "morton":
        from .scene_order import morton_permutation
        perm = morton_permutation(t[0])
    else:
        perm = torch.arange(N, dtype=torch.int64, device=t[0].device)
    prepared = _prepare(t, K, perm, opacity_space)
    chunks, vertices, sh = _compress_torch(*prepared) if backend == "torch" else _compress_hip(*prepared)
    return CompressedScene(chunks, vertices, sh, perm, K)


def _check_compressed(cs, backend):
    _check_backend(backend)
    chunks, vertices, sh, K = cs.chunks, cs.vertices, cs.sh, cs.K
    if K not in _supported_K():
        raise ValueError(f"K = {K!r} is not a supported number of SH coefficients {_supported_K()}")
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 4 or vertices.dtype != torch.int32:
        raise ValueError("vertices must be an int32 tensor of shape (N, 4)")
    N = vertices.shape[0]
    if N == 0:
        raise ValueError("an empty scene (N == 0) is not read")
    if not isinstance(chunks, torch.Tensor) or chunks.dim() != 2 or chunks.shape[1] not in (12, 18) or chunks.dtype != torch.float32:
        raise ValueError("chunks must be a float32 tensor of shape (C, 18) or (C, 12)")
    if chunks.shape[0] != -(-N // CHUNK):
        raise ValueError(f"{chunks.shape[0]} chunks for {N} vertices: C = ceil(N / {CHUNK}) = {-(-N // CHUNK)} is required")
    if (sh is None) != (K == 1):
        raise ValueError(f"sh must be None exactly when K == 1 (K = {K})")
    if sh is not None and (not isinstance(sh, torch.Tensor) or tuple(sh.shape) != (N, 3 * (K - 1)) or sh.dtype != torch.uint8):
        raise ValueError(f"sh must be a uint8 tensor of shape (N, {3 * (K - 1)})")
    tensors = [("chunks", chunks, torch.float32), ("vertices", vertices, torch.int32)] + ([("sh", sh, torch.uint8)] if K > 1 else [])
    if any(x.device != vertices.device for _, x, _ in tensors):
        raise ValueError("the tensors are on different devices")
    if backend == "hip":
        for name, x, dtype in tensors:
            _check_hip_tensor(name, x, dtype)
    return N


@torch.no_grad()
def decompress_scene(cs, *, opacity_space="logit", backend="hip", requires_grad=False) -> dict:
    """A CompressedScene -> the params dict it decodes to, in FILE order (``cs.perm`` is not undone: the format is lossy, and a
    loaded file has none): float32, contiguous leaf tensors on cs's device; "opacities" a logit of the byte clamped to [1/510,
    1 - 1/510], or the byte / 255 for opacity_space="linear"; features (N, K, 3).  backend="hip": ms_splat_decompress, one
    launch, no host wait; CUDA/ROCm contiguous tensors; bit for bit the definition; no fallback."""
    _check_space(opacity_space)
    _check_compressed(cs, backend)
    dec = _decompress_torch(cs.chunks, cs.vertices, cs.sh) if backend == "torch" else _decompress_hip(cs.chunks, cs.vertices, cs.sh)
    return _finish(*dec, cs.K, opacity_space, requires_grad)


def compressed_ply_header(N, K) -> bytes:
    """The exact header bytes of a compressed PLY of N Gaussians with K SH coefficients per channel (module docstring)."""
    if not (isinstance(N, int) and not isinstance(N, bool) and N >= 1):
        raise ValueError(f"N must be a positive int, got {N!r}")
    if K not in _supported_K():
        raise ValueError(f"K = {K!r} is not a supported number of SH coefficients {_supported_K()}")
    lines = ["ply", "format binary_little_endian 1.0", f"element chunk {-(-N // CHUNK)}"] + \
        [f"property float {p}" for p in CHUNK_PROPERTIES] + [f"element vertex {N}"] + [f"property uint {p}" for p in VERTEX_PROPERTIES]
    if K > 1:
        lines += [f"element sh {N}"] + [f"property uchar f_rest_{i}" for i in range(3 * (K - 1))]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def _little_endian(a):
    return a if sys.byteorder == "little" or a.dtype.itemsize == 1 else a.byteswap()


def _write(path, parts) -> int:
    """``parts`` (bytes or C-contiguous numpy arrays) to ``path + ".tmp"``, renamed over ``path`` -> the bytes written."""
    path = os.fspath(path)
    tmp = path + ".tmp"
    total = 0
    try:
        with open(tmp, "wb") as f:
            for p in parts:
                total += f.write(p if isinstance(p, bytes) else memoryview(_little_endian(p)).cast("B"))
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return total


def save_compressed_ply(path, params, *, opacity_space="logit", order="morton", backend="hip") -> int:
    """Write ``params`` to ``path`` as a compressed PLY (module docstring) -> the bytes written.  The tensors are not changed.
    backend="hip": packed on the device, then the three elements are copied to the host (the waits are inherent); no fallback."""
    cs = compress_scene(params, opacity_space=opacity_space, order=order, backend=backend)
    N = cs.vertices.shape[0]
    parts = [compressed_ply_header(N, cs.K), cs.chunks.cpu().numpy(), cs.vertices.cpu().numpy()]
    if cs.K > 1:
        parts.append(cs.sh.cpu().numpy())
    return _write(path, parts)


def _parse_elements(head):
    """The header at the start of ``head`` -> ([(element name, count, [(numpy type, property name)])], body offset)."""
    end = head.find(b"end_header")
    nl = head.find(b"\n", end) if end >= 0 else -1
    if not head.startswith(b"ply") or nl < 0:
        raise ValueError("not a PLY file: no 'ply' ... 'end_header' in its first bytes")
    try:
        lines = [ln.strip() for ln in head[:end].decode("ascii").splitlines()]
    except UnicodeDecodeError:
        raise ValueError("not a PLY file: the header is not ascii") from None
    fmt, elements = None, []
    for ln in lines[1:]:
        w = ln.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1:]
        elif w[0] == "element" and len(w) == 3 and w[2].isdigit():
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements and len(w) == 3 and w[1] in _TYPES:
            elements[-1][2].append((_TYPES[w[1]], w[2]))
        else:
            raise ValueError(f"malformed or unsupported header line: {ln!r}")
    if fmt != ["binary_little_endian", "1.0"]:
        raise ValueError(f"format {' '.join(fmt) if fmt else None!r}: only 'binary_little_endian 1.0' is read")
    return elements, nl + 1


def _columns(path, what, names, want, table, props):
    """The properties ``names`` of one element's rows ``table`` as a C-contiguous (rows, len(names)) array of type ``want``."""
    types = dict((n, t) for t, n in props)
    missing = [n for n in names if n not in types]
    if missing:
        raise ValueError(f"{path}: element {what} lacks the properties {missing[:4]}{' ...' if len(missing) > 4 else ''}")
    wrong = [n for n in names if types[n] != want]
    if wrong:
        raise ValueError(f"{path}: element {what}: property {wrong[0]!r} has another type than the format's")
    return np.stack([table[n] for n in names], 1).astype(want.lstrip("<"), copy=False) if len(table) else \
        np.zeros((0, len(names)), dtype=want.lstrip("<"))


def load_compressed_ply(path, *, device=None, opacity_space="logit", requires_grad=False, backend="hip") -> dict:
    """Read the compressed PLY in ``path`` (this module's files and foreign ones: module docstring) -> the params dict, in file
    order: float32, contiguous leaf tensors on ``device`` (default: the current CUDA/ROCm device for backend="hip", the CPU for
    "torch") with ``requires_grad`` as given; features always (N, K, 3).  Every check is made before anything is launched."""
    _check_space(opacity_space)
    _check_backend(backend)
    path = os.fspath(path)
    with open(path, "rb") as f:
        head = f.read(1 << 16)
        while b"end_header" not in head and len(head) < _HEADER_LIMIT:
            more = f.read(1 << 16)
            if not more:
                break
            head += more
    elements, offset = _parse_elements(head)
    by_name = {}
    for name, count, props in elements:
        if len({n for _, n in props}) != len(props):
            raise ValueError(f"{path}: element {name} has duplicate property names")
        dtype = np.dtype([(n, t) for t, n in props])
        by_name.setdefault(name, (count, props, dtype, offset))
        offset += count * dtype.itemsize
    for need in ("chunk", "vertex"):
        if need not in by_name:
            raise ValueError(f"{path}: no 'element {need}' in the header: not a compressed PLY")
    N, C = by_name["vertex"][0], by_name["chunk"][0]
    if N == 0:
        raise ValueError(f"{path}: the file holds no Gaussian (element vertex 0)")
    if C != -(-N // CHUNK):
        raise ValueError(f"{path}: {C} chunks for {N} vertices: C = ceil(N / {CHUNK}) = {-(-N // CHUNK)} is required")
    chunk_names = [n for _, n in by_name["chunk"][1]]
    n_chunk = 18 if any(p in chunk_names for p in CHUNK_PROPERTIES[12:]) else 12
    R = 0
    if "sh" in by_name:
        if by_name["sh"][0] != N:
            raise ValueError(f"{path}: element sh has {by_name['sh'][0]} rows for {N} vertices")
        R = sum(1 for _, n in by_name["sh"][1] if n.startswith("f_rest_"))
        if R % 3 or R == 0 or R // 3 + 1 not in _supported_K():
            raise ValueError(f"{path}: {R} f_rest_* properties in element sh: 3 (K - 1) with K one of {_supported_K()[1:]} is required")
    K = R // 3 + 1
    if os.path.getsize(path) < offset:
        raise ValueError(f"{path}: the body is shorter than its header says ({os.path.getsize(path)} of {offset} bytes)")

    def table(name):
        count, props, dtype, off = by_name[name]
        return np.fromfile(path, dtype=dtype, count=count, offset=off), props

    chunks = _columns(path, "chunk", CHUNK_PROPERTIES[:n_chunk], "<f4", *table("chunk"))
    vertices = _columns(path, "vertex", VERTEX_PROPERTIES, "<u4", *table("vertex")).view(np.int32)
    sh = _columns(path, "sh", [f"f_rest_{i}" for i in range(R)], "u1", *table("sh")) if R else None
    if backend == "torch":
        dev = torch.device("cpu" if device is None else device)
    else:
        from . import _hip
        _hip.lib()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"backend='hip': device must be a CUDA/ROCm device, got {dev} (there is no fallback)")
    cs = CompressedScene(torch.from_numpy(np.ascontiguousarray(chunks)).to(dev), torch.from_numpy(np.ascontiguousarray(vertices)).to(dev),
                         torch.from_numpy(np.ascontiguousarray(sh)).to(dev) if R else None, None, K)
    return decompress_scene(cs, opacity_space=opacity_space, backend=backend, requires_grad=requires_grad)


# ---------------------------------------------------------------------------------------------------------------------------
# .splat

@torch.no_grad()
def pack_splat_rows(params, *, opacity_space="logit", order="importance", backend="hip"):
    """``params`` -> (the (N, 32) uint8 rows of its .splat file, on params' device; perm int64 (N,): row i is Gaussian
    ``perm[i]``).  Only degree 0 of the features is kept.  backend="hip": ms_splat32_pack, one launch, no host wait; bit for
    bit the definition; no fallback."""
    _check_space(opacity_space)
    _check_order(order, ("importance", "keep"))
    N, K, t = _validate_params(params, backend)
    t[4] = _sh_features(t[4], K)
    if order == "importance":
        s = t[1].float()
        key = -(torch.exp((s[:, 0] + s[:, 1]) + s[:, 2]) * _linear_opacity(t[3].float(), opacity_space))
        perm = torch.argsort(key, stable=True)
    else:
        perm = torch.arange(N, dtype=torch.int64, device=t[0].device)
    pos, rot, _, rgba, _ = _prepare(t, 1, perm, opacity_space)
    scale_lin = torch.exp(t[1].float().index_select(0, perm)).contiguous()
    rows = _splat32_pack_torch(pos, scale_lin, rgba, rot) if backend == "torch" else _splat32_pack_hip(pos, scale_lin, rgba, rot)
    return rows, perm


@torch.no_grad()
def unpack_splat_rows(rows, *, opacity_space="logit", backend="hip", requires_grad=False) -> dict:
    """(N, 32) uint8 rows of a .splat file -> the params dict, features (N, 1, 3) (module docstring)."""
    _check_space(opacity_space)
    _check_backend(backend)
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape[1] != SPLAT_ROW or rows.dtype != torch.uint8:
        raise ValueError(f"rows must be a uint8 tensor of shape (N, {SPLAT_ROW})")
    if rows.shape[0] == 0:
        raise ValueError("rows is empty (N == 0)")
    if backend == "hip":
        _check_hip_tensor("rows", rows, torch.uint8)
    pos, scale_lin, rgba, rot = _splat32_unpack_torch(rows) if backend == "torch" else _splat32_unpack_hip(rows)
    return _finish(pos, rot, torch.log(scale_lin), rgba, None, 1, opacity_space, requires_grad)


def save_splat(path, params, *, opacity_space="logit", order="importance", backend="hip") -> int:
    """Write ``params`` to ``path`` as a .splat file (module docstring) -> the bytes written (32 N).  A SCENE WITH K > 1 LOSES
    ITS HIGHER SH DEGREES: the format holds a colour per Gaussian.  The tensors are not changed.  backend="hip": packed on the
    device, then one device-to-host copy of the rows (the wait is inherent); no fallback."""
    rows, _ = pack_splat_rows(params, opacity_space=opacity_space, order=order, backend=backend)
    return _write(path, [rows.cpu().numpy()])


def load_splat(path, *, device=None, opacity_space="logit", requires_grad=False, backend="hip") -> dict:
    """Read the .splat file in ``path`` -> the params dict, in file order: float32, contiguous leaf tensors on ``device``
    (default: the current CUDA/ROCm device for backend="hip", the CPU for "torch"); features (N, 1, 3).  ValueError, before
    anything is launched: a file size that is not a positive multiple of 32."""
    _check_space(opacity_space)
    _check_backend(backend)
    path = os.fspath(path)
    size = os.path.getsize(path)
    if size == 0 or size % SPLAT_ROW:
        raise ValueError(f"{path}: {size} bytes is not a positive multiple of {SPLAT_ROW}: not a .splat file")
    if sys.byteorder != "little":
        raise ValueError("a .splat file is read on little-endian hosts only")
    if backend == "torch":
        dev = torch.device("cpu" if device is None else device)
    else:
        from . import _hip
        _hip.lib()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"backend='hip': device must be a CUDA/ROCm device, got {dev} (there is no fallback)")
    rows = torch.from_numpy(np.fromfile(path, dtype=np.uint8).reshape(-1, SPLAT_ROW)).to(dev)
    return unpack_splat_rows(rows, opacity_space=opacity_space, backend=backend, requires_grad=requires_grad)


__all__ = ["CompressedScene", "compress_scene", "decompress_scene", "save_compressed_ply", "load_compressed_ply", "save_splat",
           "load_splat", "pack_splat_rows", "unpack_splat_rows", "compressed_ply_header"]
