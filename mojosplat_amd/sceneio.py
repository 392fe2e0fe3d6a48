"""Save a scene as a 3DGS PLY file and load one back: the INRIA ``point_cloud.ply``, the field's interchange format (what the
3DGS code, gsplat's ``export_splats(format="ply")`` and SuperSplat write)::

    save_ply("scene.ply", params)                                   # the dict init_from_points returns and GaussianAdam takes
    params = load_ply("scene.ply", requires_grad=True)              # float32, contiguous leaf tensors on the current GPU
    img = render_gaussians(params["means3d"], params["scales"], params["quats"], params["opacities"],
                           evaluate_sh(params["means3d"], params["features"], cam, 3), cam, backend="hip")

``params``: "means3d" (N, 3); "scales" (N, 3), log space; "quats" (N, 4), wxyz, stored as they are (not normalised);
"opacities" (N,); "features" (N, K, 3) SH coefficients, K = (d + 1)^2 for d = 0 .. MAX_SH_DEGREE, or (N, 3) RGB.  Other keys
are ignored.

THE FILE LAYOUT (this is the definition).  ``ply`` / ``format binary_little_endian 1.0`` / ``element vertex N``, every
property a ``float``, in this order (``ply_header(N, K)`` returns the exact header bytes)::

    x y z    nx ny nz    f_dc_0 f_dc_1 f_dc_2    f_rest_0 .. f_rest_{3 (K - 1) - 1}    opacity    scale_0..2    rot_0..3

``nx ny nz`` are written as +0.0.  ``f_dc_c = features[n, 0, c]``; ``f_rest_{c (K - 1) + (k - 1)} = features[n, k, c]`` for
k >= 1: CHANNEL-major, the INRIA transpose.  ``opacity`` is the logit, ``scale_*`` the log-scales, ``rot_*`` the quaternion
wxyz.  A row is F = 14 + 3 K float32, little-endian; the body is N such rows, nothing after them.

CONVERSIONS live outside the row move and are the same torch ops for both backends.  ``opacity_space="linear"``: save_ply
stores ``log(o) - log1p(-o)``, load_ply returns ``sigmoid`` of the stored value.  (N, 3) RGB features are stored as degree 0,
``f_dc = (rgb - 0.5) / SH_C0``; load_ply always returns (N, K, 3) SH features.  These two round trips go through one rounding
each way and are NOT bit-exact.  Logit opacities and SH features round-trip BIT FOR BIT: NaN payloads, infinities, -0.0 and
denormals included.

``backend="torch"`` is the definition (``pack_ply_rows_torch``, ``unpack_ply_rows_torch``: int32 views moved by plain torch
indexing, on any device; numpy for the file).  ``backend="hip"`` moves the rows with csrc/sceneio.hip (``ms_ply_pack``,
``ms_ply_unpack``: one launch each, the in-row permutation through LDS, bit for bit the definition) and has no fallback.
save_ply packs on the device, copies the rows once to pinned host memory and writes header and body; load_ply reads the body
into a pinned host buffer, copies it to the device once and unpacks.  EACH DIRECTION MAKES ONE DEVICE-TO-HOST WAIT PER FILE
(the copy between the device and the pinned buffer has to finish before the file is written / the buffer is released); that
wait is inherent.  save_ply writes ``path + ".tmp"`` and renames it over ``path``: an interrupted save leaves no truncated
scene.

load_ply ACCEPTS FOREIGN FILES: it finds the required properties by name in any order, ignores other float properties
(``nx ny nz`` may be absent, extra ones present), ignores elements after ``vertex``, and derives K from the number of
``f_rest_*`` (3 (K - 1), K a supported square; none: K = 1).

Checks, each a ValueError before anything is written or launched.  save_ply / pack_ply_rows: a missing key, wrong shapes,
unequal N, N == 0, tensors on different devices, a K that is no supported square; for backend="hip" also non-float32 or
non-contiguous tensors and CPU tensors.  load_ply / parse_ply_header: an ``ascii`` or big-endian file, a vertex property whose
type is not ``float`` / ``float32`` (both backends), a missing required property, duplicate property names, an unsupported K,
an element before ``vertex``, a body shorter than N rows; for backend="hip" also more than 192 float properties per vertex
(MS_PLY_MAX_STRIDE: 64 rows of them are staged in LDS).

The ``.splat`` and compressed-PLY formats of the web viewers: ``splatio.py``.  Not covered: ascii and big-endian files, non-float properties, extra per-Gaussian
tensors and optimiser moments (``torch.save(opt.state_dict())`` does the latter), float16 parameters, writing in Morton order
(``prepare_scene`` orders a scene), the sharded trainer.
"""
import ctypes
import os
import sys
from typing import NamedTuple, Tuple

import numpy as np
import torch

from .knn import SH_C0

TENSORS = ("means3d", "scales", "quats", "opacities", "features")          # the order of ms_ply_pack's tensor array
_FIXED = {"x": (0, 0), "y": (0, 1), "z": (0, 2), "scale_0": (1, 0), "scale_1": (1, 1), "scale_2": (1, 2),
          "rot_0": (2, 0), "rot_1": (2, 1), "rot_2": (2, 2), "rot_3": (2, 3), "opacity": (3, 0),
          "f_dc_0": (4, 0), "f_dc_1": (4, 1), "f_dc_2": (4, 2)}
_HEADER_LIMIT = 1 << 20          # a header is a few kilobytes; a file with no end_header in its first MiB is not a PLY file


class PlyLayout(NamedTuple):
    """What a header says: ``n`` vertices; ``columns``, the vertex element's property names in file order (a row is
    ``len(columns)`` float32); ``K`` SH coefficients per channel; ``body_offset``, the header's length in bytes."""
    n: int
    columns: Tuple[str, ...]
    K: int
    body_offset: int


def _supported_K():
    from .sh import MAX_SH_DEGREE
    return tuple((d + 1) ** 2 for d in range(MAX_SH_DEGREE + 1))


def property_names(K):
    """The property names of a file this module writes, in order."""
    return ("x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2") + tuple(f"f_rest_{i}" for i in range(3 * (K - 1))) + \
        ("opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3")


def ply_header(N, K) -> bytes:
    """The exact header bytes of a file of N Gaussians with K SH coefficients per channel (module docstring)."""
    if not (isinstance(N, int) and not isinstance(N, bool) and N >= 1):
        raise ValueError(f"N must be a positive int, got {N!r}")
    if K not in _supported_K():
        raise ValueError(f"K = {K!r} is not a supported number of SH coefficients {_supported_K()}")
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {N}"] + [f"property float {p}" for p in property_names(K)] + \
        ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def column_map(columns):
    """``columns``: a row's property names in file order -> (K, [(tensor, offset) or None per column]); tensor indexes
    TENSORS, offset is the float within that tensor's row (features' row: (K, 3) flattened).  ValueError: duplicate names, a
    missing required property, ``f_rest_*`` that are not 0 .. 3 (K - 1) - 1 for a supported K."""
    columns = tuple(columns)
    if len(set(columns)) != len(columns):
        dup = sorted({c for c in columns if columns.count(c) > 1})
        raise ValueError(f"duplicate property names: {dup}")
    missing = [p for p in _FIXED if p not in columns]
    if missing:
        raise ValueError(f"missing required properties: {missing}")
    rest = [c for c in columns if c.startswith("f_rest_")]
    n_rest = len(rest)
    K = n_rest // 3 + 1
    if n_rest % 3 or K not in _supported_K():
        raise ValueError(f"{n_rest} f_rest_* properties: 3 (K - 1) with K one of {_supported_K()} is required")
    missing = [f"f_rest_{i}" for i in range(n_rest) if f"f_rest_{i}" not in columns]
    if missing:
        raise ValueError(f"missing required properties: {missing[:4]}{' ...' if len(missing) > 4 else ''}")
    out = []
    for c in columns:
        if c in _FIXED:
            out.append(_FIXED[c])
        elif c.startswith("f_rest_"):
            ch, k = divmod(int(c[7:]), K - 1)                      # f_rest_{ch (K - 1) + (k - 1)} = features[n, k, ch]
            out.append((4, (k + 1) * 3 + ch))
        else:
            out.append(None)
    return K, out


def parse_ply_header(data: bytes) -> PlyLayout:
    """The inverse of ``ply_header`` on the first bytes of a file (more may follow the header), foreign headers included:
    comments and ``obj_info`` lines are skipped, elements after ``vertex`` ignored.  ValueError: module docstring."""
    end = data.find(b"end_header")
    nl = data.find(b"\n", end) if end >= 0 else -1
    if not data.startswith(b"ply") or nl < 0:
        raise ValueError("not a PLY file: no 'ply' ... 'end_header' in its first bytes")
    try:
        lines = [ln.strip() for ln in data[:end].decode("ascii").splitlines()]
    except UnicodeDecodeError:
        raise ValueError("not a PLY file: the header is not ascii") from None
    if lines[0] != "ply":
        raise ValueError("not a PLY file: the first line is not 'ply'")
    fmt = None
    n = None
    columns = []
    in_vertex = False
    for ln in lines[1:]:
        w = ln.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1:]
        elif w[0] == "element":
            if len(w) != 3 or not w[2].isdigit():
                raise ValueError(f"malformed header line: {ln!r}")
            if n is None:
                if w[1] != "vertex":
                    raise ValueError(f"element {w[1]!r} comes before 'vertex': only files whose first element is the vertices are read")
                n, in_vertex = int(w[2]), True
            else:
                in_vertex = False                                   # later elements are ignored
        elif w[0] == "property":
            if n is None:
                raise ValueError(f"malformed header: {ln!r} before any element")
            if in_vertex:
                if len(w) != 3 or w[1] not in ("float", "float32"):
                    raise ValueError(f"vertex property {ln!r}: only 'float' / 'float32' properties are read")
                columns.append(w[2])
        else:
            raise ValueError(f"malformed header line: {ln!r}")
    if fmt != ["binary_little_endian", "1.0"]:
        raise ValueError(f"format {' '.join(fmt) if fmt else None!r}: only 'binary_little_endian 1.0' is read")
    if n is None:
        raise ValueError("no 'element vertex' in the header")
    K, _ = column_map(columns)
    return PlyLayout(n, tuple(columns), K, nl + 1)


# ---------------------------------------------------------------------------------------------------------------------------
# the row move

def _check_backend(backend):
    if backend not in ("hip", "torch"):
        raise ValueError(f"Invalid backend: {backend!r} (\"hip\" or \"torch\")")


def _check_space(opacity_space):
    if opacity_space not in ("linear", "logit"):
        raise ValueError(f"Invalid opacity_space: {opacity_space!r} (\"linear\" or \"logit\")")


def _validate_params(params, backend):
    """-> (N, K or None for (N, 3) RGB features, the five tensors detached).  Every check of the module docstring."""
    _check_backend(backend)
    missing = [k for k in TENSORS if k not in params]
    if missing:
        raise ValueError(f"params lacks {missing}")
    t = [params[k] for k in TENSORS]
    for k, x in zip(TENSORS, t):
        if not isinstance(x, torch.Tensor) or not x.is_floating_point():
            raise ValueError(f"params[{k!r}] must be a floating-point tensor")
    want = {"means3d": (3,), "scales": (3,), "quats": (4,), "opacities": ()}
    for k, x in zip(TENSORS[:4], t):
        if x.dim() != 1 + len(want[k]) or tuple(x.shape[1:]) != want[k]:
            raise ValueError(f"params[{k!r}] must have shape (N{''.join(f', {d}' for d in want[k])}), got {tuple(x.shape)}")
    f = t[4]
    if f.dim() == 2 and f.shape[1] == 3:
        K = None
    elif f.dim() == 3 and f.shape[2] == 3 and f.shape[1] in _supported_K():
        K = f.shape[1]
    else:
        raise ValueError(f"params['features'] must have shape (N, 3) or (N, K, 3) with K one of {_supported_K()}, got {tuple(f.shape)}")
    N = t[0].shape[0]
    if any(x.shape[0] != N for x in t):
        raise ValueError(f"the tensors' row counts differ: { {k: x.shape[0] for k, x in zip(TENSORS, t)} }")
    if N == 0:
        raise ValueError("an empty scene (N == 0) is not written")
    if any(x.device != t[0].device for x in t):
        raise ValueError(f"the tensors are on different devices: { {k: str(x.device) for k, x in zip(TENSORS, t)} }")
    if backend == "hip":
        for k, x in zip(TENSORS, t):
            if x.dtype != torch.float32:
                raise ValueError(f"backend='hip': params[{k!r}] must be float32, got {x.dtype}")
            if not x.is_contiguous():
                raise ValueError(f"backend='hip': params[{k!r}] must be contiguous")
        if not t[0].is_cuda:
            raise ValueError("backend='hip': every tensor must be a CUDA/ROCm tensor (there is no fallback)")
    return N, K, [x.detach() for x in t]


def _sh_features(features, K):
    """(N, 3) RGB -> its degree-0 SH coefficients (N, 1, 3) (K is None); SH features as they are."""
    return features if K is not None else ((features - 0.5) / SH_C0).unsqueeze(1)


def _bits(x):
    return x.float().contiguous().view(torch.int32)          # (float() of a float32 tensor is the tensor itself)


def _pack_torch(t, N, K):
    cmap = column_map(property_names(K))[1]
    src = [_bits(x).reshape(N, -1) for x in t]
    rows = torch.zeros((N, len(cmap)), dtype=torch.int32, device=src[0].device)
    for k in range(len(TENSORS)):
        cols = [c for c, m in enumerate(cmap) if m is not None and m[0] == k]
        rows[:, cols] = src[k][:, [cmap[c][1] for c in cols]]
    return rows.view(torch.float32)


def _table(entries):
    from . import _hip
    tab = (_hip.PlyColumn * len(entries))()
    for i, (tensor, offset, column) in enumerate(entries):
        tab[i].tensor, tab[i].offset, tab[i].column = tensor, offset, column
    return tab


def _pack_hip(t, N, K):
    from . import _hip
    L = _hip.lib()
    dev = t[0].device
    cmap = column_map(property_names(K))[1]
    tab = _table([(_hip.PLY_NONE, 0, c) if m is None else (m[0], m[1], c) for c, m in enumerate(cmap)])
    widths = (ctypes.c_int * 5)(3, 3, 4, 1, 3 * K)
    ptrs = (ctypes.c_void_p * 5)(*[x.data_ptr() for x in t])
    rows = torch.empty((N, len(cmap)), dtype=torch.float32, device=dev)
    with _hip.on_device(dev):
        _hip.check(L.ms_ply_pack(N, len(cmap), ptrs, widths, tab, _hip.ptr(rows), _hip.stream(dev)), "ms_ply_pack")
    return rows


@torch.no_grad()
def pack_ply_rows_torch(params):
    """THE DEFINITION of the rows of a file's body (module docstring): (N, F) float32 on params' device, F = 14 + 3 K, moved as
    int32 so that every bit survives.  (N, 3) RGB features are converted to degree-0 SH first."""
    N, K, t = _validate_params(params, "torch")
    t[4] = _sh_features(t[4], K)
    return _pack_torch(t, N, K or 1)


@torch.no_grad()
def pack_ply_rows(params, *, backend="hip"):
    """The (N, F) float32 rows of the file body of ``params``, on params' device.  backend="torch": the definition.
    backend="hip": ms_ply_pack, one launch on the current stream, no host wait; CUDA/ROCm, float32, contiguous tensors; bit for
    bit the definition; no fallback."""
    N, K, t = _validate_params(params, backend)
    t[4] = _sh_features(t[4], K)                                   # (the same torch ops for both backends)
    return _pack_torch(t, N, K or 1) if backend == "torch" else _pack_hip(t, N, K or 1)


def _check_rows(rows, columns, backend):
    _check_backend(backend)
    columns = tuple(columns)
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape[1] != len(columns) or rows.dtype != torch.float32:
        raise ValueError(f"rows must be a float32 tensor of shape (N, {len(columns)}), one column per property")
    if rows.shape[0] == 0:
        raise ValueError("rows is empty (N == 0)")
    K, cmap = column_map(columns)
    if backend == "hip":
        from . import _hip
        if not rows.is_cuda:
            raise ValueError("backend='hip': rows must be a CUDA/ROCm tensor (there is no fallback)")
        if not rows.is_contiguous():
            raise ValueError("backend='hip': rows must be contiguous")
        if len(columns) > _hip.PLY_MAX_STRIDE:
            raise ValueError(f"backend='hip': {len(columns)} float properties per vertex, more than {_hip.PLY_MAX_STRIDE}")
    return K, cmap


def _shape(flat, K):
    means3d, scales, quats, opacities, features = flat
    return {"means3d": means3d, "scales": scales, "quats": quats, "opacities": opacities.reshape(-1),
            "features": features.reshape(-1, K, 3)}


def _unpack_torch(rows, K, cmap):
    N = rows.shape[0]
    src = rows.contiguous().view(torch.int32)
    widths = (3, 3, 4, 1, 3 * K)
    flat = []
    for k, w in enumerate(widths):
        col_of = {m[1]: c for c, m in enumerate(cmap) if m is not None and m[0] == k}
        flat.append(src[:, [col_of[o] for o in range(w)]].contiguous().view(torch.float32))
    return _shape(flat, K)


def _unpack_hip(rows, K, cmap, out=None):
    """``out``: the five (N, width) tensors to write into (tests: pre-filled, every element must be overwritten)."""
    from . import _hip
    L = _hip.lib()
    dev = rows.device
    N, S = rows.shape
    entries = [(m[0], m[1], c) for c, m in enumerate(cmap) if m is not None]
    tab = _table(entries)
    w = (3, 3, 4, 1, 3 * K)
    widths = (ctypes.c_int * 5)(*w)
    flat = [torch.empty((N, x), dtype=torch.float32, device=dev) for x in w] if out is None else list(out)
    ptrs = (ctypes.c_void_p * 5)(*[x.data_ptr() for x in flat])
    with _hip.on_device(dev):
        _hip.check(L.ms_ply_unpack(N, len(entries), S, _hip.ptr(rows), ptrs, widths, tab, _hip.stream(dev)), "ms_ply_unpack")
    return _shape(flat, K)


@torch.no_grad()
def unpack_ply_rows_torch(rows, columns):
    """THE DEFINITION of the inverse: ``rows`` (N, S) float32, ``columns`` the S property names of a row in file order (a parsed
    header's) -> the five tensors, float32 and contiguous, features (N, K, 3).  Columns of other names are ignored."""
    K, cmap = _check_rows(rows, columns, "torch")
    return _unpack_torch(rows, K, cmap)


@torch.no_grad()
def unpack_ply_rows(rows, columns, *, backend="hip"):
    """The inverse of ``pack_ply_rows`` for rows whose columns are named ``columns`` (any order, extra columns ignored).
    backend="torch": the definition.  backend="hip": ms_ply_unpack, one launch on the current stream, no host wait; rows a
    CUDA/ROCm, contiguous tensor of at most 192 columns; bit for bit the definition; no fallback."""
    K, cmap = _check_rows(rows, columns, backend)
    return _unpack_torch(rows, K, cmap) if backend == "torch" else _unpack_hip(rows, K, cmap)


# ---------------------------------------------------------------------------------------------------------------------------
# files

def _little_endian(a):
    return a if sys.byteorder == "little" else a.byteswap()


def save_ply(path, params, *, opacity_space="logit", backend="hip") -> int:
    """Write ``params`` to ``path`` in the layout of the module docstring -> the bytes written.  opacity_space: what
    params["opacities"] holds ("linear": its logit is stored).  The tensors are not changed.  backend="hip": the rows are packed
    on the device and copied once to pinned host memory -- ONE DEVICE-TO-HOST WAIT, inherent; no fallback."""
    _check_space(opacity_space)
    N, K, t = _validate_params(params, backend)
    path = os.fspath(path)
    with torch.no_grad():
        t[4] = _sh_features(t[4], K)
        if opacity_space == "linear":
            t[3] = torch.log(t[3]) - torch.log1p(-t[3])
        if backend == "torch":
            host = _pack_torch(t, N, K or 1).cpu()
        else:
            rows = _pack_hip(t, N, K or 1)
            host = torch.empty(rows.shape, dtype=torch.float32, pin_memory=True)
            host.copy_(rows)                                       # (the one wait)
    header = ply_header(N, K or 1)
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(header)
            f.write(memoryview(_little_endian(host.numpy())).cast("B"))
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return len(header) + host.numel() * 4


def load_ply(path, *, device=None, opacity_space="logit", requires_grad=False, backend="hip") -> dict:
    """Read the scene in ``path`` (this module's files and foreign ones: module docstring) -> the params dict: float32,
    contiguous leaf tensors on ``device`` (default: the current CUDA/ROCm device for backend="hip", the CPU for "torch") with
    ``requires_grad`` as given; features always (N, K, 3).  opacity_space: what the returned "opacities" hold ("linear": the
    sigmoid of the stored logit).  backend="hip": the body is read into a pinned host buffer, copied to the device once --
    ONE WAIT, inherent -- and unpacked by ms_ply_unpack; no fallback."""
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
    lay = parse_ply_header(head)
    N, S = lay.n, len(lay.columns)
    if N == 0:
        raise ValueError(f"{path}: the file holds no Gaussian (element vertex 0)")
    if os.path.getsize(path) < lay.body_offset + N * S * 4:
        raise ValueError(f"{path}: the body is shorter than {N} rows of {S} float32 "
                         f"({os.path.getsize(path) - lay.body_offset} of {N * S * 4} bytes)")
    if backend == "torch":
        dev = torch.device("cpu" if device is None else device)
        body = np.fromfile(path, dtype="<f4", count=N * S, offset=lay.body_offset).reshape(N, S)
        rows = torch.from_numpy(body.astype(np.float32, copy=False)).to(dev)
        K, cmap = _check_rows(rows, lay.columns, backend)
        out = _unpack_torch(rows, K, cmap)
    else:
        from . import _hip
        _hip.lib()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"backend='hip': device must be a CUDA/ROCm device, got {dev} (there is no fallback)")
        if S > _hip.PLY_MAX_STRIDE:
            raise ValueError(f"backend='hip': {S} float properties per vertex, more than {_hip.PLY_MAX_STRIDE}")
        host = torch.empty((N, S), dtype=torch.float32, pin_memory=True)
        buf = host.numpy()
        with open(path, "rb") as f:
            f.seek(lay.body_offset)
            if f.readinto(memoryview(buf).cast("B")) != N * S * 4:
                raise ValueError(f"{path}: the body is shorter than {N} rows of {S} float32")
        if sys.byteorder != "little":
            buf.byteswap(inplace=True)
        rows = host.to(dev)                                        # (the one wait)
        K, cmap = _check_rows(rows, lay.columns, backend)
        out = _unpack_hip(rows, K, cmap)
    with torch.no_grad():
        if opacity_space == "linear":
            out["opacities"] = torch.sigmoid(out["opacities"])
    return {k: x.contiguous().requires_grad_(bool(requires_grad)) for k, x in out.items()}


__all__ = ["save_ply", "load_ply", "pack_ply_rows", "unpack_ply_rows", "pack_ply_rows_torch", "unpack_ply_rows_torch",
           "ply_header", "parse_ply_header", "PlyLayout", "property_names", "column_map"]
