"""CPU: 3DGS PLY scene files (mojosplat_amd/sceneio.py) -- the header, the file layout against an independent numpy writer,
bit-exact and one-rounding round trips, foreign layouts, every ValueError, and the argument checks of ms_ply_pack /
ms_ply_unpack through the C ABI (no compute)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mojosplat_amd as ms
from mojosplat_amd import _hip
from mojosplat_amd.knn import SH_C0
from mojosplat_amd.sceneio import (PlyLayout, load_ply, pack_ply_rows, pack_ply_rows_torch, parse_ply_header, ply_header,
                                   property_names, save_ply, unpack_ply_rows, unpack_ply_rows_torch)

KS = (1, 4, 9, 16)
KEYS = ("means3d", "scales", "quats", "opacities", "features")

HEADER_5_16 = b"""ply
format binary_little_endian 1.0
element vertex 5
property float x
property float y
property float z
property float nx
property float ny
property float nz
property float f_dc_0
property float f_dc_1
property float f_dc_2
property float f_rest_0
property float f_rest_1
property float f_rest_2
property float f_rest_3
property float f_rest_4
property float f_rest_5
property float f_rest_6
property float f_rest_7
property float f_rest_8
property float f_rest_9
property float f_rest_10
property float f_rest_11
property float f_rest_12
property float f_rest_13
property float f_rest_14
property float f_rest_15
property float f_rest_16
property float f_rest_17
property float f_rest_18
property float f_rest_19
property float f_rest_20
property float f_rest_21
property float f_rest_22
property float f_rest_23
property float f_rest_24
property float f_rest_25
property float f_rest_26
property float f_rest_27
property float f_rest_28
property float f_rest_29
property float f_rest_30
property float f_rest_31
property float f_rest_32
property float f_rest_33
property float f_rest_34
property float f_rest_35
property float f_rest_36
property float f_rest_37
property float f_rest_38
property float f_rest_39
property float f_rest_40
property float f_rest_41
property float f_rest_42
property float f_rest_43
property float f_rest_44
property float opacity
property float scale_0
property float scale_1
property float scale_2
property float rot_0
property float rot_1
property float rot_2
property float rot_3
end_header
"""


def scene(N, K, seed=0, rgb=False):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g)
    return {"means3d": r(N, 3), "scales": r(N, 3) - 3.0, "quats": r(N, 4), "opacities": r(N),
            "features": torch.rand((N, 3), generator=g) if rgb else r(N, K, 3)}


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return all(a[k].shape == b[k].shape and torch.equal(bits(a[k]), bits(b[k])) for k in KEYS)


def numpy_file(p, K):
    """An independent writer: a numpy structured array, one explicit assignment per property."""
    N = p["means3d"].shape[0]
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(3 * (K - 1))] + \
        ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    a = np.zeros(N, dtype=[(n, "<f4") for n in names])
    m, s, q, o, f = (p[k].numpy() for k in KEYS)
    a["x"], a["y"], a["z"] = m[:, 0], m[:, 1], m[:, 2]
    for c in range(3):
        a[f"f_dc_{c}"] = f[:, 0, c]
        for k in range(1, K):
            a[f"f_rest_{c * (K - 1) + (k - 1)}"] = f[:, k, c]
        a[f"scale_{c}"] = s[:, c]
    a["opacity"] = o
    for i in range(4):
        a[f"rot_{i}"] = q[:, i]
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % N + "".join(f"property float {n}\n" for n in names) + \
        "end_header\n"
    return head.encode() + a.tobytes()


def test_header_is_pinned_and_parses_back():
    assert ply_header(5, 16) == HEADER_5_16
    lay = parse_ply_header(HEADER_5_16 + b"\x00" * 40)
    assert lay == PlyLayout(5, property_names(16), 16, len(HEADER_5_16))
    assert len(lay.columns) == 14 + 3 * 16
    for K in KS + (25,):
        h = ply_header(7, K)
        assert parse_ply_header(h) == PlyLayout(7, property_names(K), K, len(h))
    assert ms.ply_header is ply_header and ms.save_ply is save_ply and ms.load_ply is load_ply
    assert ms.pack_ply_rows is pack_ply_rows and ms.unpack_ply_rows is unpack_ply_rows


@pytest.mark.parametrize("K", KS)
def test_saved_file_equals_an_independent_numpy_writer(tmp_path, K):
    p = scene(37, K, seed=K)
    path = str(tmp_path / "a.ply")
    n = save_ply(path, p, backend="torch")
    data = open(path, "rb").read()
    assert n == len(data) == len(ply_header(37, K)) + 37 * (14 + 3 * K) * 4
    assert data == numpy_file(p, K)
    assert not os.path.exists(path + ".tmp")


def _plant(t, seed):
    """Special bit patterns in every tensor: quiet and signalling NaNs with payloads, both infinities, -0.0, denormals."""
    special = torch.from_numpy(np.array([0x7FC00001, 0x7F800001, 0xFFFFFFFF, 0xFFA5A5A5, 0x7F800000, 0xFF800000, 0x80000000,
                                         0x00000001, 0x80000001, 0x007FFFFF], dtype=np.uint32).view(np.int32))
    flat = t.view(torch.int32).reshape(-1)
    idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(seed))[:special.numel()]
    flat[idx] = special[:len(idx)]


@pytest.mark.parametrize("K", KS)
def test_logit_sh_round_trip_is_bit_exact(tmp_path, K):
    p = scene(41, K, seed=10 + K)
    for i, k in enumerate(KEYS):
        _plant(p[k], i)
    assert any(torch.isnan(p[k]).any() for k in KEYS)
    before = {k: v.clone() for k, v in p.items()}
    path = tmp_path / "rt.ply"                           # (a os.PathLike)
    save_ply(path, p, backend="torch")
    got = load_ply(path, backend="torch")
    assert same_bits(got, p) and same_bits(p, before)
    for k in KEYS:
        assert got[k].dtype == torch.float32 and got[k].is_contiguous() and got[k].is_leaf and not got[k].requires_grad
        assert got[k].device.type == "cpu"
    assert all(v.requires_grad and v.is_leaf for v in load_ply(path, backend="torch", requires_grad=True).values())
    rows = pack_ply_rows_torch(p)
    assert rows.shape == (41, 14 + 3 * K) and torch.equal(bits(rows), bits(pack_ply_rows(p, backend="torch")))
    assert torch.equal(bits(rows[:, 3:6]), torch.zeros((41, 3), dtype=torch.int32))          # +0.0, not -0.0
    assert same_bits(unpack_ply_rows_torch(rows, property_names(K)), p)
    assert same_bits(unpack_ply_rows(rows, property_names(K), backend="torch"), p)


def test_linear_opacity_and_rgb_round_trips_are_one_rounding_each_way(tmp_path):
    N = 200
    p = scene(N, 1, seed=3, rgb=True)
    p["opacities"] = torch.rand(N, generator=torch.Generator().manual_seed(4)) * 0.98 + 0.01
    path = str(tmp_path / "lin.ply")
    save_ply(path, p, opacity_space="linear", backend="torch")
    stored = load_ply(path, backend="torch")                     # the stored values, as they are
    o = p["opacities"].double()
    logit = torch.log(o) - torch.log1p(-o)
    # the stated formula in float32: log and log1p within one ulp each (relative 2^-23 of each term: the accuracy of a
    # vectorised libm), then the difference rounded once (relative 2^-24 of the result)
    eps = 2.0 ** -24
    tol = 2 * eps * (torch.log(o).abs() + torch.log1p(-o).abs()) + eps * logit.abs()
    assert bool(((stored["opacities"].double() - logit).abs() <= tol).all())
    assert torch.equal(stored["opacities"], torch.log(p["opacities"]) - torch.log1p(-p["opacities"]))
    rgb = p["features"].double()
    dc = (rgb - 0.5) / SH_C0
    assert stored["features"].shape == (N, 1, 3)
    # (the difference, SH_C0 as float32 and the quotient rounded once each; one more where the division is a multiplication
    # by the rounded reciprocal)
    assert bool(((stored["features"][:, 0].double() - dc).abs() <= 4 * eps * dc.abs() + 2.0 ** -149).all())
    assert torch.equal(stored["features"][:, 0], (p["features"] - 0.5) / SH_C0)
    lin = load_ply(path, opacity_space="linear", backend="torch")
    assert torch.equal(lin["opacities"], torch.sigmoid(stored["opacities"]))
    # back through sigmoid: the stored logit's error (|d sigmoid / dx| <= 1/4) and one ulp of a result below 1
    back_tol = 0.25 * tol + 2 * eps
    assert bool(((lin["opacities"].double() - o).abs() <= back_tol).all())
    for k in ("means3d", "scales", "quats"):
        assert torch.equal(bits(lin[k]), bits(p[k]))


def _foreign(p, K, names, extra_header="", tail_header="", fmt="binary_little_endian 1.0", typ="float"):
    """A file with the properties ``names`` in that order (names outside the layout get a fill value)."""
    N = p["means3d"].shape[0]
    own = np.frombuffer(numpy_file(p, K)[len(ply_header(N, K)):], dtype="<f4").reshape(N, -1)
    col = {n: i for i, n in enumerate(property_names(K))}
    body = np.stack([own[:, col[n]] if n in col else np.full(N, 7.25, dtype="<f4") for n in names], axis=1)
    head = f"ply\nformat {fmt}\n{extra_header}element vertex {N}\n" + "".join(f"property {typ} {n}\n" for n in names) + \
        tail_header + "end_header\n"
    return head.encode() + np.ascontiguousarray(body, dtype="<f4").tobytes()


@pytest.mark.parametrize("K", (1, 9))
def test_foreign_layouts_load_to_the_same_dict(tmp_path, K):
    p = scene(23, K, seed=20 + K)
    names = list(property_names(K))
    shuffled = [names[i] for i in torch.randperm(len(names), generator=torch.Generator().manual_seed(1)).tolist()]
    no_normals = [n for n in names if n not in ("nx", "ny", "nz")]
    extras = names[:8] + ["confidence", "semantic_id"] + names[8:]
    files = {"shuffled": _foreign(p, K, shuffled),
             "no_normals": _foreign(p, K, no_normals),
             "extras": _foreign(p, K, extras),
             "face": _foreign(p, K, names, tail_header="element face 0\nproperty list uchar int vertex_indices\n"),
             "comment": _foreign(p, K, names, extra_header="comment written by another tool\nobj_info whatever\n"),
             "float32": _foreign(p, K, names, typ="float32")}
    for tag, data in files.items():
        path = str(tmp_path / f"{tag}.ply")
        open(path, "wb").write(data)
        got = load_ply(path, backend="torch")
        assert same_bits(got, p), tag
    lay = parse_ply_header(files["extras"])
    assert lay.columns == tuple(extras) and lay.K == K and lay.n == 23


def _raises(tmp_path, data, match):
    path = str(tmp_path / "bad.ply")
    open(path, "wb").write(data)
    with pytest.raises(ValueError, match=match):
        load_ply(path, backend="torch")
    if "end_header" in data.decode("latin1"):
        with pytest.raises(ValueError, match=match):
            load_ply(path, backend="hip")                # the file's checks come before the backend is touched


def test_load_ply_rejects_bad_files(tmp_path):
    K = 4
    p = scene(9, K, seed=5)
    names = list(property_names(K))
    _raises(tmp_path, _foreign(p, K, names, fmt="ascii 1.0"), "binary_little_endian")
    _raises(tmp_path, _foreign(p, K, names, fmt="binary_big_endian 1.0"), "binary_little_endian")
    _raises(tmp_path, _foreign(p, K, names, typ="double"), "float")
    _raises(tmp_path, _foreign(p, K, names, typ="uchar"), "float")
    _raises(tmp_path, _foreign(p, K, [n for n in names if n != "rot_2"]), "missing.*rot_2")
    _raises(tmp_path, _foreign(p, K, [n for n in names if n != "f_rest_4"] + ["f_rest_9"]), "missing.*f_rest_4")
    _raises(tmp_path, _foreign(p, K, names + ["opacity"]), "duplicate.*opacity")
    _raises(tmp_path, _foreign(p, K, names[:-8 - 3] + names[-8:]), "f_rest")                       # 6 f_rest: K = 3 is no square
    _raises(tmp_path, _foreign(p, K, names + [f"f_rest_{i}" for i in range(9, 15)]), "f_rest")    # 15 f_rest: K = 6
    _raises(tmp_path, _foreign(p, K, names)[:-4], "shorter")
    _raises(tmp_path, _foreign(p, K, names, extra_header="element camera 1\nproperty float fov\n"), "before 'vertex'")
    _raises(tmp_path, b"plyformat", "not a PLY")
    with pytest.raises(ValueError, match="opacity_space"):
        load_ply(str(tmp_path / "bad.ply"), opacity_space="prob", backend="torch")
    with pytest.raises(ValueError, match="Invalid backend"):
        load_ply(str(tmp_path / "bad.ply"), backend="nope")


def test_save_ply_rejects_bad_input_and_leaves_no_file(tmp_path):
    path = str(tmp_path / "never.ply")
    good = scene(6, 4)

    def bad(match, backend="torch", **change):
        p = dict(good)
        for k, v in change.items():
            if v is None:
                del p[k]
            else:
                p[k] = v
        with pytest.raises(ValueError, match=match):
            save_ply(path, p, backend=backend)
        with pytest.raises(ValueError, match=match):
            pack_ply_rows(p, backend=backend)
        assert not os.path.exists(path) and not os.path.exists(path + ".tmp")

    bad("lacks", quats=None)
    bad("shape", means3d=torch.zeros(6, 4))
    bad("shape", opacities=torch.zeros(6, 1))
    bad("shape", features=torch.zeros(6, 5, 3))                      # K = 5 is no supported square
    bad("shape", features=torch.zeros(6, 4, 2))
    bad("row counts", scales=torch.zeros(5, 3))
    bad("empty", **{k: v[:0] for k, v in good.items()})
    bad("floating", quats=torch.zeros(6, 4, dtype=torch.int32))
    bad("different devices", quats=torch.zeros(6, 4, device="meta"))
    # the HIP path: float32 and contiguous only, and no fallback for CPU tensors
    bad("float32", backend="hip", scales=good["scales"].double())
    bad("contiguous", backend="hip", quats=torch.zeros(4, 6).t())
    bad("CUDA/ROCm", backend="hip")
    with pytest.raises(ValueError, match="opacity_space"):
        save_ply(path, good, opacity_space="prob", backend="torch")
    with pytest.raises(ValueError, match="Invalid backend"):
        save_ply(path, good, backend="nope")
    assert not os.path.exists(path) and not os.path.exists(path + ".tmp")
    # a failure while writing leaves neither file
    with pytest.raises(OSError):
        save_ply(str(tmp_path / "no_such_dir" / "x.ply"), good, backend="torch")
    assert not os.path.exists(str(tmp_path / "no_such_dir"))
    # an existing scene survives a failed save
    save_ply(path, good, backend="torch")
    before = open(path, "rb").read()
    with pytest.raises(ValueError):
        save_ply(path, dict(good, scales=torch.zeros(5, 3)), backend="torch")
    assert open(path, "rb").read() == before and not os.path.exists(path + ".tmp")


def test_unpack_rejects_bad_rows():
    rows = torch.zeros(3, 14 + 3)
    with pytest.raises(ValueError, match="shape"):
        unpack_ply_rows(rows, property_names(4), backend="torch")
    with pytest.raises(ValueError, match="shape"):
        unpack_ply_rows(rows.double(), property_names(1), backend="torch")
    with pytest.raises(ValueError, match="empty"):
        unpack_ply_rows(rows[:0], property_names(1), backend="torch")
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        unpack_ply_rows(rows, property_names(1), backend="hip")


def test_c_abi_argument_validation_of_the_ply_entry_points():
    """ms_ply_pack / ms_ply_unpack validate before they touch the device and report through the status code and
    ms_last_error_string.  Pointers are fake but non-null; nothing is dereferenced on these paths."""
    L = _hip.load()
    OK, INVALID = 0, 1
    err = lambda: L.ms_last_error_string().decode()
    P = ctypes.c_void_p(0x1000)
    N = ctypes.c_int64(10)
    K = 4
    F = 14 + 3 * K
    widths = (ctypes.c_int * 5)(3, 3, 4, 1, 3 * K)
    ptrs = (ctypes.c_void_p * 5)(*[0x1000 * (i + 1) for i in range(5)])
    holed = (ctypes.c_void_p * 5)(0x1000, 0x2000, None, 0x4000, 0x5000)
    from mojosplat_amd.sceneio import _table, column_map
    cmap = column_map(property_names(K))[1]
    pack_tab = lambda: _table([(-1, 0, c) if m is None else (m[0], m[1], c) for c, m in enumerate(cmap)])
    unpack_tab = lambda: _table([(m[0], m[1], c) for c, m in enumerate(cmap) if m is not None])
    Fu = F - 3
    big = _table([(-1, 0, c) for c in range(129)])

    assert L.ms_ply_pack(ctypes.c_int64(-1), F, ptrs, widths, pack_tab(), P, None) == INVALID and "N < 0" in err()
    assert L.ms_ply_unpack(ctypes.c_int64(-1), Fu, F, P, ptrs, widths, unpack_tab(), None) == INVALID and "N < 0" in err()
    assert L.ms_ply_pack(ctypes.c_int64(0), F, None, None, None, None, None) == OK                 # N == 0 is a no-op
    assert L.ms_ply_unpack(ctypes.c_int64(0), Fu, F, None, None, None, None, None) == OK
    assert L.ms_ply_pack(N, F, ptrs, widths, pack_tab(), None, None) == INVALID and "null" in err()
    assert L.ms_ply_pack(N, F, holed, widths, pack_tab(), P, None) == INVALID and "null" in err() and "tensor 2" in err()
    assert L.ms_ply_unpack(N, Fu, F, None, ptrs, widths, unpack_tab(), None) == INVALID and "null" in err()
    assert L.ms_ply_unpack(N, Fu, F, P, holed, widths, unpack_tab(), None) == INVALID and "null" in err()
    assert L.ms_ply_pack(N, 129, ptrs, widths, big, P, None) == INVALID and "F = 129" in err()
    assert L.ms_ply_unpack(N, 129, 150, P, ptrs, widths, big, None) == INVALID and "F = 129" in err()
    assert L.ms_ply_pack(N, 0, ptrs, widths, big, P, None) == INVALID and "F = 0" in err()
    assert L.ms_ply_unpack(N, Fu, Fu - 1, P, ptrs, widths, unpack_tab(), None) == INVALID and "S = " in err()
    assert L.ms_ply_unpack(N, Fu, 193, P, ptrs, widths, unpack_tab(), None) == INVALID and "S = 193" in err()
    t = pack_tab()
    t[0].offset = 3                                        # means3d's row is 3 floats wide
    assert L.ms_ply_pack(N, F, ptrs, widths, t, P, None) == INVALID and "offset 3" in err() and "width 3" in err()
    t = unpack_tab()
    t[Fu - 1].offset = 4                                   # rot_3 -> quats[4]
    assert L.ms_ply_unpack(N, Fu, F, P, ptrs, widths, t, None) == INVALID and "offset 4" in err() and "width 4" in err()
    t = pack_tab()
    t[1].tensor = 5
    assert L.ms_ply_pack(N, F, ptrs, widths, t, P, None) == INVALID and "tensor 5" in err()
    t = pack_tab()
    t[2].column = 1                                        # column 1 twice, column 2 never
    assert L.ms_ply_pack(N, F, ptrs, widths, t, P, None) == INVALID and "twice" in err()
    t = unpack_tab()
    t[0].column = F
    assert L.ms_ply_unpack(N, Fu, F, P, ptrs, widths, t, None) == INVALID and "column" in err()
    t = unpack_tab()
    t[1].offset = 0                                        # means3d[0] twice, means3d[1] never: an output float left unwritten
    assert L.ms_ply_unpack(N, Fu, F, P, ptrs, widths, t, None) == INVALID and "twice" in err()
    t = unpack_tab()
    t[1].tensor = -1
    assert L.ms_ply_unpack(N, Fu, F, P, ptrs, widths, t, None) == INVALID and "every one needs a column" in err()
    wide = (ctypes.c_int * 5)(3, 3, 4, 1, 120)
    assert L.ms_ply_pack(N, F, ptrs, wide, pack_tab(), P, None) == INVALID and "more than 128" in err()
    assert L.ms_ply_pack(N, F, ptrs, (ctypes.c_int * 5)(3, 0, 4, 1, 12), pack_tab(), P, None) == INVALID and "wide" in err()
    assert _hip.PLY_ROWS == 64 and _hip.PLY_MAX_COLUMNS == 128
