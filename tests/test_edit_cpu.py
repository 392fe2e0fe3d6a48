"""No GPU: scene editing (mojosplat_amd/edit.py) with backend="torch", the definition.  The SH band matrices (identity,
orthogonality, composition, a hand pin); what a transform must leave invariant, in float64 -- view-dependent colour under
the transformed camera, covariances, projections, the inverse round trip; the float32 definition against float64 inside
bounds derived from the roundings, and bit for bit against a SCALAR restatement held in this file (numpy.float32, one
operation at a time) on rows of NaN, Inf, -0.0 and denormals; every ValueError; crop and merge; the C entry's argument checks."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import mojosplat_amd as ms
from mojosplat_amd import _hip, edit
from mojosplat_amd.knn import SH_C0
from mojosplat_amd.projection import _rotmat
from mojosplat_amd.sh import evaluate_sh_torch
from edit_cases import (DENORMAL, KEYS, KS, MAPS, ROT_Z90, ROW_DENORMAL, ROW_NAN, ROW_NEGZERO, ROW_NINF, ROW_PINF, as_matrix,
                        random_rotation, rot_z, same_bits, same_scene, seeded_scene, special_scene)

F = np.float32
F64 = torch.float64
EPS = 2.0 ** -24


def camera64(seed=0, W=64, H=48):
    """A float64 camera about 6 units from the origin, looking at it."""
    eye = 6.0 * torch.nn.functional.normalize(torch.tensor([0.4, -0.3, 1.0], dtype=F64) + 0.1 * seed, dim=0)
    vm = ms.look_at(eye, torch.zeros(3), torch.tensor([0.0, 1.0, 0.0])).to(F64)
    fwd = -eye / eye.norm()                                           # (look_at works in float32: rebuild the rows in float64)
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 1.0, 0.0], dtype=F64))
    right = right / right.norm()
    Rv = torch.stack([right, torch.linalg.cross(right, fwd), fwd])
    assert float((Rv - vm[:3, :3]).abs().max()) < 1e-6
    return ms.Camera(R=Rv, T=-(Rv @ eye), H=H, W=W, fx=60.0, fy=55.0, cx=W / 2 + 1.5, cy=H / 2 - 2.0)


# ---------------------------------------------------------------------------------------------------------------------------
# the band matrices

def test_sh_rotation_matrices_identity_orthogonality_and_composition():
    eye = ms.sh_rotation_matrices(torch.eye(3), 4)
    R1, R2 = random_rotation(1), random_rotation(2)
    M1, M2, M12 = (ms.sh_rotation_matrices(R, 4) for R in (R1, R2, R1 @ R2))
    assert len(eye) == 4 and ms.sh_rotation_matrices(R1, 0) == []
    for l in range(1, 5):
        n = 2 * l + 1
        I = torch.eye(n, dtype=F64)
        assert eye[l - 1].shape == (n, n) and eye[l - 1].dtype == F64
        err = (float((eye[l - 1] - I).abs().max()), float((M1[l - 1] @ M1[l - 1].T - I).abs().max()),
               float((M12[l - 1] - M1[l - 1] @ M2[l - 1]).abs().max()))
        print(f"band {l}: identity {err[0]:.2e}, orthogonality {err[1]:.2e}, composition {err[2]:.2e}")
        assert max(err) <= 1e-12


def test_sh_rotation_matrix_of_a_quarter_turn_about_z_by_hand():
    (M1,) = ms.sh_rotation_matrices(ROT_Z90.tolist(), 1)
    want = torch.tensor([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]], dtype=F64)
    assert float((M1 - want).abs().max()) <= 1e-12
    with pytest.raises(ValueError, match="degree"):
        ms.sh_rotation_matrices(ROT_Z90, 5)
    with pytest.raises(ValueError, match="3x3"):
        ms.sh_rotation_matrices(torch.eye(4), 1)


# ---------------------------------------------------------------------------------------------------------------------------
# invariants, float64

SIMILARITIES = [dict(rotation=random_rotation(s), scale=sc, translation=t)
                for s, sc, t in ((3, 1.0, None), (4, 0.4, [1.0, -2.0, 0.5]), (5, 2.5, [-0.7, 0.2, 3.0]))]


@pytest.mark.parametrize("degree", range(5))
def test_colour_is_invariant_under_the_transformed_camera(degree):
    K = (degree + 1) ** 2
    p = seeded_scene(200, K, seed=degree, dtype=F64)
    cam = camera64(degree)
    want = evaluate_sh_torch(p["means3d"], p["features"], cam, degree, clamp=False)
    scale = float(p["features"].abs().max())
    for kw in SIMILARITIES:
        q = ms.transform_scene(p, backend="torch", **kw)
        got = evaluate_sh_torch(q["means3d"], q["features"], ms.transform_camera(cam, **kw), degree, clamp=False)
        err = float((got - want).abs().max())
        print(f"degree {degree}, s = {kw['scale']}: colour error {err:.2e} (max |c| = {scale:.2f})")
        assert err <= 1e-9 * scale
        if degree >= 1:                                               # ... and leaving the coefficients alone is wrong
            stale = evaluate_sh_torch(q["means3d"], p["features"], ms.transform_camera(cam, **kw), degree, clamp=False)
            assert float((stale - want).abs().max()) > 1e-3 * scale


def test_covariances_rotate_and_scale():
    p = seeded_scene(100, 1, seed=1, dtype=F64)

    def cov(x):
        M = _rotmat(x["quats"]) * torch.exp(x["scales"])[:, None, :]
        return M @ M.transpose(1, 2)

    for kw in SIMILARITIES:
        q = ms.transform_scene(p, backend="torch", **kw)
        R, s = kw["rotation"], kw["scale"]
        want = s * s * (R @ cov(p) @ R.T)
        rel = float(((cov(q) - want).abs().amax((1, 2)) / want.abs().amax((1, 2))).max())
        print(f"s = {s}: covariance error {rel:.2e} relative")
        assert rel <= 1e-9
        assert torch.equal(q["opacities"], p["opacities"]) and q["opacities"].data_ptr() != p["opacities"].data_ptr()


def test_a_transform_and_its_inverse_return_the_scene():
    p = seeded_scene(100, 16, seed=2, dtype=F64)
    p["quats"] = torch.nn.functional.normalize(p["quats"], dim=1)
    for kw in SIMILARITIES:
        m = as_matrix(**kw)
        inv = torch.linalg.inv(m)
        inv[3] = torch.tensor([0.0, 0.0, 0.0, 1.0])                   # (the numerical inverse leaves 1e-17 there: refused, rightly)
        with pytest.raises(ValueError, match="last row"):
            ms.transform_scene(p, torch.linalg.inv(m) + 1e-12 * torch.ones(4, 4), backend="torch")
        back = ms.transform_scene(ms.transform_scene(p, m, backend="torch"), inv, backend="torch")
        for k in KEYS:
            a, b = back[k], p[k]
            if k == "quats":                                          # q and -q are one rotation
                a = a * torch.sign((a * b).sum(1, keepdim=True))
            err = float((a - b).abs().max() / b.abs().max())
            print(f"s = {kw['scale']}: {k} round trip {err:.2e}")
            assert err <= 1e-9


def test_the_transformed_camera_projects_the_transformed_scene_alike():
    p = seeded_scene(100, 1, seed=3, dtype=F64)
    p["means3d"] = 0.5 * p["means3d"]                                # inside the view of a camera 6 units away
    cam = camera64(1)
    m2, con, z, _ = ms.project_gaussians(p["means3d"], p["scales"], p["quats"], p["opacities"], cam, backend="torch")
    assert float(z.min()) > 1.0
    for kw in SIMILARITIES:
        q = ms.transform_scene(p, backend="torch", **kw)
        cam2 = ms.transform_camera(cam, as_matrix(**kw))
        assert (cam2.H, cam2.W, cam2.fx, cam2.fy, cam2.cx, cam2.cy, cam2.near, cam2.far) == \
            (cam.H, cam.W, cam.fx, cam.fy, cam.cx, cam.cy, cam.near, cam.far) and cam2.view_matrix.dtype == F64
        m2b, conb, zb, _ = ms.project_gaussians(q["means3d"], q["scales"], q["quats"], q["opacities"], cam2, backend="torch")
        err = (float((m2b - m2).abs().max()), float((conb - con).abs().max() / con.abs().max()),
               float((zb - kw["scale"] * z).abs().max()))
        print(f"s = {kw['scale']}: means2d {err[0]:.2e}, conics {err[1]:.2e}, depths {err[2]:.2e}")
        assert max(err) <= 1e-8


# ---------------------------------------------------------------------------------------------------------------------------
# the float32 definition

@pytest.mark.parametrize("K", (4, 16, 25))
def test_float32_stays_within_its_roundings_of_float64(K):
    """features: a band's sum has at most 9 terms with |M| <= 1 and a row of M of norm 1, so sum |M c| <= 3 max |c|; an entry's
    rounding and a product's are 2 * 2^-24 of that, at most 8 sums add 2^-24 of a partial sum each: 30 * 2^-24 max |c| < 32.
    means: three products with a rounded entry (2 * 2^-24 each), three sums and t's own rounding on partial sums of at most
    s |x|_1 + |t_i|: 6 * 2^-24 < 8."""
    p32 = seeded_scene(300, K, seed=4)
    p64 = {k: v.double() for k, v in p32.items()}
    for kw in SIMILARITIES:
        a, b = ms.transform_scene(p32, backend="torch", **kw), ms.transform_scene(p64, backend="torch", **kw)
        assert all(v.dtype == torch.float32 for v in a.values()) and all(v.dtype == F64 for v in b.values())
        t = torch.zeros(3, dtype=F64) if kw["translation"] is None else torch.tensor(kw["translation"], dtype=F64)
        bound = 8 * EPS * (kw["scale"] * p64["means3d"].abs().sum(1, keepdim=True) + t.abs())
        err = (a["means3d"].double() - b["means3d"]).abs()
        print(f"K = {K}, s = {kw['scale']}: means error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        for l in range(1, math.isqrt(K)):
            band = slice(l * l, (l + 1) ** 2)
            bound = 32 * EPS * p64["features"][:, band].abs().amax(1, keepdim=True)
            err = (a["features"][:, band].double() - b["features"][:, band]).abs()
            print(f"   band {l}: features error / bound {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all())
        assert torch.equal(a["features"][:, 0], p32["features"][:, 0])


def spec_transform(p, c):
    """The formulas of the module docstring, one numpy.float32 operation at a time -> means, scales, quats, features."""
    A, t, r, l = [[F(v) for v in row] for row in c.A], [F(v) for v in c.t], [F(v) for v in c.r], F(c.l)
    M = [[[F(v) for v in row] for row in m] for m in c.M]
    means, scales, quats, feats = (p[k].numpy() for k in ("means3d", "scales", "quats", "features"))
    om, osc, oq, of = (np.array(x, copy=True) for x in (means, scales, quats, feats))
    for n in range(means.shape[0]):
        x, y, z = means[n]
        for i in range(3):
            om[n, i] = F(F(F(F(A[i][0] * x) + F(A[i][1] * y)) + F(A[i][2] * z)) + t[i])
            osc[n, i] = F(scales[n, i] + l)
        (rw, rx, ry, rz), (qw, qx, qy, qz) = r, quats[n]
        oq[n, 0] = F(F(F(F(rw * qw) - F(rx * qx)) - F(ry * qy)) - F(rz * qz))
        oq[n, 1] = F(F(F(F(rw * qx) + F(rx * qw)) + F(ry * qz)) - F(rz * qy))
        oq[n, 2] = F(F(F(F(rw * qy) - F(rx * qz)) + F(ry * qw)) + F(rz * qx))
        oq[n, 3] = F(F(F(F(rw * qz) + F(rx * qy)) - F(ry * qx)) + F(rz * qw))
        for li, m in enumerate(M, start=1):
            for ch in range(3):
                for row in range(2 * li + 1):
                    acc = F(m[row][0] * feats[n, li * li, ch])
                    for j in range(1, 2 * li + 1):
                        acc = F(acc + F(m[row][j] * feats[n, li * li + j, ch]))
                    of[n, li * li + row, ch] = acc
    return om, osc, oq, of


@pytest.mark.parametrize("K", KS)
def test_the_definition_equals_the_scalar_restatement_bit_for_bit(K):
    p = special_scene(K)
    assert math.isnan(float(p["means3d"][ROW_NAN, 1])) and float(p["scales"][ROW_PINF, 2]) == math.inf
    assert float(p["quats"][ROW_NINF, 0]) == -math.inf and math.copysign(1.0, float(p["means3d"][ROW_NEGZERO, 0])) == -1.0
    assert 0.0 < float(p["quats"][ROW_DENORMAL, 3]) < 2.0 ** -126
    for name, kw in MAPS.items():
        s, R, t = edit._similarity(None, kw.get("rotation"), kw.get("translation"), kw.get("scale", 1.0))
        c = edit._Constants(s, R, t, 0 if K is None else math.isqrt(K) - 1, single=True)
        with np.errstate(all="ignore"):
            want = spec_transform(p, c)
        got = ms.transform_scene(p, backend="torch", **kw)
        for k, w in zip(("means3d", "scales", "quats", "features"), want):
            assert np.array_equal(got[k].numpy().view(np.int32), w.view(np.int32)), (name, k)
        assert same_bits(got["opacities"], p["opacities"])
        finite_rows = [ROW_NEGZERO, ROW_DENORMAL]
        assert bool(torch.isfinite(got["features"][finite_rows]).all()) and not bool(torch.isfinite(got["means3d"][ROW_NAN]).all())
    # no map at all: A = I, r = (1, 0, 0, 0), l = 0 exactly -- the geometry comes back as it went in, denormals included (the
    # band matrices are least-squares results, the identity to 1e-15 only)
    same = ms.transform_scene(p, backend="torch")
    for k in KEYS[:4]:
        assert torch.equal(same[k][ROW_DENORMAL], p[k][ROW_DENORMAL]), k
    assert float(same["quats"][ROW_DENORMAL, 3]) == pytest.approx(DENORMAL, rel=1e-4)


def test_the_constants_are_rounded_once_from_float64():
    kw = MAPS["similarity"]
    s, R, t = edit._similarity(as_matrix(**kw), None, None, 1.0)
    assert s == pytest.approx(1.7, abs=1e-15) and float((R - kw["rotation"]).abs().max()) < 1e-15
    c32, c64 = edit._Constants(s, R, t, 2, single=True), edit._Constants(s, R, t, 2, single=False)
    assert c32.A == (s * R).float().double().tolist() and c32.l == float(F(math.log(s))) and c64.l == math.log(s)
    q = torch.tensor(c64.r, dtype=F64)
    assert float((_rotmat(q[None])[0] - R).abs().max()) < 1e-15 and q[0] > 0 and abs(float(q.norm()) - 1) < 1e-15
    # w >= 0; on w == 0 the first non-zero component is positive; every branch of the extraction
    for axis in ([1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [1.0, -1.0, 0.5], [-1.0, 0.2, 0.1]):
        a = torch.tensor(axis, dtype=F64)
        a = a / a.norm()
        for angle in (0.3, 2.0, 3.0, math.pi):
            Kx = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=F64)
            Rm = torch.eye(3, dtype=F64) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)
            q = torch.tensor(edit._quaternion(Rm), dtype=F64)
            assert float((_rotmat(q[None])[0] - Rm).abs().max()) < 1e-14 and float(q[0]) >= 0.0
            if angle == math.pi:
                lead = [v for v in q.tolist() if abs(v) > 1e-12][0]
                assert float(q[0]) < 1e-15 and (lead > 0 or float(q[0]) > 0)
    half_turn = edit._quaternion(torch.diag(torch.tensor([-1.0, -1.0, 1.0], dtype=F64)))
    assert half_turn == [0.0, 0.0, 0.0, 1.0] and all(math.copysign(1.0, v) == 1.0 for v in half_turn)


def test_outputs_are_new_contiguous_leaves():
    p = seeded_scene(10, 4)
    p["means3d"].requires_grad_(True)
    for K in (4, None):
        p = {**p, "features": seeded_scene(10, K)["features"]}
        out = ms.transform_scene(p, as_matrix(**MAPS["similarity"]).tolist(), backend="torch")
        again = ms.transform_scene(p, as_matrix(**MAPS["similarity"])[:3].numpy(), backend="torch", requires_grad=True)
        assert same_scene(out, again)
        for k in KEYS:
            assert out[k].is_leaf and not out[k].requires_grad and out[k].is_contiguous() and again[k].requires_grad
            assert out[k].shape == p[k].shape and out[k].untyped_storage().data_ptr() != p[k].untyped_storage().data_ptr()
        assert torch.equal(out["features"].reshape(10, -1, 3)[:, 0], p["features"].detach().reshape(10, -1, 3)[:, 0])


# ---------------------------------------------------------------------------------------------------------------------------
# ValueErrors

def test_every_value_error_is_raised_before_any_library_is_loaded(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(_hip, "load", no_library)
    monkeypatch.setattr(_hip, "lib", no_library)
    p = seeded_scene(8, 4)
    I = torch.eye(4, dtype=F64)

    def bad(match, *a, **kw):
        for backend in ("torch", "hip"):
            with pytest.raises(ValueError, match=match):
                ms.transform_scene(p, *a, backend=backend, **kw)
        with pytest.raises(ValueError, match=match):
            ms.transform_camera(camera64(), *a, **kw)

    shear = I.clone()
    shear[0, 1] = 0.1
    bad("uniform scale times a rotation", shear)
    bad("uniform scale times a rotation", torch.diag(torch.tensor([1.0, 2.0, 1.0, 1.0], dtype=F64)))
    bad("determinant", torch.diag(torch.tensor([1.0, 1.0, -1.0, 1.0], dtype=F64)))
    bad("determinant", rotation=torch.diag(torch.tensor([1.0, -1.0, 1.0])))
    last = I.clone()
    last[3, 0] = 1e-3
    bad("last row", last)
    last = I.clone()
    last[3, 3] = 2.0
    bad("last row", last)
    bad("determinant", torch.diag(torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=F64)))
    bad("finite and positive", scale=0.0)
    bad("finite and positive", scale=-1.0)
    bad("finite and positive", scale=math.inf)
    nan = I.clone()
    nan[1, 1] = math.nan
    bad("non-finite", nan)
    nan = I.clone()
    nan[0, 3] = math.nan
    bad("non-finite", nan)
    nan = torch.eye(3, dtype=F64)
    nan[2, 0] = math.nan
    bad("non-finite", rotation=nan)
    bad("three finite", translation=[0.0, math.inf, 0.0])
    bad("not both", I, scale=2.0)
    bad("not both", I, rotation=torch.eye(3))
    bad("not both", I, translation=[0.0, 0.0, 0.0])
    bad("4x4 or 3x4", torch.eye(3))
    bad("give the scale as scale=", rotation=2.0 * torch.eye(3))
    # a matrix typed in float32 is accepted, one off by 1e-4 is not
    ms.transform_scene(p, as_matrix(**MAPS["similarity"]).float(), backend="torch")
    off = as_matrix(**MAPS["similarity"])
    off[0, 0] += 1e-4
    bad("uniform scale times a rotation", off)
    # the params' checks are save_ply's
    with pytest.raises(ValueError, match="features"):
        ms.transform_scene({**p, "features": torch.zeros(8, 5, 3)}, backend="torch")
    with pytest.raises(ValueError, match="lacks"):
        ms.transform_scene({k: v for k, v in p.items() if k != "quats"}, backend="torch")
    with pytest.raises(ValueError, match="backend"):
        ms.transform_scene(p, backend="cuda")
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        ms.transform_scene(p, backend="hip")
    with pytest.raises(ValueError, match="float32"):
        ms.transform_scene({k: v.double() for k, v in p.items()}, backend="hip")
    with pytest.raises(ValueError, match="one dtype"):
        ms.transform_scene({**p, "scales": p["scales"].double()}, backend="torch")
    with pytest.raises(ValueError, match="one dtype"):
        ms.transform_scene({k: v.half() for k, v in p.items()}, backend="torch")


# ---------------------------------------------------------------------------------------------------------------------------
# crop and merge

def test_crop_scene():
    p = seeded_scene(12, 4, seed=5)
    p["means3d"] = torch.tensor([[0, 0, 0], [1, 1, 1], [1, 0, -1], [1.0001, 0, 0], [-1, -1, -1], [0, 2, 0], [math.nan, 0, 0],
                                 [0.5, -0.5, 0.25], [0, 0, math.nan], [-1.0001, 0, 0], [0, 0, 1], [3, 3, 3]], dtype=torch.float32)
    out, keep = ms.crop_scene(p, box=([-1, -1, -1], [1, 1, 1]))
    assert keep.dtype == torch.bool and keep.tolist() == [True, True, True, False, True, False, False, True, False, False, True, False]
    for k in KEYS:                                                    # rows in order, new leaves
        assert torch.equal(out[k], p[k][keep]) and out[k].is_leaf and out[k].is_contiguous() and not out[k].requires_grad
        assert out[k].untyped_storage().data_ptr() != p[k].untyped_storage().data_ptr()
    out, keep = ms.crop_scene(p, box=(torch.tensor([-1.0, -1, -1]), np.array([1.0, 1, 1])), invert=True, requires_grad=True)
    assert keep.tolist() == [False, False, False, True, False, True, False, False, False, True, False, True]       # NaN rows: dropped
    assert torch.equal(out["features"], p["features"][keep]) and out["scales"].requires_grad
    out, keep = ms.crop_scene(p, sphere=([0, 0, 0], 1.0))
    assert keep.tolist() == [True, False, False, False, False, False, False, True, False, False, True, False]       # |x| = 1: kept
    _, keep = ms.crop_scene(p, sphere=([0, 0, 0], 1.0), invert=True)
    assert keep.tolist() == [False, True, True, True, True, True, False, False, False, True, False, True]
    out, keep = ms.crop_scene(p, sphere=([9, 9, 9], 0.5))
    assert not keep.any() and out["features"].shape == (0, 4, 3) and out["opacities"].shape == (0,)
    with pytest.raises(ValueError, match="exactly one"):
        ms.crop_scene(p)
    with pytest.raises(ValueError, match="exactly one"):
        ms.crop_scene(p, box=([0, 0, 0], [1, 1, 1]), sphere=([0, 0, 0], 1.0))
    with pytest.raises(ValueError, match="radius"):
        ms.crop_scene(p, sphere=([0, 0, 0], -1.0))
    with pytest.raises(ValueError, match="three numbers"):
        ms.crop_scene(p, box=([0, 0], [1, 1, 1]))


def test_merge_scenes():
    a, b = seeded_scene(5, 4, seed=6), seeded_scene(3, 16, seed=7)
    m = ms.merge_scenes(a, b)
    assert m["features"].shape == (8, 16, 3) and torch.equal(m["features"][:5, :4], a["features"])
    assert not m["features"][:5, 4:].any() and torch.equal(m["features"][5:], b["features"])
    for k in KEYS[:4]:
        assert torch.equal(m[k], torch.cat([a[k], b[k]])) and m[k].is_leaf and m[k].is_contiguous()
    m = ms.merge_scenes(b, a, requires_grad=True)                     # the other way round pads the second
    assert torch.equal(m["features"][3:, :4], a["features"]) and not m["features"][3:, 4:].any() and m["quats"].requires_grad
    rgb = seeded_scene(4, None, seed=8)
    m = ms.merge_scenes(rgb, a)                                       # RGB meets SH: converted to degree 0, then padded
    assert m["features"].shape == (9, 4, 3) and torch.equal(m["features"][:4, 0], (rgb["features"] - 0.5) / SH_C0)
    assert not m["features"][:4, 1:].any() and torch.equal(m["features"][4:], a["features"])
    m = ms.merge_scenes(rgb, rgb)                                     # RGB with RGB stays RGB
    assert m["features"].shape == (8, 3) and torch.equal(m["features"][4:], rgb["features"])
    m = ms.merge_scenes(a, a)
    assert m["features"].shape == (10, 4, 3)
    with pytest.raises(ValueError, match="dtype"):
        ms.merge_scenes(a, {k: v.double() for k, v in b.items()})
    with pytest.raises(ValueError, match="lacks"):
        ms.merge_scenes(a, {})


# ---------------------------------------------------------------------------------------------------------------------------
# the example, the names, the C entry

def test_the_example_transforms_a_file(tmp_path, monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import transform_ply
    p = seeded_scene(40, 4, seed=9)
    src, dst = str(tmp_path / "in.compressed.ply"), str(tmp_path / "out.ply")
    ms.save_compressed_ply(src, p, backend="torch")
    monkeypatch.setattr(sys, "argv", ["transform_ply.py", src, dst, "--rotate-axis-angle", "0", "0", "1", "90", "--scale", "2",
                                      "--translate", "1", "0", "0", "--crop-box", "-4", "-4", "-4", "4", "4", "4", "--backend", "torch"])
    transform_ply.main()
    got = ms.load_ply(dst, backend="torch")
    loaded = ms.load_compressed_ply(src, backend="torch")
    assert float((transform_ply.axis_angle_matrix([0, 0, 2.0], 90.0) - rot_z(90.0)).abs().max()) < 1e-15
    want = ms.transform_scene(loaded, rotation=transform_ply.axis_angle_matrix([0, 0, 1.0], 90.0), scale=2.0, translation=[1.0, 0.0, 0.0], backend="torch")
    keep = ((want["means3d"].abs() <= 4).all(1))
    assert 5 < int(keep.sum()) < 40 and same_scene(got, {k: v[keep] for k, v in want.items()})
    assert [transform_ply.saver_for(n) for n in ("a.splat", "a.ply", "a.compressed.ply")] == \
        [ms.save_splat, ms.save_ply, ms.save_compressed_ply]


def test_public_names_and_the_exported_symbol():
    for name in ("sh_rotation_matrices", "transform_scene", "transform_camera", "crop_scene", "merge_scenes"):
        assert name in ms.__all__ and getattr(ms, name) is getattr(edit, name)
    lib = _hip.load()
    assert hasattr(lib, "ms_scene_transform") and "ms_scene_transform" in _hip.EXPORTS
    assert ctypes.sizeof(_hip.Transform) == 181 * 4


def test_c_abi_argument_validation():
    """ms_scene_transform validates before it touches the device (fake non-null pointers; nothing is dereferenced)."""
    L = _hip.load()
    P, Q = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002)
    xf = _hip.Transform()
    OK, INVALID, TOO_LARGE = 0, 1, 3
    N = ctypes.c_int64(10)

    def err():
        return L.ms_last_error_string().decode()

    ptrs = [P] * 4, [P] * 4
    assert L.ms_scene_transform(ctypes.c_int64(-1), 4, *ptrs[0], xf, *ptrs[1], None) == INVALID and "N < 0" in err()
    assert L.ms_scene_transform(ctypes.c_int64(0), 4, None, None, None, None, None, None, None, None, None, None) == OK
    for K in (0, 2, 5, 26, -1):
        assert L.ms_scene_transform(N, K, *ptrs[0], xf, *ptrs[1], None) == INVALID and f"K = {K}" in err()
    assert L.ms_scene_transform(N, 16, *ptrs[0], None, *ptrs[1], None) == INVALID and "xf" in err()
    for i in range(8):
        a = [P] * 8
        a[i] = None
        assert L.ms_scene_transform(N, 9, *a[:4], xf, *a[4:], None) == INVALID and "null" in err()
        a[i] = Q
        assert L.ms_scene_transform(N, 1, *a[:4], xf, *a[4:], None) == INVALID and "misaligned" in err()
    for K in (1, 25):
        assert L.ms_scene_transform(ctypes.c_int64(2 ** 40), K, *ptrs[0], xf, *ptrs[1], None) == TOO_LARGE
