"""Scene editing: move a scene in space.  A rigid or similarity transform x' = s R x + t of the whole scene -- means, scales,
rotations AND the view-dependent colour -- plus the small companions an import / export pipeline needs (the camera that goes
with a transformed scene, a crop, a merge)::

    params = load_ply("scene.ply")                                          # y-down, arbitrary SfM units
    params = transform_scene(params, rotation=R_up, scale=1 / metres_per_unit, translation=-centre)
    cam = transform_camera(cam, rotation=R_up, scale=1 / metres_per_unit, translation=-centre)   # sees the same image
    params, kept = crop_scene(params, box=((-1, -1, 0), (1, 1, 2)))
    both = merge_scenes(params, other)

``params`` is the five-key dict ``save_ply`` takes (``sceneio._validate_params`` checks it): "means3d" (N, 3); "scales" (N, 3),
LOG-scales; "quats" (N, 4), wxyz, not normalised; "opacities" (N,), in either space (they pass through); "features"
(N, K, 3) SH coefficients with K in {1, 4, 9, 16, 25}, or (N, 3) RGB.  Other keys are ignored.

WHY NOT FIVE LINES OF TORCH.  Rotating the means and the quaternions and leaving the SH coefficients alone silently gives
wrong view-dependent colour: band l >= 1 of every Gaussian has to be multiplied by the rotation's (2l+1) x (2l+1) real Wigner
matrix in this package's basis and sign convention (``sh.py``: gsplat's, k = l (l + 1) + m, 3DGS signs).

``sh_rotation_matrices(R, degree)`` -> [M_1 .. M_degree], float64.  For unit directions d and the row vector b_l(d) (band l of
``sh.sh_basis_torch``), M_l is the matrix with b_l(R^T d) = b_l(d) M_l; the rotated scene's band-l coefficients are
c'_l = M_l c_l per channel.  It is computed by least squares over 64 fixed Fibonacci-sphere directions from the package's own
basis function (``pinv(basis(dirs)) @ basis(dirs @ R)`` per band), so the convention cannot drift from the evaluator's.

THE MAP.  ``transform_scene(params, matrix)`` with a 4x4 (or 3x4) matrix -- nested lists, numpy or a tensor, read in float64 --
or ``transform_scene(params, rotation=R, translation=t, scale=s)``; both is a ValueError.  Accepted (ValueError otherwise,
before any launch): every entry finite; last row [0, 0, 0, 1]; the upper 3x3 B = s R with det B > 0, s = det(B)^(1/3) finite
and positive, max |B^T B / s^2 - I| <= 1e-6 (this admits matrices typed in float32 and rejects shear, non-uniform scale and
reflections, which a quaternion and three log-scales cannot represent).  R is then replaced by its nearest rotation (the polar
factor U V^T of the SVD, float64).  Given as parts, ``rotation`` passes the same test with s = 1 and ``scale`` is taken as it is.

THE CONSTANTS, all derived in float64 and rounded ONCE to float32: A = fl(s R); t; r = the unit quaternion wxyz of R with
w >= 0; l = fl(ln s); M_1 .. M_deg.  r is extracted by Shepperd's method: of the trace and the three diagonal entries the
largest picks which component is computed from a square root (so that no small number is divided by), the other three come from
the off-diagonal sums and differences; then r is normalised and its sign chosen so that w > 0, or, where w == 0, so that the
first non-zero component is positive.

THE DEFINITION is ``backend="torch"``.  For float32 tensors every operation below is a separately rounded float32 multiply or
add, in exactly this order; nothing is skipped for a zero matrix entry, so NaN, Inf and -0.0 propagate::

    means   x'_i = ((A_i0 x + A_i1 y) + A_i2 z) + t_i
    scales  scales + l
    quats   q' = r (x) q, not normalised (the renderer normalises)
            w' = ((r_w q_w - r_x q_x) - r_y q_y) - r_z q_z        x' = ((r_w q_x + r_x q_w) + r_y q_z) - r_z q_y
            y' = ((r_w q_y - r_x q_z) + r_y q_w) + r_z q_x        z' = ((r_w q_z + r_x q_y) - r_y q_x) + r_z q_w
            each product rounded, the sums taken left to right; a - b c is evaluated as a + (-b) c -- the same bits for every
            input that is not a NaN (negation is exact), and only multiplies and adds occur
    features  band 0 copied; band l, row m: acc = M[m][0] c[l^2]; acc = acc + M[m][j] c[l^2 + j], j = 1 .. 2l, per channel;
            (N, 3) RGB copied
    opacities  detach().clone()

float64 tensors run the same formulas in float64 with the unrounded constants (the invariance tests use this).  The five
tensors must share one dtype, float32 or float64.  The result is five new, contiguous leaf tensors that share no storage with
the input, ``requires_grad`` as given (default False).

``backend="hip"`` is ``ms_scene_transform`` (csrc/transform.hip): float32 CUDA/ROCm contiguous tensors (ValueError otherwise:
there is no fallback), ONE launch on the current stream, no atomics, no workspace, no host wait; 4 (11 + 3 K) bytes read and as
many written per Gaussian; bit for bit the definition.

``transform_camera`` returns the camera that sees the transformed scene as the given camera saw the original: view rotation
R_v R^T, view translation s T_v - R_v R^T t, so that V' x' = s (V x) and the projection is unchanged; intrinsics are kept.
``near`` / ``far`` are NOT rescaled: depths grow by s, so scale them yourself if s differs much from 1.

``crop_scene`` keeps the Gaussians whose mean lies in a closed box or a closed sphere (or, ``invert=True``, outside it);
``merge_scenes`` concatenates two scenes.  Both are torch ops and run on CPU tensors too.

Not covered: optimiser moments (an edited scene starts a fresh optimiser), non-uniform scale, shear and reflections, the
sharded trainer, per-Gaussian masks for a partial transform (crop, transform, merge does that).
"""
import math

import torch

from .sceneio import TENSORS, _check_backend, _sh_features, _validate_params
from .utils import Camera

_N_DIRS = 64
_ORTHO_TOL = 1e-6


def _degree_of(K):
    return 0 if K is None else math.isqrt(K) - 1


# ---------------------------------------------------------------------------------------------------------------------------
# the rotation of the SH bands

def _fibonacci_sphere(n):
    i = torch.arange(n, dtype=torch.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    rho = torch.sqrt(1.0 - z * z)
    return torch.stack([rho * torch.cos(phi), rho * torch.sin(phi), z], dim=1)


def sh_rotation_matrices(R, degree):
    """[M_1 .. M_degree], M_l float64 (2l+1, 2l+1) on the CPU, with b_l(R^T d) = b_l(d) M_l for the basis of ``sh.py`` (module
    docstring): a scene rotated by R has the band-l coefficients M_l c_l.  R: 3x3, anything ``torch.as_tensor`` reads."""
    from .sh import MAX_SH_DEGREE, sh_basis_torch
    if not (isinstance(degree, int) and 0 <= degree <= MAX_SH_DEGREE):
        raise ValueError(f"degree must be an int in [0, {MAX_SH_DEGREE}], got {degree!r}")
    R = _as_f64(R, "R")
    if R.shape != (3, 3):
        raise ValueError(f"R must be 3x3, got {tuple(R.shape)}")
    dirs = _fibonacci_sphere(_N_DIRS)
    a, a_rot = sh_basis_torch(degree, dirs), sh_basis_torch(degree, dirs @ R)
    return [torch.linalg.pinv(a[:, l * l:(l + 1) ** 2]) @ a_rot[:, l * l:(l + 1) ** 2] for l in range(1, degree + 1)]


# ---------------------------------------------------------------------------------------------------------------------------
# the map

def _as_f64(x, what):
    try:
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=torch.float64)     # (a list is read in float64, not float32)
        return t.detach().to(device="cpu", dtype=torch.float64)
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"{what} is not numeric: {e}") from None


def _rotation_of(B, what):
    """B = s R -> (s, R): the checks of the module docstring, then the polar factor."""
    if not bool(torch.isfinite(B).all()):
        raise ValueError(f"{what} has a non-finite entry")
    det = float(torch.linalg.det(B))
    if not det > 0.0:
        raise ValueError(f"{what}: the 3x3 part has determinant {det:g}; a positive one is required (a reflection or a "
                         "singular matrix is not a similarity transform of a Gaussian scene)")
    s = det ** (1.0 / 3.0)
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError(f"{what}: the scale {s!r} is not finite and positive")
    err = float((B.T @ B / (s * s) - torch.eye(3, dtype=torch.float64)).abs().max())
    if not err <= _ORTHO_TOL:
        raise ValueError(f"{what}: the 3x3 part is not a uniform scale times a rotation (max |B^T B / s^2 - I| = {err:.3g} > "
                         f"{_ORTHO_TOL:g}): shear and non-uniform scale are not representable")
    U, _, Vh = torch.linalg.svd(B / s)
    return s, U @ Vh


def _similarity(matrix, rotation, translation, scale):
    """-> (s float, R (3, 3) float64, t (3,) float64): the accepted maps of the module docstring, ValueError otherwise."""
    parts = rotation is not None or translation is not None or not (isinstance(scale, (int, float)) and scale == 1.0)
    if matrix is not None:
        if parts:
            raise ValueError("give either matrix or rotation / translation / scale, not both")
        m = _as_f64(matrix, "matrix")
        if m.shape not in ((4, 4), (3, 4)):
            raise ValueError(f"matrix must be 4x4 or 3x4, got {tuple(m.shape)}")
        if not bool(torch.isfinite(m).all()):
            raise ValueError("matrix has a non-finite entry")
        if m.shape[0] == 4 and m[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
            raise ValueError(f"matrix: the last row is {m[3].tolist()}, not [0, 0, 0, 1] (a projective map is not a similarity)")
        s, R = _rotation_of(m[:3, :3], "matrix")
        return s, R, m[:3, 3].clone()
    try:
        s = float(scale)
    except (TypeError, ValueError):
        raise ValueError(f"scale must be a number, got {scale!r}") from None
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError(f"scale must be finite and positive, got {s!r}")
    R = torch.eye(3, dtype=torch.float64)
    if rotation is not None:
        R = _as_f64(rotation, "rotation")
        if R.shape != (3, 3):
            raise ValueError(f"rotation must be 3x3, got {tuple(R.shape)}")
        one, R = _rotation_of(R, "rotation")
        if abs(one - 1.0) > _ORTHO_TOL:
            raise ValueError(f"rotation: the matrix scales by {one:.9g}; give the scale as scale=")
    t = torch.zeros(3, dtype=torch.float64)
    if translation is not None:
        t = _as_f64(translation, "translation").reshape(-1)
        if t.shape != (3,) or not bool(torch.isfinite(t).all()):
            raise ValueError("translation must be three finite numbers")
    return s, R, t


def _quaternion(R):
    """The unit quaternion wxyz of a rotation matrix, float64, by Shepperd's method; w >= 0 (module docstring)."""
    m = R.tolist()
    tr = m[0][0] + m[1][1] + m[2][2]
    pick = max(range(4), key=lambda i: (tr, m[0][0], m[1][1], m[2][2])[i])
    if pick == 0:
        w = 0.5 * math.sqrt(1.0 + tr)
        q = [w, (m[2][1] - m[1][2]) / (4 * w), (m[0][2] - m[2][0]) / (4 * w), (m[1][0] - m[0][1]) / (4 * w)]
    else:
        i = pick - 1
        j, k = (i + 1) % 3, (i + 2) % 3
        u = 0.5 * math.sqrt(1.0 + m[i][i] - m[j][j] - m[k][k])
        q = [0.0] * 4
        q[0] = (m[k][j] - m[j][k]) / (4 * u)
        q[1 + i] = u
        q[1 + j] = (m[j][i] + m[i][j]) / (4 * u)
        q[1 + k] = (m[k][i] + m[i][k]) / (4 * u)
    n = math.sqrt(sum(c * c for c in q))
    q = [c / n for c in q]
    lead = next((c for c in q if c != 0.0), 1.0)
    if q[0] < 0.0 or (q[0] == 0.0 and lead < 0.0):
        q = [-c for c in q]
    return [c + 0.0 for c in q]                                     # (-0.0 -> +0.0)


class _Constants:
    """What the formulas read, as Python floats: A (3 x 3), t, r, l, M (a list of matrices as nested lists)."""

    def __init__(self, s, R, t, degree, single):
        A = (s * R)
        M = sh_rotation_matrices(R, degree)
        r = torch.tensor(_quaternion(R), dtype=torch.float64)
        ell = torch.tensor(math.log(s), dtype=torch.float64)
        if single:                                                  # the one rounding
            A, t, r, ell = (x.to(torch.float32).to(torch.float64) for x in (A, t, r, ell))
            M = [x.to(torch.float32).to(torch.float64) for x in M]
        self.A, self.t, self.r, self.l, self.M = A.tolist(), t.tolist(), r.tolist(), float(ell), [x.tolist() for x in M]

    def struct(self):
        from . import _hip
        xf = _hip.Transform()
        xf.A[:] = [v for row in self.A for v in row]
        xf.t[:] = self.t
        xf.r[:] = self.r
        xf.l = self.l
        for name, M in zip(("M1", "M2", "M3", "M4"), self.M):
            getattr(xf, name)[:] = [v for row in M for v in row]
        return xf


# ---------------------------------------------------------------------------------------------------------------------------
# the definition, and the launch

def _transform_torch(t, K, c):
    means, scales, quats, _, feats = t
    A, tt, (rw, rx, ry, rz) = c.A, c.t, c.r
    x, y, z = means.unbind(1)
    out_means = torch.stack([((A[i][0] * x + A[i][1] * y) + A[i][2] * z) + tt[i] for i in range(3)], dim=1)
    out_scales = scales + c.l
    qw, qx, qy, qz = quats.unbind(1)
    out_quats = torch.stack([((rw * qw + (-rx) * qx) + (-ry) * qy) + (-rz) * qz,
                             ((rw * qx + rx * qw) + ry * qz) + (-rz) * qy,
                             ((rw * qy + (-rx) * qz) + ry * qw) + rz * qx,
                             ((rw * qz + rx * qy) + (-ry) * qx) + rz * qw], dim=1)
    out_feats = feats.clone()
    for l, M in enumerate(c.M, start=1):
        base, width = l * l, 2 * l + 1
        for m in range(width):
            acc = M[m][0] * feats[:, base]
            for j in range(1, width):
                acc = acc + M[m][j] * feats[:, base + j]
            out_feats[:, base + m] = acc
    return out_means, out_scales, out_quats, out_feats


def _transform_hip(t, K, c, out=None):
    """``out``: the four tensors to write into (tests: pre-filled, every element must be overwritten)."""
    from . import _hip
    L = _hip.lib()
    means, scales, quats, _, feats = t
    dev, N = means.device, means.shape[0]
    outs = [torch.empty_like(x) for x in (means, scales, quats, feats)] if out is None else list(out)
    xf = c.struct()
    with _hip.on_device(dev):
        _hip.check(L.ms_scene_transform(N, K or 1, _hip.ptr(means), _hip.ptr(scales), _hip.ptr(quats), _hip.ptr(feats), xf,
                                        *[_hip.ptr(x) for x in outs], _hip.stream(dev)), "ms_scene_transform")
    return tuple(outs)


def _leaves(tensors, requires_grad):
    return {k: x.detach().contiguous().requires_grad_(bool(requires_grad)) for k, x in zip(TENSORS, tensors)}


def transform_scene(params, matrix=None, *, rotation=None, translation=None, scale=1.0, backend="hip", requires_grad=False) -> dict:
    """The scene moved by x' = s R x + t (module docstring: the accepted maps, the constants, the formulas) -> a new params
    dict of five contiguous leaf tensors.  backend="torch": the definition, float32 or float64 tensors on any device.
    backend="hip": ms_scene_transform, one launch on the current stream, no host wait; float32 CUDA/ROCm contiguous tensors;
    bit for bit the definition; no fallback.  Every check is made before anything is launched."""
    _check_backend(backend)
    s, R, tr = _similarity(matrix, rotation, translation, scale)
    N, K, t = _validate_params(params, backend)
    dtype = t[0].dtype
    if any(x.dtype != dtype for x in t) or dtype not in (torch.float32, torch.float64):
        raise ValueError(f"the five tensors must share one dtype, float32 or float64, got { {k: x.dtype for k, x in zip(TENSORS, t)} }")
    c = _Constants(s, R, tr, _degree_of(K), single=dtype == torch.float32)
    with torch.no_grad():
        out = _transform_torch(t, K, c) if backend == "torch" else _transform_hip(t, K, c)
        means, scales, quats, feats = out
        return _leaves((means, scales, quats, t[3].clone(), feats), requires_grad)


# ---------------------------------------------------------------------------------------------------------------------------
# the companions (torch ops; they run on CPU tensors too)

def transform_camera(camera, matrix=None, *, rotation=None, translation=None, scale=1.0) -> Camera:
    """The camera that sees ``transform_scene(params, <the same map>)`` as ``camera`` sees ``params``: view rotation
    R_v R^T, view translation s T_v - R_v R^T t (computed in float64 from ``camera.view_matrix``, returned in its dtype and
    on its device), so that V' x' = s (V x): means2d, conics and colours are unchanged, depths grow by s.  Intrinsics are
    kept; ``near`` / ``far`` are NOT rescaled."""
    s, R, t = _similarity(matrix, rotation, translation, scale)
    vm = camera.view_matrix.detach()
    v = vm.to(device="cpu", dtype=torch.float64)
    Rv = v[:3, :3] @ R.T
    Tv = s * v[:3, 3] - Rv @ t
    return Camera(R=Rv.to(device=vm.device, dtype=vm.dtype).contiguous(), T=Tv.to(device=vm.device, dtype=vm.dtype).contiguous(),
                  H=camera.H, W=camera.W, fx=camera.fx, fy=camera.fy, cx=camera.cx, cy=camera.cy, near=camera.near, far=camera.far)


def _three(x, what, device, dtype):
    v = _as_f64(x, what).reshape(-1)
    if v.shape != (3,):
        raise ValueError(f"{what} must be three numbers")
    return v.to(device=device, dtype=dtype)


def crop_scene(params, *, box=None, sphere=None, invert=False, requires_grad=False):
    """-> (params of the kept Gaussians, keep_mask (N,) bool).  ``box=(lo, hi)``: lo <= mean <= hi in every coordinate;
    ``sphere=(centre, radius)``: |mean - centre|^2 <= radius^2; both closed, compared in the means' dtype; exactly one must be
    given.  ``invert=True`` keeps the outside instead.  A Gaussian whose mean has a NaN is dropped either way.  Rows keep their
    order; the result is five new contiguous leaf tensors (possibly empty)."""
    if (box is None) == (sphere is None):
        raise ValueError("give exactly one of box=(lo, hi) and sphere=(centre, radius)")
    _, _, t = _validate_params(params, "torch")
    means = t[0]
    with torch.no_grad():
        if box is not None:
            lo, hi = (_three(b, "box bound", means.device, means.dtype) for b in box)
            inside = ((means >= lo) & (means <= hi)).all(dim=1)
        else:
            centre, radius = sphere
            radius = float(radius)
            if not radius >= 0.0:
                raise ValueError(f"the sphere's radius must be >= 0, got {radius!r}")
            d = means - _three(centre, "sphere centre", means.device, means.dtype)
            inside = (d * d).sum(dim=1) <= radius * radius
        keep = (~inside if invert else inside) & ~torch.isnan(means).any(dim=1)
        return _leaves([x[keep].clone() for x in t], requires_grad), keep


def merge_scenes(a, b, *, requires_grad=False) -> dict:
    """The Gaussians of ``a`` followed by those of ``b``.  Features of the lower K are zero-padded to the larger (the missing
    bands contribute nothing); (N, 3) RGB features are converted to degree-0 SH (``(rgb - 0.5) / SH_C0``) when the other scene
    holds SH, and stay RGB when both are RGB.  Both scenes must use the SAME opacity space (logit or linear: nothing is
    converted), one dtype and one device."""
    _, Ka, ta = _validate_params(a, "torch")
    _, Kb, tb = _validate_params(b, "torch")
    if ta[0].device != tb[0].device:
        raise ValueError(f"the scenes are on different devices: {ta[0].device} and {tb[0].device}")
    if any(x.dtype != y.dtype for x, y in zip(ta, tb)):
        raise ValueError("the scenes' tensors differ in dtype")
    with torch.no_grad():
        if (Ka is None) != (Kb is None) or (Ka is not None and Ka != Kb):
            K = max(Ka or 1, Kb or 1)
            for t, k in ((ta, Ka), (tb, Kb)):
                f = _sh_features(t[4], k)
                pad = f.new_zeros((f.shape[0], K - f.shape[1], 3))
                t[4] = torch.cat([f, pad], dim=1)
        return _leaves([torch.cat([x, y], dim=0) for x, y in zip(ta, tb)], requires_grad)


__all__ = ["sh_rotation_matrices", "transform_scene", "transform_camera", "crop_scene", "merge_scenes"]
