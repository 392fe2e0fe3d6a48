"""The inputs both edit test files run on (tests/test_edit_cpu.py, tests/test_hip_edit.py): seeded random scenes, the maps, and
the five rows of special values -- one kind per row, so that no sum ever meets two NaNs of different bits (which of two
NaNs an addition returns is the one thing IEEE 754 leaves open)."""
import math

import torch

KEYS = ("means3d", "scales", "quats", "opacities", "features")
KS = (1, 4, 9, 16, 25, None)               # None: (N, 3) RGB features
# around the 64 rows of a workgroup, a partial last one, several; K = 1 and RGB take 256 rows a workgroup
NS = (1, 63, 64, 65, 257)
NS_K1 = NS + (255, 256)


def sizes(K):
    return NS_K1 if K in (1, None) else NS


def seeded_scene(N, K, seed=0, device="cpu", dtype=torch.float32):
    g = torch.Generator().manual_seed(1000 * seed + 32 * N + (K or 0))
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    f = torch.rand((N, 3), generator=g, dtype=torch.float64) if K is None else 1.5 * r(N, K, 3)
    p = {"means3d": 2.0 * r(N, 3), "scales": r(N, 3) - 1.0, "quats": r(N, 4), "opacities": 2.0 * r(N), "features": f}
    return {k: v.to(device=device, dtype=dtype) for k, v in p.items()}


def random_rotation(seed):
    """A proper rotation, float64, from the QR factorisation of a seeded Gaussian matrix."""
    g = torch.Generator().manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn((3, 3), generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    return q if torch.linalg.det(q) > 0 else -q


def rot_z(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)


ROT_Z90 = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
# name -> keyword arguments of transform_scene / transform_camera
MAPS = {
    "identity": dict(),
    "z90": dict(rotation=ROT_Z90),
    "similarity": dict(rotation=random_rotation(11), scale=1.7, translation=[0.3, -1.1, 2.5]),
}


def as_matrix(rotation=None, scale=1.0, translation=None):
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = scale * (torch.eye(3, dtype=torch.float64) if rotation is None else rotation)
    if translation is not None:
        m[:3, 3] = torch.as_tensor(translation, dtype=torch.float64)
    return m


SPECIAL_N = 5
ROW_NAN, ROW_PINF, ROW_NINF, ROW_NEGZERO, ROW_DENORMAL = range(SPECIAL_N)
DENORMAL = 1e-40


def special_scene(K, device="cpu"):
    """N = 5, float32: row 0 holds NaNs, row 1 +Inf, row 2 -Inf, row 3 -0.0 (and +0.0), row 4 denormals, each in some
    components of every tensor and next to ordinary values."""
    p = seeded_scene(SPECIAL_N, K, seed=9)
    for row, v in ((ROW_NAN, math.nan), (ROW_PINF, math.inf), (ROW_NINF, -math.inf), (ROW_NEGZERO, -0.0), (ROW_DENORMAL, DENORMAL)):
        p["means3d"][row, 1] = v
        p["scales"][row, 2] = v
        p["quats"][row, 0] = v
        p["quats"][row, 3] = v
        p["opacities"][row] = v
        if K is None:
            p["features"][row, 2] = v
        else:
            p["features"][row, 0, 1] = v
            for k in range(1, K, 2):                                # every second higher coefficient, channels in turn
                p["features"][row, k, k % 3] = v
    p["means3d"][ROW_NEGZERO] = torch.tensor([-0.0, -0.0, 0.0])
    p["quats"][ROW_NEGZERO] = torch.tensor([-0.0, 0.0, -0.0, -0.0])
    if K is not None and K > 1:
        p["features"][ROW_NEGZERO, 1:4] = -0.0                      # a whole band of -0.0: sums of signed zeros
    return {k: v.to(device) for k, v in p.items()}


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.device == b.device and torch.equal(bits(a), bits(b))


def same_scene(a, b):
    return all(same_bits(a[k], b[k]) for k in KEYS)
