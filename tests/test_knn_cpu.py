"""CPU: the definition of the k-nearest-neighbour search (mojosplat_amd/knn.py, knn_torch) on hand-computed cases, against
a float64 brute force and chunk by chunk; init_from_points(backend="torch") against its formulas and as the input of
GaussianAdam and densify_and_prune; scene_extent; every ValueError; and the host logic of ms_knn (argument validation
needs no GPU)."""
import ctypes
import math

import pytest
import torch

import mojosplat_amd as ms
from mojosplat_amd import Camera, DensifyStats, GaussianAdam, _hip, densify_and_prune, init_from_points, knn, scene_extent
from mojosplat_amd.knn import knn_torch
from mojosplat_amd.sh import evaluate_sh_torch

INF = float("inf")


def test_four_points_on_a_line():
    p = torch.tensor([[0.0, 0, 0], [1, 0, 0], [3, 0, 0], [7, 0, 0]])
    d, i = knn(p, k=3, backend="torch")
    assert d.dtype == torch.float32 and i.dtype == torch.int64 and d.shape == i.shape == (4, 3)
    assert d.tolist() == [[1, 9, 49], [1, 4, 36], [4, 9, 16], [16, 36, 49]]
    assert i.tolist() == [[1, 2, 3], [0, 2, 3], [1, 0, 3], [2, 1, 0]]
    d1, i1 = knn(p, k=1, backend="torch")
    assert d1.tolist() == [[1], [1], [4], [16]] and i1.tolist() == [[1], [0], [1], [2]]
    d2, none = knn(p, k=2, return_index=False, backend="torch")
    assert none is None and torch.equal(d2, d[:, :2])


def test_unit_square_and_its_centre():
    p = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0]])
    d, i = knn(p, k=3, backend="torch")
    # a corner: the centre at 0.5, then the two adjacent corners at 1, the smaller row first; the centre: four ties by row
    assert d.tolist() == [[0.5, 1, 1]] * 4 + [[0.5, 0.5, 0.5]]
    assert i.tolist() == [[4, 1, 2], [4, 0, 3], [4, 0, 3], [4, 1, 2], [0, 1, 2]]
    d4, i4 = knn(p, k=4, backend="torch")
    assert d4[:4, 3].tolist() == [2.0] * 4 and i4[:, 3].tolist() == [3, 2, 1, 0, 3]


def test_identical_points_are_neighbours_and_ties_go_by_row():
    p = torch.tensor([[2.0, 2, 2], [2, 2, 2], [5, 2, 2], [2, 2, 2]])
    d, i = knn(p, k=3, backend="torch")
    assert d.tolist() == [[0, 0, 9], [0, 0, 9], [9, 9, 9], [0, 0, 9]]
    assert i.tolist() == [[1, 3, 2], [0, 3, 2], [0, 1, 3], [0, 1, 2]]


def test_chunked_equals_unchunked():
    g = torch.Generator().manual_seed(0)
    p = torch.rand((300, 3), generator=g)
    p[100:140] = p[:40]                                         # duplicates: ties across chunk borders
    whole = knn_torch(p, 5, chunk=300)
    for chunk in (1, 7, 64, 299, 1000):
        part = knn_torch(p, 5, chunk=chunk)
        assert torch.equal(part[0], whole[0]) and torch.equal(part[1], whole[1]), chunk
    assert torch.equal(knn_torch(p, 5)[1], whole[1])
    # float64 points: computed in float32, from the rounded coordinates
    assert torch.equal(knn(p.double(), k=5, backend="torch")[1], whole[1])


def test_neighbour_sets_against_a_float64_brute_force():
    g = torch.Generator().manual_seed(1)
    N, k = 500, 8
    p = torch.rand((N, 3), generator=g)
    d64 = torch.cdist(p.double(), p.double()) ** 2
    d64.fill_diagonal_(INF)
    val, ind = torch.sort(d64, dim=1)
    # no float64 tie within 1e-6 relative among the first k + 1 of any row: the float32 order cannot differ from it
    gap = (val[:, 1:k + 1] - val[:, :k]) / val[:, 1:k + 1]
    assert float(gap.min()) > 1e-6
    d, i = knn(p, k=k, backend="torch")
    assert torch.equal(torch.sort(i, dim=1).values, torch.sort(ind[:, :k], dim=1).values)
    assert torch.equal(i, ind[:, :k])
    assert float(((d.double() - val[:, :k]) / val[:, :k]).abs().max()) <= 6 * 2.0 ** -24       # (five roundings of 2^-24 each)


def _cam(position):
    """A camera at `position` looking along +z: R = I, T = -position."""
    return Camera(R=torch.eye(3), T=-torch.tensor(position, dtype=torch.float32), H=48, W=64, fx=60.0, fy=60.0, cx=32.0, cy=24.0)


def test_init_from_points_values():
    g = torch.Generator().manual_seed(2)
    N = 200
    p = torch.rand((N, 3), generator=g)
    p[7] = p[3]
    p[9] = p[3]
    p[11] = p[3]                                                # four equal points: m = 0, the floor min_dist2 holds
    rgb = torch.rand((N, 3), generator=g)
    out = init_from_points(p, rgb, backend="torch")
    assert list(out) == ["means3d", "scales", "quats", "opacities", "features"]
    for t in out.values():
        assert t.dtype == torch.float32 and t.is_contiguous() and t.is_leaf and t.requires_grad and t.grad_fn is None
    assert torch.equal(out["means3d"].detach(), p) and out["means3d"].data_ptr() != p.data_ptr()
    d, _ = knn(p, k=3, backend="torch")
    m = ((d[:, 0] + d[:, 1]) + d[:, 2]) / torch.tensor(3.0)
    want = torch.log(torch.sqrt(torch.clamp_min(m, 1e-7)) * 1.0)
    assert out["scales"].shape == (N, 3) and all(torch.equal(out["scales"].detach()[:, c], want) for c in range(3))
    assert float(m[3]) == 0.0 and float(out["scales"].detach()[3, 0]) == pytest.approx(0.5 * math.log(1e-7), rel=1e-6)
    # against float64: the scale is the root of the mean squared distance
    m64 = (torch.cdist(p.double(), p.double()) ** 2).fill_diagonal_(INF).sort(dim=1).values[:, :3].mean(1)
    ok = m64 > 1e-7
    assert float((out["scales"].detach()[:, 0].double()[ok] - 0.5 * torch.log(m64[ok])).abs().max()) <= 1e-6
    assert out["quats"].shape == (N, 4) and torch.equal(out["quats"].detach(), torch.tensor([1.0, 0, 0, 0]).expand(N, 4))
    assert out["opacities"].shape == (N,) and float(out["opacities"].detach()[0]) == pytest.approx(math.log(0.1 / 0.9), rel=1e-6)
    assert torch.equal(out["features"].detach(), rgb) and out["features"].data_ptr() != rgb.data_ptr()

    # init_scale, k, linear opacities, no gradients
    o2 = init_from_points(p, rgb, k=5, init_scale=0.5, init_opacity=0.3, opacity_space="linear", min_dist2=1e-4,
                          requires_grad=False, backend="torch")
    d5, _ = knn(p, k=5, backend="torch")
    m5 = ((((d5[:, 0] + d5[:, 1]) + d5[:, 2]) + d5[:, 3]) + d5[:, 4]) / torch.tensor(5.0)
    assert torch.equal(o2["scales"][:, 1], torch.log(torch.sqrt(torch.clamp_min(m5, 1e-4)) * 0.5))
    assert torch.equal(o2["opacities"], torch.full((N,), 0.3)) and not any(t.requires_grad for t in o2.values())


def test_init_from_points_colours_and_sh_layout():
    g = torch.Generator().manual_seed(3)
    N = 60
    p = torch.rand((N, 3), generator=g) + torch.tensor([0.0, 0.0, 3.0])
    u8 = torch.randint(0, 256, (N, 3), generator=g, dtype=torch.uint8)
    assert torch.equal(init_from_points(p, u8, backend="torch")["features"].detach(), u8.float() / 255.0)
    assert torch.equal(init_from_points(p, None, backend="torch")["features"].detach(), torch.full((N, 3), 0.5))
    assert torch.equal(init_from_points(p, u8.double() / 255.0, backend="torch")["features"].detach(), (u8.double() / 255.0).float())
    rgb = torch.rand((N, 3), generator=g)
    cam = _cam([0.1, -0.2, 0.0])
    for degree in (0, 1, 3):
        f = init_from_points(p, rgb, sh_degree=degree, backend="torch")["features"].detach()
        assert f.shape == (N, (degree + 1) ** 2, 3)
        assert torch.equal(f[:, 0], (rgb - 0.5) / 0.2820947917738781) and not f[:, 1:].any()
        back = evaluate_sh_torch(p, f, cam, 0)
        assert float((back - rgb).abs().max()) <= 1e-6
        if degree:
            assert float((evaluate_sh_torch(p, f, cam, degree) - rgb).abs().max()) <= 1e-6
    grey = init_from_points(p, None, sh_degree=2, backend="torch")["features"]
    assert not grey.detach().any()


def test_the_dict_feeds_the_optimiser_and_the_densifier():
    g = torch.Generator().manual_seed(4)
    N = 120
    params = init_from_points(torch.rand((N, 3), generator=g), torch.rand((N, 3), generator=g), sh_degree=1, backend="torch")
    opt = GaussianAdam(params, lr=1e-3, backend="torch")
    for t in params.values():
        t.grad = torch.randn(t.shape, generator=g)
    before = params["means3d"].detach().clone()
    opt.step()
    assert not torch.equal(params["means3d"].detach(), before) and all(torch.isfinite(t).all() for t in params.values())
    stats = DensifyStats(N)
    stats.grad2d[:30] = 1.0
    stats.count[:] = 1.0
    res = densify_and_prune(params, stats, opt, scene_scale=10.0, opacity_space="logit", generator=g, backend="torch")
    assert res.n_cloned + res.n_split == 30 and res.params["features"].shape[1:] == (4, 3)
    assert res.params["means3d"].shape[0] == N + res.n_cloned + res.n_split - res.n_pruned


def test_scene_extent():
    cams = [_cam([0.0, 0.0, 0.0]), _cam([4.0, 0.0, 0.0]), _cam([2.0, 6.0, 0.0])]
    # centres' mean (2, 2, 0); distances sqrt(8), sqrt(8), 4
    assert scene_extent(cams) == pytest.approx(4.4, rel=1e-6)
    assert scene_extent(iter(cams[:1])) == 0.0
    assert isinstance(scene_extent(cams), float)
    # a rotated camera: the centre is -R^T T
    c, s = math.cos(0.3), math.sin(0.3)
    R = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    centre = torch.tensor([10.0, 0.0, 0.0])
    far = Camera(R=R, T=-(R @ centre), H=48, W=64, fx=60.0, fy=60.0, cx=32.0, cy=24.0)
    assert scene_extent([cams[0], far]) == pytest.approx(1.1 * 5.0, rel=1e-6)
    with pytest.raises(ValueError, match="at least one camera"):
        scene_extent([])


def test_every_value_error():
    p = torch.rand((20, 3), generator=torch.Generator().manual_seed(5))
    for call in (lambda *a, **kw: knn(*a, **{"backend": "torch", **kw}), lambda *a, **kw: init_from_points(*a, **{"backend": "torch", **kw})):
        for bad in (0, 9, -1, 3.0, True, None):
            with pytest.raises(ValueError, match="k must be"):
                call(p, k=bad)
        for bad in (p[:, :2], p.reshape(-1), p.reshape(20, 3, 1), p.long(), p.tolist()):
            with pytest.raises(ValueError, match="shape"):
                call(bad)
        with pytest.raises(ValueError, match="k \\+ 1 = 4 <= N"):
            call(p[:3], k=3)
        with pytest.raises(ValueError, match="k \\+ 1 = 9 <= N"):
            call(p[:8], k=8)
        assert call(p[:4], k=3) is not None                     # N = k + 1 is enough
        for bad in (INF, -INF, float("nan")):
            q = p.clone()
            q[13, 1] = bad
            with pytest.raises(ValueError, match="not finite"):
                call(q)
        with pytest.raises(ValueError, match="backend"):
            call(p, backend="triton")
        # backend="hip" (the default) has no fallback
        with pytest.raises(ValueError, match="CUDA/ROCm"):
            call(p, backend="hip")
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        knn(p)
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        init_from_points(p)
    init = lambda **kw: init_from_points(p, **{"backend": "torch", **kw})
    for bad in (torch.rand(19, 3), torch.rand(20, 4), torch.rand(20), torch.rand(20, 3).tolist(), torch.rand(20, 3, device="meta")):
        with pytest.raises(ValueError, match="colors"):
            init(colors=bad)
    with pytest.raises(ValueError, match="colors"):
        init(colors=torch.zeros((20, 3), dtype=torch.int32))
    for bad in (-1, 5, 1.0, True):
        with pytest.raises(ValueError, match="sh_degree"):
            init(sh_degree=bad)
    for bad in (0.0, -1.0, INF, float("nan"), "1"):
        with pytest.raises(ValueError, match="init_scale"):
            init(init_scale=bad)
        with pytest.raises(ValueError, match="min_dist2"):
            init(min_dist2=bad)
    for bad in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="init_opacity"):
            init(init_opacity=bad)
    with pytest.raises(ValueError, match="opacity_space"):
        init(opacity_space="sigmoid")


def test_exports():
    for name in ("knn", "init_from_points", "scene_extent"):
        assert name in ms.__all__ and hasattr(ms, name)
    assert ms.knn is knn and ms.init_from_points is init_from_points and ms.scene_extent is scene_extent


def test_library_exports_and_validates_ms_knn():
    lib = _hip.load()
    for name in ("ms_knn_workspace_bytes", "ms_knn"):
        assert hasattr(lib, name) and name in _hip.EXPORTS
    B = _hip.KNN_BLOCK
    assert B >= 64 and B % 64 == 0 and _hip.KNN_MAX_K == 8
    P, ODD, OFF8 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002), ctypes.c_void_p(0x1004)    # validation never dereferences
    OK, INVALID, WORKSPACE, TOO_LARGE = 0, 1, 2, 3
    err = lambda: lib.ms_last_error_string().decode()
    # 16 bytes per sorted point, 32 per block's box
    assert lib.ms_knn_workspace_bytes(1000, 3) == 16000 + 32 * -(-1000 // B)
    assert lib.ms_knn_workspace_bytes(0, 3) == 0 and lib.ms_knn_workspace_bytes(1000, 9) == 0 and lib.ms_knn_workspace_bytes(1 << 31, 3) == 0

    def call(N=1000, points=P, order=P, k=3, dist2=P, idx=P, ws=P):
        return lib.ms_knn(N, points, order, k, dist2, idx, ws, None)

    for bad in (0, -1, 9):
        assert call(k=bad) == INVALID and "k = " in err()
    for N, k in ((3, 3), (1, 1), (0, 1), (-5, 2), (8, 8)):
        assert call(N=N, k=k) == INVALID and "neighbours" in err(), (N, k)
    assert call(N=1 << 31) == TOO_LARGE and "2^31" in err()
    for arg in ("points", "dist2", "ws"):
        assert call(**{arg: None}) == INVALID and "null" in err(), arg
    assert call(points=ODD) == INVALID and "misaligned" in err()
    assert call(order=ODD) == INVALID and "misaligned" in err()
    assert call(dist2=ODD) == INVALID and "misaligned" in err()
    assert call(idx=OFF8) == INVALID and "misaligned" in err()
    assert call(ws=ctypes.c_void_p(0x1008)) == INVALID and "misaligned" in err()
    assert WORKSPACE == 2 and OK == 0                           # (ms_knn takes no workspace size: nothing to be short of)
