"""GPU: the exact k-nearest-neighbour search in HIP (csrc/knn.hip; mojosplat_amd/knn.py with backend="hip") against its
definition (knn_torch) run on the same device and inputs: ``torch.equal`` on the squared distances AND on the indices, no
tolerance, on the point sets that break an inexact search -- sizes around the block size, mass ties at box-boundary
distances, duplicates, far clusters, degenerate boxes, coordinates coarser than the points' spacing, densities four decades
apart."""
import pytest
import torch

from mojosplat_amd import GaussianAdam, _hip, init_from_points, knn, photometric_loss
from mojosplat_amd.autograd import render_gaussians_trainable
from mojosplat_amd.knn import _knn_hip, knn_torch
from mojosplat_amd.scene_order import morton_permutation
from mojosplat_amd.scenes import randscene_v1

pytestmark = pytest.mark.gpu

B = _hip.KNN_BLOCK
KS = (1, 3, 8)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _same(points, k, tag=""):
    """knn(backend="hip") gives the definition's bits; -> (dist2, idx)."""
    want_d, want_i = knn_torch(points, k)
    got_d, got_i = knn(points, k=k)
    assert got_d.shape == (points.shape[0], k) and got_d.dtype == torch.float32 and got_d.is_contiguous()
    assert got_i.shape == (points.shape[0], k) and got_i.dtype == torch.int64 and got_i.is_contiguous()
    bad = int((got_d != want_d).any(1).sum()), int((got_i != want_i).any(1).sum())
    assert torch.equal(got_d, want_d) and torch.equal(got_i, want_i), f"{tag} k={k}: rows with a wrong distance / index: {bad}"
    return got_d, got_i


def _lattice(device, side=12, seed=0):
    r = torch.arange(side, dtype=torch.float32)
    p = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), dim=-1).reshape(-1, 3)
    return p[torch.randperm(p.shape[0], generator=_gen(seed))].contiguous().to(device)


def _blobs(n_blobs, per_blob, seed, lo=-4.0, hi=0.0):
    """Gaussian blobs in the unit cube whose standard deviations run from 10^lo to 10^hi."""
    g = _gen(seed)
    centres = torch.rand((n_blobs, 1, 3), generator=g)
    sigma = 10.0 ** torch.linspace(lo, hi, n_blobs).reshape(n_blobs, 1, 1)
    return (centres + sigma * torch.randn((n_blobs, per_blob, 3), generator=g)).reshape(-1, 3)


@pytest.mark.parametrize("k", KS)
def test_sizes_around_the_block(device, k):
    for N in sorted({k + 1, 5, 63, 64, 65, B - 1, B, B + 1, 3 * B + 7}):
        if N < k + 1:
            continue
        _same(torch.rand((N, 3), generator=_gen(N)).to(device), k, f"uniform N={N}")


@pytest.mark.parametrize("k", KS)
def test_all_points_identical(device, k):
    """Nothing can be pruned and every tie is broken by row."""
    p = torch.full((2 * B + 3, 3), 0.25, device=device)
    d, i = _same(p, k, "identical")
    assert not d.any() and i[0].tolist() == list(range(1, k + 1)) and i[-1].tolist() == list(range(k))


@pytest.mark.parametrize("k", KS)
def test_shuffled_lattice(device, k):
    """Mass distance ties at box-boundary distances: a non-strict skip test or a tie-break by sorted position fails here."""
    d, _ = _same(_lattice(device), k, "lattice")
    assert float(d[:, 0].max()) == 1.0


@pytest.mark.parametrize("k", KS)
def test_lattice_with_every_point_stored_twice(device, k):
    """Self is excluded by row: the twin at distance 0 is a neighbour."""
    p = _lattice(device, seed=1)
    p = torch.cat([p, p])[torch.randperm(2 * p.shape[0], generator=_gen(2)).to(device)].contiguous()
    d, _ = _same(p, k, "doubled lattice")
    assert not d[:, 0].any() and (k == 1 or float(d[:, 1].min()) == 1.0)


@pytest.mark.parametrize("k", KS)
def test_two_clusters_far_apart(device, k):
    """The small cluster has only k points: each of them takes a neighbour from the cluster 1e3 away."""
    g = _gen(3)
    big = torch.rand((3 * B + 5, 3), generator=g)
    small = torch.rand((k, 3), generator=g) + torch.tensor([1e3, 0.0, 0.0])
    p = torch.cat([big[:B], small, big[B:]]).to(device)
    d, i = _same(p, k, "two clusters")
    rows = torch.arange(B, B + k, device=device)
    far = (i[rows] < B) | (i[rows] >= B + k)
    assert bool((far.sum(1) == 1).all()) and bool((d[rows, -1] > 9e5).all())


@pytest.mark.parametrize("k", KS)
def test_degenerate_bounding_boxes(device, k):
    g = _gen(4)
    N = 2 * B + 9
    t = torch.rand((N, 1), generator=g)
    line = torch.tensor([0.3, -1.0, 2.0]) + t * torch.tensor([1.0, 2.0, -0.5])
    _same(line.to(device), k, "collinear")
    axis = torch.cat([t, torch.zeros((N, 2))], dim=1)
    _same(axis.contiguous().to(device), k, "on an axis")
    plane = torch.rand((N, 3), generator=g)
    plane[:, 1] = 0.75
    _same(plane.to(device), k, "coplanar")
    u, v = torch.rand((N, 1), generator=g), torch.rand((N, 1), generator=g)
    _same((u * torch.tensor([1.0, 1.0, 0.0]) + v * torch.tensor([0.0, 1.0, 1.0])).to(device), k, "oblique plane")


@pytest.mark.parametrize("k", KS)
def test_offset_coarser_than_the_spacing(device, k):
    """A unit cube at 1e6: float32 there steps by 1/16, so many points coincide and many distances are exactly 0."""
    p = (torch.rand((3000, 3), generator=_gen(5)) + 1e6).to(device)
    d, _ = _same(p, k, "offset cube")
    assert int((d[:, 0] == 0).sum()) > 100


@pytest.mark.parametrize("k", KS)
def test_blobs_four_decades_apart(device, k):
    _same(_blobs(9, 300, seed=6).to(device), k, "blobs")


def test_many_blocks(device):
    """20 000 points, half uniform and half blobs: hundreds of blocks against the chunked definition (4e8 pairs)."""
    p = torch.cat([torch.rand((10_000, 3), generator=_gen(7)), _blobs(20, 500, seed=8)])
    p = p[torch.randperm(p.shape[0], generator=_gen(9))].contiguous().to(device)
    _same(p, 3, "20k")


def test_any_order_gives_the_same_bits(device):
    p = torch.cat([torch.rand((1500, 3), generator=_gen(10)), _blobs(5, 200, seed=11), _lattice("cpu", 6)]).to(device)
    N = p.shape[0]
    for k in KS:
        want = _same(p, k, "orders")
        for name, order in (("as stored", None),
                            ("random", torch.randperm(N, generator=_gen(12)).to(device=device, dtype=torch.int32)),
                            ("reversed morton", morton_permutation(p).flip(0).to(torch.int32).contiguous())):
            got = _knn_hip(p, N, k, True, order=order)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (name, k)


def test_two_calls_give_the_same_bits_and_return_index(device):
    p = _blobs(6, 500, seed=13).to(device)
    a, b = knn(p, k=8), knn(p, k=8)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    d, none = knn(p, k=8, return_index=False)
    assert none is None and torch.equal(d, a[0])
    # the default is k = 3, the HIP backend
    d3, i3 = knn(p)
    assert torch.equal(d3, a[0][:, :3]) and torch.equal(i3, a[1][:, :3])


def test_no_fallback(device):
    p = torch.rand((100, 3), generator=_gen(14)).to(device)
    with pytest.raises(ValueError, match="float32"):
        knn(p.double())
    with pytest.raises(ValueError, match="float32"):
        knn(p.half())
    with pytest.raises(ValueError, match="contiguous"):
        knn(torch.rand((3, 100), device=device).t())
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        knn(p.cpu())
    q = p.clone()
    q[5, 2] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        knn(q)


def test_init_from_points_is_bit_identical(device):
    p = torch.cat([torch.rand((700, 3), generator=_gen(15)), _blobs(4, 100, seed=16)]).to(device)
    p[10] = p[3]
    p[20] = p[3]
    p[30] = p[3]
    rgb = torch.rand((p.shape[0], 3), generator=_gen(17)).to(device)
    for kw in (dict(), dict(sh_degree=3, k=5, init_scale=0.7, opacity_space="linear", init_opacity=0.4),
               dict(colors=(rgb * 255).to(torch.uint8), sh_degree=0, requires_grad=False)):
        kw = {"colors": rgb, **kw}
        ref, got = init_from_points(p, backend="torch", **kw), init_from_points(p, **kw)
        assert list(ref) == list(got)
        for n in ref:
            a, b = ref[n], got[n]
            assert b.is_cuda and b.is_leaf and b.is_contiguous() and b.dtype == torch.float32 and b.requires_grad == a.requires_grad
            assert torch.equal(a.detach(), b.detach()), n
        assert bool(torch.isfinite(got["scales"]).all())


def test_one_training_step_from_a_point_cloud(device):
    """500 points at 64 x 64: render_gaussians_trainable -> photometric_loss -> GaussianAdam.step."""
    names = ("means3d", "scales", "quats", "opacities", "features")
    scene, cam = randscene_v1(500, 64, 64, ell=-1.5, seed=4, device=device)
    with torch.no_grad():
        target = render_gaussians_trainable(*[scene[n] for n in names], cam).detach()
    p = init_from_points(scene["means3d"], torch.rand((500, 3), generator=_gen(18)).to(device), init_opacity=0.5,
                         opacity_space="linear")
    opt = GaussianAdam(p, lr=1e-3)
    before = {n: p[n].detach().clone() for n in names}
    loss = photometric_loss(render_gaussians_trainable(*[p[n] for n in names], cam), target)
    loss.backward()
    grad = p["means3d"].grad
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().sum()) > 0
    opt.step()
    assert all(bool(torch.isfinite(p[n]).all()) for n in names)
    assert not torch.equal(p["means3d"].detach(), before["means3d"])
