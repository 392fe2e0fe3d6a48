"""GPU: the row move of scene files in HIP (csrc/sceneio.hip; mojosplat_amd/sceneio.py with backend="hip") against its
definition (pack_ply_rows_torch / unpack_ply_rows_torch) on the same device and inputs, compared as int32 -- random bit
patterns, so NaN payloads, infinities, -0.0 and denormals all occur -- at sizes around the 64 rows of a workgroup; files
written by one backend and read by the other; a saved and loaded scene rendered and stepped."""
import pytest
import torch

from mojosplat_amd import GaussianAdam, _hip, init_from_points, load_ply, pack_ply_rows, render_gaussians, save_ply, unpack_ply_rows
from mojosplat_amd import sceneio
from mojosplat_amd.autograd import render_gaussians_trainable
from mojosplat_amd.scenes import randscene_v1
from mojosplat_amd.sceneio import column_map, pack_ply_rows_torch, property_names, unpack_ply_rows_torch

pytestmark = pytest.mark.gpu

B = _hip.PLY_ROWS
NS = sorted({1, 63, 64, 65, 257, 1000, B - 1, B, B + 1})
KS = (1, 4, 9, 16)
KEYS = ("means3d", "scales", "quats", "opacities", "features")
SENTINEL = 0x5EA71E55


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _random_bits(shape, g, device):
    return torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32).to(device)


def _scene(N, K, seed, device, rgb=False):
    g = _gen(seed)
    return {"means3d": _random_bits((N, 3), g, device), "scales": _random_bits((N, 3), g, device),
            "quats": _random_bits((N, 4), g, device), "opacities": _random_bits((N,), g, device),
            "features": _random_bits((N, 3) if rgb else (N, K, 3), g, device)}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return all(a[k].shape == b[k].shape and torch.equal(_bits(a[k]), _bits(b[k])) for k in KEYS)


@pytest.mark.parametrize("K", KS + ("rgb",))
def test_pack_equals_the_definition(device, K):
    for N in NS:
        p = _scene(N, 1 if K == "rgb" else K, 100 + N, device, rgb=K == "rgb")
        assert N < 1000 or bool(torch.isnan(p["means3d"]).any())          # (random bits: one float in 128 is a NaN)
        want = pack_ply_rows_torch(p)
        got = pack_ply_rows(p)
        assert got.shape == want.shape == (N, 14 + 3 * (1 if K == "rgb" else K))
        assert got.dtype == torch.float32 and got.is_contiguous() and got.device == p["means3d"].device
        bad = int((_bits(got) != _bits(want)).any(1).sum())
        assert bad == 0, f"N={N} K={K}: {bad} rows differ"


@pytest.mark.parametrize("K", KS)
def test_unpack_equals_the_definition(device, K):
    F = 14 + 3 * K
    names = list(property_names(K))
    g = _gen(7 + K)
    perm = torch.randperm(F + 5, generator=g).tolist()
    shuffled = [(names + [f"extra_{i}" for i in range(5)])[i] for i in perm]
    widths = (3, 3, 4, 1, 3 * K)
    for N in NS:
        for tag, cols in (("identity", names), ("shuffled", shuffled)):
            rows = _random_bits((N, len(cols)), g, device)
            want = unpack_ply_rows_torch(rows, cols)
            got = unpack_ply_rows(rows, cols)
            assert _same(got, want), f"{tag} N={N} K={K}"
            assert all(got[k].dtype == torch.float32 and got[k].is_contiguous() for k in KEYS)
            assert got["features"].shape == (N, K, 3) and got["opacities"].shape == (N,)
            # into outputs full of a sentinel: every element is overwritten
            out = [torch.full((N, w), SENTINEL, dtype=torch.int32, device=device).view(torch.float32) for w in widths]
            again = sceneio._unpack_hip(rows, K, column_map(cols)[1], out=out)
            assert _same(again, want), f"{tag} N={N} K={K}: an output element kept the sentinel"
            assert again["means3d"].data_ptr() == out[0].data_ptr()


def test_unpack_at_the_widest_row_and_pack_of_unpack(device):
    """S = 192 floats per row (the documented cap: 64 such rows fill the kernel's LDS image), then pack(unpack) = the named columns."""
    K, N = 16, 130
    names = list(property_names(K))
    S = _hip.PLY_MAX_STRIDE
    g = _gen(3)
    cols = [(names + [f"extra_{i}" for i in range(S - len(names))])[i] for i in torch.randperm(S, generator=g).tolist()]
    rows = _random_bits((N, S), g, device)
    want = unpack_ply_rows_torch(rows, cols)
    got = unpack_ply_rows(rows, cols)
    assert _same(got, want)
    packed = pack_ply_rows(got)
    where = [cols.index(n) for n in names if n not in ("nx", "ny", "nz")]
    keep = [i for i, n in enumerate(names) if n not in ("nx", "ny", "nz")]
    assert torch.equal(_bits(packed)[:, keep], _bits(rows)[:, where])
    with pytest.raises(ValueError, match="more than 192"):
        unpack_ply_rows(torch.zeros((2, S + 1), device=device), cols + ["one_more"])


def test_bases_that_are_not_16_byte_aligned(device):
    """Tensors that start 4 bytes into an allocation take the dword path; the result is the same."""
    N, K = 131, 4
    F = 14 + 3 * K
    p = _scene(N, K, 55, device)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=device)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    q = {k: shifted(v) for k, v in p.items()}
    want = pack_ply_rows_torch(p)
    assert torch.equal(_bits(pack_ply_rows(q)), _bits(want))
    rows = shifted(want)
    names = property_names(K)
    assert _same(unpack_ply_rows(rows, names), p)
    out = [shifted(torch.full((N, w), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)) for w in (3, 3, 4, 1, 3 * K)]
    assert _same(sceneio._unpack_hip(want, K, column_map(names)[1], out=out), p)
    assert F % 2 == 0 and (N * F) % 4 == 2                    # (and the last workgroup ends in a tail of 2 floats)


@pytest.mark.parametrize("K", (1, 16))
def test_files_cross_the_backends_both_ways(device, tmp_path, K):
    N = 777
    p = _scene(N, K, 9 + K, device)
    cpu = {k: v.cpu() for k, v in p.items()}
    before = {k: v.clone() for k, v in p.items()}
    a, b = str(tmp_path / "hip.ply"), str(tmp_path / "torch.ply")
    na = save_ply(a, p)                                        # GPU, "hip"
    assert _same(p, before)                                    # the source tensors are unchanged
    nb = save_ply(b, cpu, backend="torch")                     # CPU, "torch"
    data = open(a, "rb").read()
    assert na == nb == len(data) and data == open(b, "rb").read()
    got_cpu = load_ply(a, backend="torch")
    assert all(v.device.type == "cpu" for v in got_cpu.values()) and _same(got_cpu, cpu)
    got_gpu = load_ply(b)
    assert all(v.is_cuda and v.is_leaf and v.is_contiguous() and v.dtype == torch.float32 for v in got_gpu.values())
    assert got_gpu["means3d"].device == torch.device("cuda", torch.cuda.current_device())
    assert _same({k: v.cpu() for k, v in got_gpu.items()}, cpu)
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        load_ply(a, device="cpu")
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        save_ply(a, cpu)
    assert open(a, "rb").read() == data


def test_linear_opacities_and_rgb_agree_across_backends(device, tmp_path):
    """The conversions are the same torch ops for both backends: on the same device the two files are the same bytes."""
    scene, _ = randscene_v1(300, 64, 64, seed=8, device=device)          # activated opacities, (N, 3) RGB
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    save_ply(a, scene, opacity_space="linear")
    save_ply(b, scene, opacity_space="linear", backend="torch")
    assert open(a, "rb").read() == open(b, "rb").read()
    x, y = load_ply(a, opacity_space="linear"), load_ply(a, opacity_space="linear", backend="torch", device=device)
    assert _same(x, y) and x["features"].shape == (300, 1, 3)
    # o -> logit -> sigmoid: the logit is off by a few 2^-24 of |log o| + |log1p(-o)|, and d sigmoid = o (1 - o) of that is at
    # most 2^-22 * max x exp(-x) < 1e-7; the sigmoid's own rounding adds 2^-23
    assert float((x["opacities"] - scene["opacities"]).abs().max()) < 1e-6


def test_a_loaded_scene_renders_and_trains(device, tmp_path):
    """init_from_points (degree 3, 500 points) -> save -> load: both dicts render the same bits at 64 x 64, and the loaded one
    goes straight into GaussianAdam and takes a step."""
    scene, cam = randscene_v1(500, 64, 64, ell=-1.5, seed=4, device=device)
    p = init_from_points(scene["means3d"], torch.rand((500, 3), generator=_gen(18)).to(device), sh_degree=3, init_opacity=0.5)
    with torch.no_grad():
        p["features"][:, 1:] = 0.1 * torch.randn((500, 15, 3), generator=_gen(19)).to(device)
        p["quats"].copy_(scene["quats"])
    path = str(tmp_path / "scene.ply")
    before = {k: v.detach().clone() for k, v in p.items()}
    save_ply(path, p)
    assert _same(p, before)
    q = load_ply(path, requires_grad=True)
    assert _same(p, q)
    assert all(v.is_leaf and v.requires_grad and v.is_contiguous() and v.dtype == torch.float32 for v in q.values())

    def render(d):
        with torch.no_grad():
            return render_gaussians(d["means3d"], d["scales"], d["quats"], torch.sigmoid(d["opacities"]), d["features"], cam,
                                    sh_degree=3, backend="hip")

    img_p, img_q = render(p), render(q)
    assert img_p.shape == (64, 64, 3) and float(img_p.abs().sum()) > 0
    assert torch.equal(_bits(img_p), _bits(img_q))
    opt = GaussianAdam(q, lr=1e-3)
    img = render_gaussians_trainable(q["means3d"], q["scales"], q["quats"], torch.sigmoid(q["opacities"]), q["features"], cam,
                                     sh_degree=3)
    img.square().mean().backward()
    opt.step()
    assert bool(torch.isfinite(q["means3d"]).all()) and not torch.equal(q["means3d"].detach(), p["means3d"].detach())
