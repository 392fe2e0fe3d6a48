"""GPU: the viewer formats in HIP (csrc/splatio.hip; mojosplat_amd/splatio.py with backend="hip") against their definition
(backend="torch") on the same device and inputs, BIT FOR BIT -- chunks, packed words, SH bytes, .splat rows and every decoded
float -- at sizes around the 256 Gaussians of a chunk and on the hand-built edge cases of tests/test_splatio_cpu.py; both
orders; two calls in a row; a partial last chunk into guard-filled buffers; bases the kernels cannot vectorise on; the
ValueErrors of the HIP path; files written by one backend and read by the other."""
import pytest
import torch

import mojosplat_amd as ms
from mojosplat_amd import splatio
from splatio_cases import KEYS, KS, NS, hand_built_scene, seeded_scene

pytestmark = pytest.mark.gpu

GUARD = 0x5A


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and a.device == b.device and torch.equal(_bits(a), _bits(b))


def _same_scene(a, b):
    return all(_equal(a[k], b[k]) for k in KEYS)


def _same_compressed(a, b):
    return a.K == b.K and all(_equal(x, y) for x, y in zip(a[:4], b[:4]))


def _check_scene(p, space, orders=("morton", "keep")):
    N = p["means3d"].shape[0]
    for order in orders:
        want = ms.compress_scene(p, opacity_space=space, order=order, backend="torch")
        got = ms.compress_scene(p, opacity_space=space, order=order)
        again = ms.compress_scene(p, opacity_space=space, order=order)
        assert _same_compressed(got, want), f"compress N={N} {order}"
        assert _same_compressed(again, got), f"compress N={N} {order}: two calls differ"
        assert got.vertices.dtype == torch.int32 and got.vertices.is_contiguous() and got.chunks.shape == (-(-N // 256), 18)
        # the decoded floats, as the kernel leaves them and as the params dict
        raw_want = splatio._decompress_torch(want.chunks, want.vertices, want.sh)
        raw_got = splatio._decompress_hip(want.chunks, want.vertices, want.sh)
        for name, x, y in zip(("pos", "rot", "lsc", "rgba", "shr"), raw_got, raw_want):
            assert _equal(x, y), f"decompress N={N} {order}: {name}"
        assert all(_equal(x, y) for x, y in zip(splatio._decompress_hip(want.chunks, want.vertices, want.sh), raw_got))
        d_want = ms.decompress_scene(want, opacity_space=space, backend="torch")
        d_got = ms.decompress_scene(want, opacity_space=space)
        assert _same_scene(d_got, d_want)
        assert all(v.is_leaf and v.is_contiguous() and v.dtype == torch.float32 and v.is_cuda for v in d_got.values())
    for order in ("importance", "keep"):
        want, wperm = splatio.pack_splat_rows(p, opacity_space=space, order=order, backend="torch")
        got, gperm = splatio.pack_splat_rows(p, opacity_space=space, order=order)
        again, _ = splatio.pack_splat_rows(p, opacity_space=space, order=order)
        assert _equal(got, want) and _equal(gperm, wperm) and _equal(again, got), f"splat pack N={N} {order}"
        raw_want = splatio._splat32_unpack_torch(want)
        raw_got = splatio._splat32_unpack_hip(want)
        for name, x, y in zip(("pos", "scale", "rgba", "rot"), raw_got, raw_want):
            assert _equal(x, y), f"splat unpack N={N} {order}: {name}"
        assert all(_equal(x, y) for x, y in zip(splatio._splat32_unpack_hip(want), raw_got))
        assert _same_scene(splatio.unpack_splat_rows(want, opacity_space=space),
                           splatio.unpack_splat_rows(want, opacity_space=space, backend="torch"))


@pytest.mark.parametrize("K", KS)
def test_hip_equals_the_definition_bit_for_bit(device, K):
    for N in NS:
        _check_scene(seeded_scene(N, K, device=device), "logit")


def test_the_hand_built_cases_equal_the_definition(device):
    p = hand_built_scene(device)
    _check_scene(p, "linear")
    cs = ms.compress_scene(p, opacity_space="linear", order="keep")
    assert int((cs.vertices[256:, 0] != 0).sum()) == 0 and float(cs.chunks[0, 6]) == -20.0 and float(cs.chunks[0, 10]) == 20.0


def _guard(rows, width, dtype, device):
    """A (rows, width) tensor of `dtype` whose every byte is GUARD."""
    size = torch.empty((), dtype=dtype).element_size()
    return torch.full((rows, width * size), GUARD, dtype=torch.uint8, device=device).view(dtype)


def _untouched(t, n):
    return bool((t[n:].contiguous().view(torch.uint8) == GUARD).all())


def test_a_partial_last_chunk_writes_no_row_past_n(device):
    """N = 257: the second chunk holds one row.  Every output gets 300 rows (chunks: one) to spare, filled with a guard byte."""
    N, K, spare = 257, 9, 300
    p = seeded_scene(N, K, seed=2, device=device)
    want = ms.compress_scene(p, order="keep", backend="torch")
    t = splatio._validate_params(p, "hip")[2]
    prepared = splatio._prepare(t, K, want.perm, "logit")
    out = (_guard(2 + 1, 18, torch.float32, device), _guard(N + spare, 4, torch.int32, device),
           _guard(N + spare, 3 * (K - 1), torch.uint8, device))
    splatio._compress_hip(*prepared, out=out)
    for got, ref, n in zip(out, (want.chunks, want.vertices, want.sh), (2, N, N)):
        assert _equal(got[:n], ref) and _untouched(got, n)
    assert _equal(out[0][1, 0:3], out[0][1, 3:6])                      # a chunk of one row: min == max
    ref = splatio._decompress_torch(want.chunks, want.vertices, want.sh)
    out = tuple(_guard(N + spare, w, torch.float32, device) for w in (3, 4, 3, 4, 3 * (K - 1)))
    splatio._decompress_hip(want.chunks, want.vertices, want.sh, out=out)
    for got, r in zip(out, ref):
        assert _equal(got[:N], r) and _untouched(got, N)
    rows, perm = splatio.pack_splat_rows(p, order="keep", backend="torch")
    pos, rot, _, rgba, _ = prepared
    scale_lin = torch.exp(p["scales"]).contiguous()
    out = _guard(N + spare, 32, torch.uint8, device)
    splatio._splat32_pack_hip(pos, scale_lin, rgba, rot, out=out)
    assert _equal(out[:N], rows) and _untouched(out, N)
    ref = splatio._splat32_unpack_torch(rows)
    out = tuple(_guard(N + spare, w, torch.float32, device) for w in (3, 3, 4, 4))
    splatio._splat32_unpack_hip(rows, out=out)
    for got, r in zip(out, ref):
        assert _equal(got[:N], r) and _untouched(got, N)


def test_sh_arrays_whose_bases_are_not_aligned(device):
    """shr 4 bytes and sh 1 byte into an allocation: the SH maps take their element-by-element path; the result is the same."""
    N, K = 300, 4
    R = 3 * (K - 1)
    p = seeded_scene(N, K, seed=4, device=device)
    want = ms.compress_scene(p, order="keep", backend="torch")
    pos, rot, lsc, rgba, shr = splatio._prepare(splatio._validate_params(p, "hip")[2], K, want.perm, "logit")

    def shifted(t, dtype):
        buf = torch.empty(t.numel() + 1, dtype=dtype, device=device)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % (4 * buf.element_size()) == buf.element_size() and v.is_contiguous()
        return v

    out = (torch.empty((2, 18), device=device), torch.empty((N, 4), dtype=torch.int32, device=device),
           shifted(torch.zeros((N, R), dtype=torch.uint8, device=device), torch.uint8))
    splatio._compress_hip(pos, rot, lsc, rgba, shifted(shr, torch.float32), out=out)
    assert _equal(out[2], want.sh) and _equal(out[1], want.vertices) and _equal(out[0], want.chunks)
    ref = splatio._decompress_torch(want.chunks, want.vertices, want.sh)
    out = tuple(torch.empty((N, w), device=device) for w in (3, 4, 3, 4)) + (shifted(torch.zeros((N, R), device=device), torch.float32),)
    splatio._decompress_hip(want.chunks, want.vertices, shifted(want.sh, torch.uint8), out=out)
    assert all(_equal(x, y) for x, y in zip(out, ref))


def test_chunks_of_12_floats_decode_like_the_definition(device):
    p = seeded_scene(300, 4, seed=5, device=device)
    cs = ms.compress_scene(p)
    cs12 = cs._replace(chunks=cs.chunks[:, :12].contiguous())
    assert _same_scene(ms.decompress_scene(cs12), ms.decompress_scene(cs12, backend="torch"))
    assert not torch.equal(ms.decompress_scene(cs12)["features"][:, 0], ms.decompress_scene(cs)["features"][:, 0])


def test_the_value_errors_of_the_hip_path(device):
    p = seeded_scene(40, 4, device=device)
    calls = (ms.compress_scene, splatio.pack_splat_rows)
    for fn in calls:
        with pytest.raises(ValueError, match="CUDA/ROCm"):
            fn({k: v.cpu() for k, v in p.items()})
        with pytest.raises(ValueError, match="contiguous"):
            fn({**p, "quats": p["quats"].t().contiguous().t()})
        with pytest.raises(ValueError, match="float32"):
            fn({**p, "scales": p["scales"].double()})
        with pytest.raises(ValueError, match="float32"):
            fn({**p, "features": p["features"].half()})
    cs = ms.compress_scene(p)
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        ms.decompress_scene(cs._replace(chunks=cs.chunks.cpu(), vertices=cs.vertices.cpu(), sh=cs.sh.cpu()))
    with pytest.raises(ValueError, match="contiguous"):
        ms.decompress_scene(cs._replace(sh=cs.sh.t().contiguous().t()))
    with pytest.raises(ValueError, match="different devices"):
        ms.decompress_scene(cs._replace(sh=cs.sh.cpu()))
    rows, _ = splatio.pack_splat_rows(p)
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        splatio.unpack_splat_rows(rows.cpu())
    with pytest.raises(ValueError, match="contiguous"):
        splatio.unpack_splat_rows(rows.t().contiguous().t())
    with pytest.raises(ValueError, match="uint8"):
        splatio.unpack_splat_rows(rows.int())


@pytest.mark.parametrize("K", (1, 16))
def test_files_cross_the_backends_both_ways(device, tmp_path, K):
    N = 777
    p = seeded_scene(N, K, seed=6, device=device)
    before = {k: v.clone() for k, v in p.items()}
    for ext, save, load in ((".compressed.ply", ms.save_compressed_ply, ms.load_compressed_ply), (".splat", ms.save_splat, ms.load_splat)):
        a, b = str(tmp_path / ("hip" + ext)), str(tmp_path / ("torch" + ext))
        na = save(a, p)                                            # "hip"
        nb = save(b, p, backend="torch")                           # the definition on the same device
        assert _same_scene(p, before)
        data = open(a, "rb").read()
        assert na == nb == len(data) and data == open(b, "rb").read()
        x = load(a, backend="torch", device=device)                # saved with "hip", loaded with "torch"
        y = load(b)                                                # ... and the reverse
        assert _same_scene(x, y)
        assert all(v.is_cuda and v.is_leaf and v.is_contiguous() and v.dtype == torch.float32 for v in y.values())
        assert y["features"].shape == (N, K if ext != ".splat" else 1, 3)
        assert y["means3d"].device == torch.device("cuda", torch.cuda.current_device())
        assert all(v.device.type == "cpu" for v in load(a, backend="torch").values())
        with pytest.raises(ValueError, match="CUDA/ROCm"):
            load(a, device="cpu")
        with pytest.raises(ValueError, match="CUDA/ROCm"):
            save(a, {k: v.cpu() for k, v in p.items()})
        assert open(a, "rb").read() == data
