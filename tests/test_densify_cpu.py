"""CPU: the densification statistics' definition (densify.py, update_torch), the DensifyStats book-keeping,
and the argument checks of the two C entry points that update them on the GPU."""
import ctypes

import pytest
import torch

import mojosplat_amd as ms
from mojosplat_amd import _hip
from mojosplat_amd.densify import DensifyStats, update_torch


def _stats(n, grad=0.0, count=0.0, maxr=0.0):
    st = DensifyStats(n, "cpu")
    st.grad2d.fill_(grad), st.count.fill_(count), st.max_radii.fill_(maxr)
    return st


def test_update_torch_leaves_culled_gaussians_untouched():
    st = _stats(4, grad=0.5, count=2.0, maxr=0.25)
    radii = torch.tensor([[0, 0], [3, 0], [0, 5], [2, 2]], dtype=torch.int32)
    g = torch.tensor([[1.0, 1.0], [2.0, -1.0], [-3.0, 4.0], [0.0, 0.0]])
    update_torch(st, g, radii, 64, 32)
    assert st.grad2d.tolist() == [0.5, 0.5, 0.5, 0.5]
    assert st.count.tolist() == [2.0, 2.0, 2.0, 3.0]        # alive, zero gradient: counts
    assert st.max_radii.tolist() == [0.25, 0.25, 0.25, 0.25]  # 2 / 64 < 0.25


def test_update_torch_scales_the_gradient_to_ndc():
    st = _stats(3)
    radii = torch.ones(3, 2, dtype=torch.int32)
    g = torch.tensor([[1.0, 0.0], [0.0, 1.0], [3.0, 4.0]])
    W, H = 200, 100
    update_torch(st, g, radii, W, H)
    assert st.grad2d[0].item() == pytest.approx(W / 2)
    assert st.grad2d[1].item() == pytest.approx(H / 2)
    assert st.grad2d[2].item() == pytest.approx(((3 * W / 2) ** 2 + (4 * H / 2) ** 2) ** 0.5)


def test_update_torch_normalises_the_largest_radius():
    st = _stats(3)
    radii = torch.tensor([[7, 3], [2, 9], [4, 4]], dtype=torch.int32)
    update_torch(st, torch.zeros(3, 2), radii, 320, 640)
    assert st.max_radii.tolist() == [torch.tensor(7 / 640, dtype=torch.float32).item(),
                                     torch.tensor(9 / 640, dtype=torch.float32).item(),
                                     torch.tensor(4 / 640, dtype=torch.float32).item()]
    update_torch(st, torch.zeros(3, 2), torch.tensor([[1, 1], [20, 1], [0, 30]], dtype=torch.int32), 320, 640)
    assert st.max_radii[0].item() == torch.tensor(7 / 640, dtype=torch.float32).item()   # max, not last
    assert st.max_radii[1].item() == torch.tensor(20 / 640, dtype=torch.float32).item()
    assert st.max_radii[2].item() == torch.tensor(4 / 640, dtype=torch.float32).item()   # culled: untouched


def test_update_torch_accumulates_over_views():
    st = _stats(2)
    g1, g2 = torch.tensor([[0.1, 0.2], [0.3, 0.0]]), torch.tensor([[0.0, 0.5], [1.0, 1.0]])
    r1 = torch.tensor([[1, 1], [2, 2]], dtype=torch.int32)
    r2 = torch.tensor([[3, 1], [0, 0]], dtype=torch.int32)
    update_torch(st, g1, r1, 10, 10)
    update_torch(st, g2, r2, 10, 10)
    n = lambda g: float(torch.sqrt((g[0] * 5) ** 2 + (g[1] * 5) ** 2))
    assert st.count.tolist() == [2.0, 1.0]
    assert st.grad2d[0].item() == pytest.approx(n(g1[0]) + n(g2[0]))
    assert st.grad2d[1].item() == pytest.approx(n(g1[1]))
    assert st.max_radii.tolist() == pytest.approx([0.3, 0.2])
    assert st.mean_grad()[0].item() == pytest.approx((n(g1[0]) + n(g2[0])) / 2)


def test_densify_stats_keeps_its_buffers_aligned():
    st = DensifyStats(5, "cpu")
    assert ms.DensifyStats is DensifyStats
    for t in (st.grad2d, st.count, st.max_radii):
        assert t.shape == (5,) and t.dtype == torch.float32
    st.grad2d.copy_(torch.arange(5.0))
    st.count.copy_(torch.tensor([1.0, 0.0, 2.0, 4.0, 1.0]))
    st.max_radii.copy_(torch.arange(5.0) / 10)
    assert st.mean_grad().tolist() == [0.0, 1.0, 1.0, 0.75, 4.0]   # count 0: clamped to 1
    kept = st.select(torch.tensor([True, False, True, False, True]))
    assert kept.n == 3 and kept.grad2d.tolist() == [0.0, 2.0, 4.0] and kept.count.tolist() == [1.0, 2.0, 1.0]
    assert kept.max_radii.tolist() == pytest.approx([0.0, 0.2, 0.4])
    cloned = st.select(torch.tensor([3, 3, 0]))
    assert cloned.grad2d.tolist() == [3.0, 3.0, 0.0] and cloned.count.tolist() == [4.0, 4.0, 1.0]
    assert st.n == 5   # select copies
    kept.append(2)
    assert kept.n == 4 + 1 and kept.grad2d.tolist() == [0.0, 2.0, 4.0, 0.0, 0.0]
    assert kept.count.tolist() == [1.0, 2.0, 1.0, 0.0, 0.0] and kept.max_radii[3:].tolist() == [0.0, 0.0]
    kept.reset()
    assert all((t == 0).all() and t.numel() == 5 for t in (kept.grad2d, kept.count, kept.max_radii))


def test_densify_stats_check_rejects_what_the_kernel_cannot_write():
    st = DensifyStats(4, "cpu")
    st.check(4, torch.device("cpu"))
    with pytest.raises(ValueError, match=r"\[5\]"):
        st.check(5, torch.device("cpu"))
    with pytest.raises(ValueError, match="float32"):
        DensifyStats(0, _buffers=(torch.zeros(4, dtype=torch.float64), st.count, st.max_radii)).check(4, torch.device("cpu"))
    with pytest.raises(ValueError, match="contiguous"):
        DensifyStats(0, _buffers=(torch.zeros(8)[::2], st.count, st.max_radii)).check(4, torch.device("cpu"))
    with pytest.raises(ValueError, match="meta"):
        DensifyStats(0, _buffers=(st.grad2d, st.count, torch.zeros(4, device="meta"))).check(4, torch.device("cpu"))


def test_densify_entry_points_validate_their_arguments():
    """Both entry points check their arguments before touching the device (fake non-null pointers are never
    dereferenced on these paths), as test_host_logic.py's validation tests do for their neighbours."""
    L = _hip.load()
    P = ctypes.c_void_p(0x1000)
    N = ctypes.c_int64(10)
    OK, INVALID = 0, 1
    err = lambda: L.ms_last_error_string().decode()

    assert L.ms_densify_stats_update(ctypes.c_int64(-1), 8, 8, P, P, P, P, P, None) == INVALID and "N < 0" in err()
    assert L.ms_densify_stats_update(N, 8, 8, None, P, P, P, P, None) == INVALID and "null" in err()
    assert L.ms_densify_stats_update(N, 8, 8, P, P, P, None, P, None) == INVALID and "null" in err()
    assert L.ms_densify_stats_update(N, 0, 8, P, P, P, P, P, None) == INVALID and "image" in err()
    assert L.ms_densify_stats_update(N, 8, 8, ctypes.c_void_p(0x1004), P, P, P, P, None) == INVALID \
        and "aligned" in err()
    assert L.ms_densify_stats_update(N, 8, 8, P, P, P, ctypes.c_void_p(0x1002), P, None) == INVALID \
        and "aligned" in err()
    assert L.ms_densify_stats_update(ctypes.c_int64(0), 8, 8, None, None, None, None, None, None) == OK

    def fin(n=N, rows=P, stats=(P, P, P), W=8, cdim=3, quats=P):
        return L.ms_render_bwd_finish_densify(n, P, P, 1, quats, P, cdim, P, 1., 1., 0., 0., W, 8, .3, rows, P, P, P, P, P,
                                              .01, 100., *stats, None)
    assert fin(n=ctypes.c_int64(-1)) == INVALID and "bad argument" in err()
    assert fin(stats=(P, None, P)) == INVALID and "bad argument" in err()
    assert fin(cdim=4) == INVALID and "bad argument" in err()
    assert fin(rows=None) == INVALID and "null" in err()
    assert fin(W=0) == INVALID and "camera" in err()
    assert fin(quats=ctypes.c_void_p(0x1004)) == INVALID and "aligned" in err()
    assert fin(stats=(P, P, ctypes.c_void_p(0x1001))) == INVALID and "aligned" in err()
    assert fin(n=ctypes.c_int64(0), rows=None) == OK   # N == 0 is a no-op
