"""CPU only: how far a float32 SEPARABLE evaluation of the photometric loss (two 11-tap passes, the summation order of
csrc/loss.hip) lies from the float64 definition, next to the float32 2-D definition's own distance (e32) -- the
stand-in that checks the factor 4 of tests/test_hip_loss.py before any kernel runs ("Photometric loss").

    python scripts/loss_f32_margin.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mojosplat_amd.loss import C1, C2, gaussian_window, photometric_loss_torch  # noqa: E402

EPS32 = torch.finfo(torch.float32).eps


def separable_loss(x, y, lam):
    """The definition with w * t evaluated as a horizontal then a vertical 11-tap pass, in x's dtype."""
    xn, yn = (t[None].permute(0, 3, 1, 2) for t in (x, y))
    C = xn.shape[1]
    g = gaussian_window(x.dtype)
    conv = torch.nn.functional.conv2d
    w = lambda t: conv(conv(t, g.view(1, 1, 1, 11).expand(C, 1, 1, 11), padding=(0, 5), groups=C),
                       g.view(1, 1, 11, 1).expand(C, 1, 11, 1), padding=(5, 0), groups=C)
    mx, my = w(xn), w(yn)
    sxx, syy, sxy = w(xn * xn) - mx * mx, w(yn * yn) - my * my, w(xn * yn) - mx * my
    ssim_v = (((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))).mean()
    l1 = (x - y).abs().mean()
    return (1 - lam) * l1 + lam * (1 - ssim_v), l1.detach(), ssim_v.detach()


def inputs(kind, H, W, C=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return torch.rand(H, W, C, generator=g), torch.rand(H, W, C, generator=g)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(0.031 * (c + 1) * xx + 0.5 * c) * torch.cos(0.023 * (c + 2) * yy)
                        for c in range(C)], -1)
    if kind == "smooth":
        return base, base + 0.02 * torch.randn(H, W, C, generator=g)
    if kind == "blobs-on-black":   # stands in for a render on a black background: large exactly-zero regions
        mask = ((torch.sin(0.02 * xx) * torch.sin(0.03 * yy)) > 0.3).float()[..., None]
        return base * mask, (base + 0.05 * torch.randn(H, W, C, generator=g)).clamp(0, 1) * mask
    x = torch.rand(H, W, C, generator=g)
    return x, x.clone()


def evaluate(fn, x, y, dtype, lam=0.2):
    xd = x.to(dtype).clone().requires_grad_(True)
    loss, l1, ssim_v = fn(xd, y.to(dtype), lam)
    loss.backward()
    return torch.stack([loss.detach(), l1, ssim_v]).double(), xd.grad.double()


def main():
    worst = 0.0
    for kind in ("noise", "smooth", "blobs-on-black", "same"):
        for H, W in ((170, 250), (360, 640), (1080, 1920)):
            x, y = inputs(kind, H, W)
            v64, g64 = evaluate(lambda a, b, l: photometric_loss_torch(a, b, l, return_parts=True), x, y, torch.float64)
            v32, g32 = evaluate(lambda a, b, l: photometric_loss_torch(a, b, l, return_parts=True), x, y, torch.float32)
            vs, gs = evaluate(separable_loss, x, y, torch.float32)
            e32, esep = (v32 - v64).abs(), (vs - v64).abs()
            need_v = max(max(0.0, float(esep[k]) - 4 * EPS32 * abs(float(v64[k]))) / max(float(e32[k]), 1e-300) for k in range(3))
            r32, rsep, ref = float((g32 - g64).norm()), float((gs - g64).norm()), float(g64.norm())
            m32, msep, mref = float((g32 - g64).abs().max()), float((gs - g64).abs().max()), float(g64.abs().max())
            need_g = max(max(0.0, rsep - 4 * EPS32 * ref) / max(r32, 1e-300), max(0.0, msep - 4 * EPS32 * mref) / max(m32, 1e-300))
            need_v = need_v if need_v < 1e100 else float("inf")
            print(f"{kind:15s} {H}x{W}: value e32 {[f'{float(v):.2e}' for v in e32]} separable {[f'{float(v):.2e}' for v in esep]} "
                  f"| grad L2 f32 {r32:.3e} separable {rsep:.3e} (|g64| {ref:.3e}) max f32 {m32:.3e} separable {msep:.3e} "
                  f"| factor needed: value {need_v:.2f} gradient {need_g:.2f}")
            worst = max(worst, need_g, need_v if need_v != float("inf") else 0.0)
    print(f"largest factor the separable stand-in needs: {worst:.2f} (tests/test_hip_loss.py allows 4)")


if __name__ == "__main__":
    main()
