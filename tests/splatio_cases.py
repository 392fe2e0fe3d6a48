"""The scenes both splatio test files run on (tests/test_splatio_cpu.py, tests/test_hip_splatio.py): seeded random ones at
sizes around the 256 Gaussians of a chunk, and one built by hand whose rows hit the formats' edge cases."""
import torch

NS = (1, 255, 256, 257, 700)
KS = (1, 4, 9, 16)
KEYS = ("means3d", "scales", "quats", "opacities", "features")


def seeded_scene(N, K, seed=0, device="cpu"):
    """Logit opacities, log-scales around -1, SH features of which a few per cent leave the byte range [-4, 4)."""
    g = torch.Generator().manual_seed(1000 * seed + 16 * N + K)
    r = lambda *s: torch.randn(s, generator=g)
    p = {"means3d": r(N, 3), "scales": r(N, 3) - 1.0, "quats": r(N, 4), "opacities": 2.0 * r(N), "features": 1.5 * r(N, K, 3)}
    return {k: v.to(device) for k, v in p.items()}


# rows of the hand-built scene (N = 300: a full chunk and one of 44 rows; LINEAR opacities; K = 4)
ROW_NEGATIVE_LARGEST, ROW_EQUAL_PAIR, ROW_EQUAL_ALL, ROW_SCALE_LOW, ROW_SCALE_HIGH, ROW_SH, ROW_OPACITY_0, ROW_OPACITY_1 = range(8)
HAND_N, HAND_K = 300, 4


def hand_built_scene(device="cpu"):
    g = torch.Generator().manual_seed(77)
    N, K = HAND_N, HAND_K
    p = {"means3d": torch.randn((N, 3), generator=g), "scales": torch.randn((N, 3), generator=g) - 1.0,
         "quats": torch.randn((N, 4), generator=g), "opacities": 0.05 + 0.9 * torch.rand((N,), generator=g),
         "features": torch.randn((N, K, 3), generator=g)}
    p["means3d"][256:] = torch.tensor([0.25, -1.5, 3.0])                 # the second chunk: one position (hi - lo < 1e-5 -> word 0)
    p["quats"][ROW_NEGATIVE_LARGEST] = torch.tensor([0.1, -0.9, 0.2, 0.3])   # the largest component is negative: all four change sign
    p["quats"][ROW_EQUAL_PAIR] = torch.tensor([0.1, 0.7, -0.7, 0.1])     # |x| == |y|: the first index (1) wins
    p["quats"][ROW_EQUAL_ALL] = torch.tensor([-0.5, 0.5, 0.5, 0.5])      # all equal: index 0 wins, and it is negative
    p["scales"][ROW_SCALE_LOW] = torch.tensor([-30.0, -1.0, -1.0])       # the clamp to [-20, 20]
    p["scales"][ROW_SCALE_HIGH] = torch.tensor([-1.0, 30.0, -1.0])
    p["features"][ROW_SH, 1, :] = torch.tensor([-5.0, 4.0, 3.99])        # the byte clamp: 0, 255 (from 256), 255
    p["opacities"][ROW_OPACITY_0] = 0.0                                  # byte 0
    p["opacities"][ROW_OPACITY_1] = 1.0                                  # byte 255
    return {k: v.to(device) for k, v in p.items()}
