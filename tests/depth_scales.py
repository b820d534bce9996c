"""Depth scales and inverse-depth variances other than TUM's: what the tests of those two Config fields share (no test lives here).

The synthetic scenes quantise depth at 5000 units per metre. requantise() restates such a depth map at another scale, so that the scene
stays geometrically consistent with the configured scale: d' = clip(floor(d * scale / 5000 + 0.5), 1, 65535) where d > 0, 0 where d == 0.

  5000    control
  1000    millimetres, what most sensors deliver
  256     a power of two: 256 / x is exact for every power of two x, and the ties of to_depth sit elsewhere than at 5000
  6553.5  not an integer
  3.0     a scene of about 2 m quantises to about 6 levels: single known children and equal children dominate the fusion
  30000   the far end of the scenes (about 2.2 m) sits at the 65535 clamp (2.18 m): a little further and to_depth saturates in the products

Every scale is exact in float32. The variances: the default, one that makes every weight 1, and one that is not a power of ten."""
import numpy as np

SCENE_SCALE = 5000.0
SCALES = (5000.0, 1000.0, 256.0, 6553.5, 3.0, 30000.0)
VARIANCES = (1e-4, 1.0, 3e-7)
BLOCKY = 1 << 63  # seeds with the top bit set render the piecewise-constant texture the DSO selector needs

# Every scale with a non-default variance at least once, every variance in every candidate mode (the grid is used once per mode).
GRID = ((5000.0, 1e-4), (5000.0, 3e-7), (1000.0, 1.0), (256.0, 3e-7), (6553.5, 1.0), (3.0, 3e-7), (3.0, 1e-4), (30000.0, 1.0), (30000.0, 1e-4))
assert {s for s, _ in GRID} == set(SCALES) and {v for _, v in GRID} == set(VARIANCES)
assert all(any(v != 1e-4 for s, v in GRID if s == scale) for scale in SCALES)
assert all(np.float32(s) == s for s in SCALES)


def scale_id(scale, variance=None):
    s = f"s{scale:g}"
    return s if variance is None else f"{s}-v{variance:g}"


def requantise(depth, scale):
    """uint16 depth maps at 5000 units per metre (or an int16 array holding that payload) -> the same scene at `scale` units per metre."""
    d = np.ascontiguousarray(depth)
    if d.dtype == np.int16:
        d = d.view(np.uint16)
    assert d.dtype == np.uint16
    q = np.clip(np.floor(d.astype(np.float64) * float(scale) / SCENE_SCALE + 0.5), 1, 65535).astype(np.uint16)
    return np.where(d > 0, q, np.uint16(0)).astype(np.uint16)


def requantise_tensor(depth, scale):
    """requantise() for an int16 device tensor holding the u16 payload -> a new tensor on the same device."""
    import torch
    return torch.from_numpy(requantise(depth.cpu().numpy(), scale).view(np.int16)).to(depth.device)
