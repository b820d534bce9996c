"""The per-pixel merge of depth fusion on the host (vors_fuse_depth_pixels, lie.h fuse_depth_pixel): needs no GPU.

The numpy statement below is the rule table of include/vors_hip.h in float32, one IEEE operation per numpy operation and in the header's
expression order (the library is built without contraction), with to_depth as test_to_depth_host.py restates it. Equality with the library
must be exact: depths, weights and the six counters.

Cases are built, not hoped for: every test asserts that the cases it is about occur."""
import numpy as np
import pytest

import vors_amd as V
from test_to_depth_host import restated as to_depth_np

SCALE = 5000.0
F32 = np.float32
EMPTY = np.uint64(V.ZKEY_EMPTY)
AGREE, FRONT, BEHIND, MEASURED, FILLED, NOTHING = range(6)


def make_keys(z, src):
    """bits(z) << 32 | src; src < 0 = nothing landed."""
    z, src = np.asarray(z, F32), np.asarray(src, np.int64)
    key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.where(src >= 0, src, 0).astype(np.uint64)
    return np.where(src >= 0, key, EMPTY)


def restated(scale, tol_m, key, d, kf_weight=None, max_weight=255, fill_min_weight=0):
    """-> (depth, weight, case) per pixel."""
    key, d = np.asarray(key, np.uint64).ravel(), np.asarray(d, np.uint16).ravel()
    scale, tol = F32(scale), F32(tol_m)
    has_p, has_m = key != EMPTY, d != 0
    zp = (key >> np.uint64(32)).astype(np.uint32).view(F32)
    src = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
    wk = np.ones(key.shape, np.int64)
    if kf_weight is not None:
        wk[has_p] = np.asarray(kf_weight, np.uint8).ravel()[src[has_p]]
    df, wf = d.astype(F32), wk.astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = zp - df / scale
        mean = (wf * (F32(1.0) / zp) + scale / df) / (wf + F32(1.0))
        agree = has_p & has_m & (np.abs(r) <= tol)
        front = has_p & has_m & (r < -tol)
        behind = has_p & has_m & (r > tol)
        measured = ~has_p & has_m
        filled = has_p & ~has_m & (fill_min_weight > 0) & (wk >= fill_min_weight)
        case = np.full(key.shape, NOTHING)
        depth, weight = np.zeros(key.shape, np.uint16), np.zeros(key.shape, np.int64)
        for mask, k in ((agree, AGREE), (front, FRONT), (behind, BEHIND), (measured, MEASURED), (filled, FILLED)):
            case[mask] = k
        depth[agree] = to_depth_np(scale, mean[agree])
        weight[agree] = np.minimum(wk[agree] + 1, max_weight)
        keep = front | behind | measured
        depth[keep] = d[keep]
        weight[keep] = 1
        depth[filled] = to_depth_np(scale, (F32(1.0) / zp)[filled])
        weight[filled] = wk[filled]
    weight[depth == 0] = 0   # a fused depth that rounds to 0 carries no weight: depth 0 <=> weight 0
    return depth, weight.astype(np.uint8), case


def check(tol_m, key, d, kf_weight=None, max_weight=255, fill_min_weight=0, scale=SCALE):
    depth, weight, counts = V.fuse_depth_pixels(scale, tol_m, key, d, kf_weight, max_weight, fill_min_weight)
    wd, ww, case = restated(scale, tol_m, key, d, kf_weight, max_weight, fill_min_weight)
    assert depth.dtype == np.uint16 and weight.dtype == np.uint8 and depth.shape == np.shape(key) and counts.shape == (6,)
    bad = np.nonzero((depth.ravel() != wd) | (weight.ravel() != ww))[0]
    assert bad.size == 0, (bad[:5], depth.ravel()[bad[:5]], wd[bad[:5]], weight.ravel()[bad[:5]], ww[bad[:5]], case[bad[:5]])
    assert counts.tolist() == np.bincount(case, minlength=6).tolist()
    assert int(counts.sum()) == np.size(key)
    assert ((depth == 0) == (weight == 0)).all()
    return depth.ravel(), weight.ravel(), case, counts


def random_pixels(rng, n, n_kf, scale=SCALE):
    """Depths over the whole range (0, 1 and 65535 among them), predictions near the measurement, far from it, and missing."""
    d = rng.integers(1, 65536, n).astype(np.uint16)
    d[rng.random(n) < 0.25] = 0
    d[:8] = [1, 1, 65535, 65535, 1, 65535, 0, 0]
    near = d.astype(F32) / F32(scale) + rng.normal(0, 0.012, n).astype(F32)
    far = rng.uniform(0.05, 14.0, n).astype(F32)
    z = np.where(rng.random(n) < 0.6, near, far).astype(F32)
    z = np.where((z > 0) & (d != 0), z, far).astype(F32)
    src = rng.integers(0, n_kf, n)
    src[rng.random(n) < 0.3] = -1
    src[4:8] = [-1, -1, 3, -1]
    return make_keys(z, src), d


def test_random_pixels_against_the_table():
    rng = np.random.default_rng(21)
    n, n_kf = 6000, 5000
    key, d = random_pixels(rng, n, n_kf)
    w = rng.integers(0, 256, n_kf).astype(np.uint8)
    w = np.where(rng.random(n_kf) < 0.3, rng.integers(0, 5, n_kf), w).astype(np.uint8)   # small weights and zeros among them
    for weights in (w, None):
        for max_weight, fill in ((255, 0), (255, 1), (8, 3), (1, 200), (100, 128)):
            _, weight, case, counts = check(0.01, key, d, weights, max_weight, fill)
            assert (counts[[AGREE, FRONT, BEHIND, MEASURED, NOTHING]] > 0).all(), counts
            assert (counts[FILLED] > 0) == (fill > 0 and (weights is not None or fill == 1)), (max_weight, fill, counts)
            assert weight.max() <= max(max_weight, 255 if (fill and weights is not None) else 1)
    # an image-shaped call gives image-shaped maps
    depth, weight, _ = V.fuse_depth_pixels(SCALE, 0.01, key.reshape(60, 100), d.reshape(60, 100), w)
    assert depth.shape == weight.shape == (60, 100)
    # int64 / int16 payloads (what the device tensors hold) are taken as they are
    again = V.fuse_depth_pixels(SCALE, 0.01, key.view(np.int64), d.view(np.int16), w)
    assert (again[0].ravel() == depth.ravel()).all() and (again[1].ravel() == weight.ravel()).all()


def test_residual_exactly_at_the_tolerance():
    # d = 5000 at scale 5000 is 1.0 exactly; 1.25 and 0.75 give r = +-0.25 exactly, their float neighbours lie on either side
    up, dn = F32(1.25), F32(0.75)
    z = np.array([up, np.nextafter(up, F32(2)), np.nextafter(up, F32(0)), dn, np.nextafter(dn, F32(0)), np.nextafter(dn, F32(2))], F32)
    key, d = make_keys(z, np.arange(6)), np.full(6, 5000, np.uint16)
    _, weight, case, _ = check(0.25, key, d)
    assert case.tolist() == [AGREE, BEHIND, AGREE, AGREE, FRONT, AGREE] and weight.tolist() == [2, 1, 2, 2, 1, 2]
    # tol_m = 0: only an exact match agrees
    _, _, case, _ = check(0.0, make_keys(np.array([1.0, np.nextafter(F32(1), F32(2)), np.nextafter(F32(1), F32(0))], F32), np.arange(3)),
                          np.full(3, 5000, np.uint16))
    assert case.tolist() == [AGREE, BEHIND, FRONT]
    # any pixel's own |r| as the tolerance puts that pixel on the boundary
    rng = np.random.default_rng(3)
    dd = rng.integers(1, 65536, 500).astype(np.uint16)
    zz = (dd.astype(F32) / F32(SCALE) + rng.normal(0, 0.01, 500).astype(F32)).astype(F32)
    zz = np.where(zz > 0, zz, F32(0.5))
    kk = make_keys(zz, np.arange(500))
    for i in range(0, 500, 25):
        tol = np.abs(zz[i] - F32(dd[i]) / F32(SCALE))
        _, _, case, _ = check(float(tol), kk, dd)
        assert case[i] == AGREE and (case != AGREE).any()


def test_weight_saturation_fill_gate_and_extreme_depths():
    w = np.array([1, 2, 7, 8, 9, 254, 255, 0], np.uint8)
    src = np.arange(8)
    d = np.full(8, 10000, np.uint16)
    key = make_keys(np.full(8, 2.0, F32), src)
    for max_weight, want in ((255, [2, 3, 8, 9, 10, 255, 255, 1]), (8, [2, 3, 8, 8, 8, 8, 8, 1]), (1, [1] * 8)):
        depth, weight, case, _ = check(0.01, key, d, w, max_weight)
        assert (case == AGREE).all() and weight.tolist() == want and (depth == 10000).all()
    # the fill gate: fill_min_weight 0 never fills; at wk it fills, at wk + 1 it does not
    none = np.zeros(8, np.uint16)
    for fill, want in ((0, [NOTHING] * 8), (1, [FILLED] * 7 + [NOTHING]), (8, [NOTHING] * 3 + [FILLED] * 4 + [NOTHING]),
                       (9, [NOTHING] * 4 + [FILLED] * 3 + [NOTHING]), (255, [NOTHING] * 6 + [FILLED, NOTHING])):
        depth, weight, case, _ = check(0.01, key, none, w, 255, fill)
        assert case.tolist() == want, fill
        assert (depth[case == FILLED] == 10000).all() and (weight[case == FILLED] == w[case == FILLED]).all()
    # without a weight plane every point weighs 1: fill_min_weight 1 fills, 2 does not
    assert (check(0.01, key, none, None, 255, 1)[2] == FILLED).all() and (check(0.01, key, none, None, 255, 2)[2] == NOTHING).all()
    # a filled pixel carries to_depth(scale, 1 / Z'), the bits of d_pred_depth, over the whole range and beyond the saturation
    z = np.array([1e-5, 1e-4, 2e-4, 0.0123, 1.0, 13.106, 13.107, 13.2, 1e6], F32)
    depth, weight, case, _ = check(0.01, make_keys(z, np.arange(9)), np.zeros(9, np.uint16), None, 255, 1)
    assert (case == FILLED).all() and (depth == to_depth_np(SCALE, F32(1.0) / z)).all()
    assert depth[0] == 0 and weight[0] == 0 and depth[-1] == 65535 and weight[-1] == 1   # nearer than half a unit: no depth, no weight
    # depths 1 and 65535 measured: agreeing, conflicting and alone
    z = np.array([1 / 5000.0, 65535 / 5000.0, 5.0, 5.0, 1 / 5000.0, 65535 / 5000.0], F32)
    d = np.array([1, 65535, 1, 65535, 1, 65535], np.uint16)
    depth, weight, case, _ = check(1e-3, make_keys(z, [0, 1, 2, 3, -1, -1]), d)
    assert case.tolist() == [AGREE, AGREE, BEHIND, FRONT, MEASURED, MEASURED]
    assert depth.tolist() == [1, 65535, 1, 65535, 1, 65535] and weight.tolist() == [2, 2, 1, 1, 1, 1]
    # a NaN prediction (which the device never writes) agrees and conflicts with nothing; "filled" with it is depth 0, weight 0
    depth, weight, case, _ = check(0.01, make_keys(np.array([np.nan, np.nan], F32), [0, 1]), np.array([5000, 0], np.uint16), None, 255, 1)
    assert case.tolist() == [NOTHING, FILLED] and depth.tolist() == [0, 0] and weight.tolist() == [0, 0]


def test_the_mean_is_taken_in_inverse_depth():
    # 1 m with weight 3 and 2 m measured: inverse depths 1 and 0.5, mean (3 + 0.5) / 4 = 0.875 -> 5000 / 0.875 = 5714.29
    depth, weight, counts = V.fuse_depth_pixels(SCALE, 2.0, make_keys(np.array([1.0], F32), [0]), np.array([10000], np.uint16),
                                                np.array([3], np.uint8))
    assert depth.tolist() == [5714] and weight.tolist() == [4] and counts.tolist() == [1, 0, 0, 0, 0, 0]


def test_refusals():
    lib = V.lib()
    key, d = make_keys(np.array([1.0, 1.0], F32), [0, 4]), np.array([5000, 5000], np.uint16)
    w = np.ones(5, np.uint8)
    depth, weight, counts = np.full(2, 7, np.uint16), np.full(2, 7, np.uint8), np.full(6, 7, np.uint32)

    def call(scale=SCALE, tol=0.01, max_weight=255, fill=0, n=2, k=key, dd=d, ww=w, n_kf=5):
        return lib.vors_fuse_depth_pixels(scale, tol, max_weight, fill, n, V._ptr(k), V._ptr(dd), V._ptr(ww), n_kf, V._ptr(depth), V._ptr(weight),
                                          V._ptr(counts))

    refused = [(dict(k=None), "NULL"), (dict(dd=None), "NULL"), (dict(tol=-1e-3), "tol_m"), (dict(tol=float("nan")), "tol_m"),
               (dict(max_weight=0), "max_weight"), (dict(max_weight=256), "max_weight"), (dict(fill=-1), "fill_min_weight"),
               (dict(fill=256), "fill_min_weight"), (dict(scale=0.0), "depth_scale"), (dict(n_kf=4), "source pixel"),
               (dict(n_kf=4, ww=None), "source pixel"), (dict(n_kf=0), "source pixel")]
    for bad, word in refused:
        assert call(**bad) == -1, bad
        assert word.encode() in lib.vors_last_error(), (bad, lib.vors_last_error())
    assert (depth == 7).all() and (weight == 7).all() and (counts == 7).all()   # a refusal writes nothing
    assert call() == 0 and depth.tolist() == [5000, 5000] and weight.tolist() == [2, 2] and counts.tolist() == [2, 0, 0, 0, 0, 0]
    assert call(n=0) == 0 and counts.tolist() == [0] * 6
    # an empty key names no source: legal whatever n_kf_pixels is; each output is nullable
    empty = np.full(2, EMPTY, np.uint64)
    assert call(k=empty, n_kf=0, ww=None) == 0 and counts.tolist() == [0, 0, 0, 2, 0, 0]
    assert lib.vors_fuse_depth_pixels(SCALE, 0.01, 255, 0, 2, V._ptr(key), V._ptr(d), None, 5, None, None, None) == 0
    with pytest.raises(V.VorsError):
        V.fuse_depth_pixels(SCALE, 0.01, key, d[:1])
    with pytest.raises(V.VorsError):
        V.fuse_depth_pixels(SCALE, 0.01, key, d, w[:3])   # the key of pixel 1 names source 4
