"""The host helpers at depth scales other than 5000 (tests/depth_scales.py gives the scales and why): needs no GPU. The device tests of
tests/test_gpu_depth_scale*.py lean on these helpers, so they are pinned here at the same scales.

  1. vors_to_depth / vors_from_depth at every scale against a float64 statement of the rule: ONE float32 division, round half away from
     zero, saturate at 65535, Unknown <-> 0. The float64 statement: the float32 quotient of two float32 numbers is the float64 quotient
     rounded once more (53 >= 2 * 24 + 2 bits: the double rounding is innocuous for a division), and floor(q + 0.5) is exact in float64
     for every float32 q below 2^52. The ties of each scale are enumerated in the test:
       * the real quotient scale / x is k + 0.5 only for x = 2 scale / (2k + 1), a float32 only when 2k + 1 divides the odd part m of
         2 scale = m 2^a (5000: 625; 1000: 125; 256: 1; 6553.5: 13107 = 3 * 17 * 257; 3: 3; 30000: 1875);
       * the FLOAT32 quotient is k + 0.5 for many more x: wherever the real quotient rounds to it. For every k up to the saturation the
         float32 nearest 2 scale / (2k + 1) and its two neighbours are tried, and those whose quotient is exactly k + 0.5 must give k + 1.
  2. vors_fuse_depth_pixels, vors_render_points_host and vors_depth_normals_host at 1000, 256 and 30000 against the numpy restatements of
     test_fuse_depth_host.py, test_render_points_host.py and test_normals_host.py, with the scale passed through."""
import numpy as np
import pytest

import vors_amd as V
import test_fuse_depth_host as FH
import test_normals_host as NH
import test_render_points_host as RH
from depth_scales import SCALES, scale_id

F32 = np.float32
OPERATOR_SCALES = (1000.0, 256.0, 30000.0)
ODD_PART = {5000.0: 625, 1000.0: 125, 256.0: 1, 6553.5: 13107, 3.0: 3, 30000.0: 1875}   # of 2 * scale
SCALE = pytest.mark.parametrize("scale", SCALES, ids=scale_id)
OPERATOR_SCALE = pytest.mark.parametrize("scale", OPERATOR_SCALES, ids=scale_id)


def to_depth64(scale, x):
    """The rule in float64 (see above) -> uint16."""
    x = np.asarray(x, F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = (np.float64(F32(scale)) / x.astype(np.float64)).astype(F32).astype(np.float64)   # the float32 quotient, exactly
        r = np.floor(q + 0.5)                                                                 # round half away from zero for q >= 0
        r = np.where(np.abs(q) >= 2.0 ** 52, q, r)
    out = np.zeros(x.shape, np.uint16)                                                        # NaN, zero, negative: 0
    big, mid = r >= 65535.0, (r > 0) & (r < 65535.0)
    out[big] = 65535
    out[mid] = r[mid].astype(np.uint16)
    return out


def check_to_depth(scale, x):
    x = np.asarray(x, F32)
    got, want = V.to_depth(scale, x), to_depth64(scale, x)
    bad = np.nonzero(got != want)[0]
    assert got.dtype == np.uint16 and bad.size == 0, (scale, x[bad[:5]], got[bad[:5]], want[bad[:5]])
    return got


def odd_divisors(m):
    return [d for d in range(1, m + 1, 2) if m % d == 0]


# ------------------------------------------------------------------------------------------------------------ 1
@SCALE
def test_to_depth_random_inverse_depths(scale):
    rng = np.random.default_rng(7)
    # inverse depths of depths from half a unit to beyond the saturation, uniform and log-uniform
    lo, hi = scale / 80000.0, scale / 0.4
    got = check_to_depth(scale, np.concatenate([rng.uniform(lo, hi, 20000), np.exp(rng.uniform(np.log(lo), np.log(hi), 20000))]).astype(F32))
    assert (got == 65535).any() and (got == 0).any() and ((got > 0) & (got < 65535)).any()


@SCALE
def test_to_depth_every_tie(scale):
    s = F32(scale)
    assert float(s) == scale and float(s) * 2 == ODD_PART[scale] * 2.0 ** round(np.log2(2 * scale / ODD_PART[scale]))
    # the real ties: 2k + 1 an odd divisor of the odd part of 2 scale
    div = np.array(odd_divisors(ODD_PART[scale]), np.float64)
    x = (2.0 * scale / div).astype(F32)
    assert (x.astype(np.float64) * div == 2.0 * scale).all(), "these quotients are exact"
    k = ((div - 1) / 2).astype(np.int64)
    assert (s / x == (k + 0.5).astype(F32)).all()
    assert (check_to_depth(scale, x) == np.minimum(k + 1, 65535)).all()    # away from zero, not to even
    assert (check_to_depth(scale, -x) == 0).all()
    # the float32 ties: for every k the float32 nearest 2 scale / (2k + 1) and its neighbours
    k = np.arange(0, 65540, dtype=np.int64)
    x0 = (2.0 * scale / (2 * k + 1)).astype(F32)
    x = np.concatenate([np.nextafter(x0, F32(0)), x0, np.nextafter(x0, F32(np.inf))])
    kk = np.concatenate([k, k, k])
    tie = (s / x) == (kk + 0.5).astype(F32)
    tie &= kk < 2 ** 22   # (k + 0.5 is a float32 itself)
    assert int(tie.sum()) >= len(div) and set(div.astype(np.int64) // 2) <= set(kk[tie].tolist()), "the real ties are among them"
    assert int(tie.sum()) > 1000, f"only {int(tie.sum())} float32 ties at scale {scale}"
    got = check_to_depth(scale, x)
    assert (got[tie] == np.minimum(kk[tie] + 1, 65535)).all()
    assert (kk[tie] >= 65534).any() and (kk[tie] < 100).any(), "ties from the first units up to the saturation"
    # depth units that are powers of two at scale 256: the quotient is exact, nothing to round
    if scale == 256.0:
        p2 = (2.0 ** np.arange(-8, 9)).astype(F32)
        assert (check_to_depth(scale, p2) == np.clip(256.0 / p2, 0, 65535).astype(np.uint16)).all()


@SCALE
def test_to_depth_special_values_and_saturation(scale):
    inf, nan = F32(np.inf), F32(np.nan)
    x = np.array([0.0, -0.0, -1.0, -1e-30, -1e30, nan, -nan, inf, -inf, 1e-38, 1e-45, 3e38, 1e30], F32)
    assert check_to_depth(scale, x).tolist() == [65535, 0, 0, 0, 0, 0, 0, 0, 0, 65535, 65535, 0, 0]
    # around the saturation: a quotient of 65534.5 rounds up to 65535, nothing beyond wraps
    x0 = F32(scale / 65535.5)
    near = [x0]
    for _ in range(100):
        near.append(np.nextafter(near[-1], F32(0)))
    lo = x0
    for _ in range(600):   # (a step of x moves the quotient by about 2^-8 here: 600 steps reach below 65534.5)
        lo = np.nextafter(lo, F32(np.inf))
        near.append(lo)
    near = np.array(near, F32)
    q = F32(scale) / near
    assert (q >= 65535.5).any() and (q < 65534.5).any()
    got = check_to_depth(scale, near)
    assert (got[q >= 65534.5] == 65535).all() and (got[q < 65534.5] < 65535).all() and (got == 65534).any()
    beyond = np.array([scale / 65536.0, scale / 65537.0, scale / 70000.0, scale / 131071.0, scale / 131072.0, scale / 1e6, scale / 1e9,
                       scale / 2.0 ** 23, scale / 2.0 ** 24, scale / 2.0 ** 31, scale / 2.0 ** 32, scale / 2.0 ** 33], F32)
    assert (check_to_depth(scale, beyond) == 65535).all()        # (a cast without the clamp wraps 65536 to 0 and 70000 to 4464)
    # below one unit: 0.5 rounds up, the float just below it rounds down
    half = F32(2.0 * scale)
    assert check_to_depth(scale, np.array([half, np.nextafter(half, F32(np.inf))], F32)).tolist() == [1, 0]


@SCALE
def test_from_depth_and_the_round_trip(scale):
    d = np.arange(0, 65536, dtype=np.uint16)
    f = V.from_depth(scale, d)
    assert f.dtype == F32 and np.isnan(f[0]) and np.isfinite(f[1:]).all()                      # 0 is Unknown
    want = (np.float64(F32(scale)) / d[1:].astype(np.float64)).astype(F32)                      # one float32 division
    assert (f[1:].view(np.uint32) == want.view(np.uint32)).all()
    back = check_to_depth(scale, f)
    assert back[0] == 0 and (back[1:] == d[1:]).all()                                           # Unknown is encoded with 0
    again = V.from_depth(scale, back)
    assert (again[1:].view(np.uint32) == f[1:].view(np.uint32)).all() and np.isnan(again[0])


# ------------------------------------------------------------------------------------------------------------ 2: fusion
@OPERATOR_SCALE
def test_fuse_depth_pixels_random_pixels_against_the_table(scale):
    rng = np.random.default_rng(21)
    n, n_kf = 6000, 5000
    key, d = FH.random_pixels(rng, n, n_kf, scale)
    w = rng.integers(0, 256, n_kf).astype(np.uint8)
    w = np.where(rng.random(n_kf) < 0.3, rng.integers(0, 5, n_kf), w).astype(np.uint8)
    for weights in (w, None):
        for max_weight, fill in ((255, 0), (255, 1), (8, 3), (1, 200), (100, 128)):
            depth, weight, case, counts = FH.check(0.01, key, d, weights, max_weight, fill, scale=scale)
            assert (counts[[FH.AGREE, FH.FRONT, FH.BEHIND, FH.MEASURED, FH.NOTHING]] > 0).all(), counts
            assert (counts[FH.FILLED] > 0) == (fill > 0 and (weights is not None or fill == 1)), (max_weight, fill, counts)
            if counts[FH.FILLED] > 0:   # predictions up to 14 m are filled in: beyond 65535 / scale metres the depth saturates
                assert (depth[case == FH.FILLED] == 65535).any() == (14.0 * scale > 65535.5), scale


@OPERATOR_SCALE
def test_fuse_depth_pixels_tolerance_mean_and_extreme_depths(scale):
    s = F32(scale)
    # d = scale units is 1.0 m exactly where the scale is an integer below 65536; 1.25 and 0.75 give r = +-0.25 exactly
    unit = int(scale) if scale < 65536 else None
    if unit is not None:
        up, dn = F32(1.25), F32(0.75)
        z = np.array([up, np.nextafter(up, F32(2)), np.nextafter(up, F32(0)), dn, np.nextafter(dn, F32(0)), np.nextafter(dn, F32(2))], F32)
        _, weight, case, _ = FH.check(0.25, FH.make_keys(z, np.arange(6)), np.full(6, unit, np.uint16), scale=scale)
        assert case.tolist() == [FH.AGREE, FH.BEHIND, FH.AGREE, FH.AGREE, FH.FRONT, FH.AGREE] and weight.tolist() == [2, 1, 2, 2, 1, 2]
    # the mean is taken in inverse depth: 1 m with weight 3 and 2 m measured -> (3 + 0.5) / 4 = 0.875 -> scale / 0.875
    two_m = int(2 * scale)
    depth, weight, counts = V.fuse_depth_pixels(scale, 2.0, FH.make_keys(np.array([1.0], F32), [0]), np.array([two_m], np.uint16), np.array([3], np.uint8))
    assert depth.tolist() == [int(np.floor(scale / 0.875 + 0.5))] and weight.tolist() == [4] and counts.tolist() == [1, 0, 0, 0, 0, 0]
    # a filled pixel carries to_depth(scale, 1 / Z') over the whole range and beyond the saturation
    sat = 65535.0 / scale
    z = np.array([0.4 / scale, 0.6 / scale, 1.0 / scale, 0.0123, 1.0, 0.999 * sat, sat, 1.001 * sat, 1.1 * sat, 2.5 * sat, 1e6], F32)
    depth, weight, case, _ = FH.check(0.01, FH.make_keys(z, np.arange(len(z))), np.zeros(len(z), np.uint16), None, 255, 1, scale=scale)
    assert (case == FH.FILLED).all() and (depth == to_depth64(scale, F32(1.0) / z)).all()
    assert depth[0] == 0 and weight[0] == 0 and depth[1] == 1 and (depth[-4:] == 65535).all() and (weight[-4:] == 1).all()
    # depths 1 and 65535 measured: agreeing, conflicting and alone
    z = np.array([1 / scale, 65535 / scale, 5.0 * sat, 0.3 / scale, 1 / scale, 65535 / scale], F32)
    d = np.array([1, 65535, 1, 65535, 1, 65535], np.uint16)
    depth, weight, case, _ = FH.check(1e-3 * 5000.0 / scale, FH.make_keys(z, [0, 1, 2, 3, -1, -1]), d, scale=scale)
    assert case.tolist() == [FH.AGREE, FH.AGREE, FH.BEHIND, FH.FRONT, FH.MEASURED, FH.MEASURED]
    assert depth.tolist() == [1, 65535, 1, 65535, 1, 65535] and weight.tolist() == [2, 2, 1, 1, 1, 1]


# ------------------------------------------------------------------------------------------------------------ 2: rendering
def render_list(with_pose):
    """test_render_points_host.py's hostile list + points far enough to saturate at every scale used here (300 m * 256 > 65535), in the
    lower third of the image, which the list leaves empty: they win their pixels."""
    xyz, gray = RH.hostile_list(with_pose)
    rng = np.random.default_rng(29)
    m = 80
    xy = np.stack([rng.uniform(0, RH.COLS, m), rng.uniform(0.72 * RH.ROWS, RH.ROWS, m)], 1).astype(F32)
    far = V.camera_back_project(RH.cam(RH.ROWS, RH.COLS), RH.POSE if with_pose else None, xy, np.where(np.arange(m) % 2 == 0, 70.0, 300.0).astype(F32))
    return np.ascontiguousarray(np.concatenate([xyz, far]), F32), np.concatenate([gray, rng.integers(1, 256, m).astype(np.uint8)])


@OPERATOR_SCALE
@pytest.mark.parametrize("footprint", [1, 2, 3])
@pytest.mark.parametrize("with_pose", [False, True], ids=["no_pose", "pose"])
def test_render_points_host_equals_restatement(scale, footprint, with_pose):
    xyz, gray = render_list(with_pose)
    k, pose = RH.cam(RH.ROWS, RH.COLS), (RH.POSE if with_pose else None)
    for _, count, rng2 in RH.CASES[:2] + RH.CASES[5:6]:   # whole, a range, a short count with a range
        got = V.render_points_host(xyz, gray, k, RH.ROWS, RH.COLS, scale, pose7=pose, footprint=footprint, count=count, range2=rng2)
        want = RH.restatement(xyz, gray, len(xyz) if count is None else count, rng2, k, RH.ROWS, RH.COLS, scale, pose, footprint)
        RH.assert_same(got, want, f"scale {scale} footprint {footprint}")
    whole = V.render_points_host(xyz, gray, k, RH.ROWS, RH.COLS, scale, pose7=pose, footprint=footprint)
    covered = whole["zkey"] != RH.EMPTY
    zp = (whole["zkey"][covered] >> np.uint64(32)).astype(np.uint32).view(F32)
    assert (whole["depth"][covered] == to_depth64(scale, F32(1.0) / zp)).all()         # ... and the float64 statement of the rule
    assert (whole["depth"][covered] == 65535).any(), "no pixel whose depth saturates"
    assert (whole["depth"][covered] == 0).any(), "no covered pixel whose depth rounds to 0"
    assert ((whole["depth"][covered] > 0) & (whole["depth"][covered] < 65535)).any()


# ------------------------------------------------------------------------------------------------------------ 2: normals
DIST = 1.2   # metres: both tilts stay below 65535 / 30000 = 2.18 m (z in 0.9 .. 1.76)


@OPERATOR_SCALE
@pytest.mark.parametrize("tilt", sorted(NH.TILTS))
@pytest.mark.parametrize("step", [1, 2, 4])
def test_depth_normals_host_tilted_planes_against_float64(scale, tilt, step):
    """test_normals_host.py's comparison with the float64 stencil on the same quantised depths, under its bound: the bound is the float32
    rounding of the back-projected points against the length of the tangents, neither of which depends on the depth scale. The angle to
    the plane's true normal is bounded by the quantisation instead: the two depths of a tangent are each within half a unit, so their
    difference is off by at most 1 / scale metres along a ray (rx, ry, 1) at most 1.25 long, over a base of 2 step pixels of
    z_min / f_max metres each; two tangents: 1.25 sqrt(2) < 2."""
    normal = NH.TILTS[tilt][0]
    d = NH.tilted_depth(normal, DIST, scale=scale)
    assert d.max() < 65535 and d.min() > 0
    out = NH.normals(d, step, scale=scale)
    ref, has = NH.reference64(d, NH.CAM, step, 1.0, scale=scale)
    assert has.all() and out["counts"].tolist() == [d.size] * 3
    n = out["normals"]
    worst = NH.angles_deg(n, ref).max()
    print(f"scale {scale} tilt {tilt} step {step}: largest angle {worst:.3g} deg")
    assert worst <= NH.ANGLE_BOUND_DEG
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=-1) - 1.0).max() <= 1e-6
    want = -np.array(normal) / np.linalg.norm(normal)
    z_min = d.min() / scale
    base = 2 * step * z_min / float(max(abs(NH.CAM[2]), abs(NH.CAM[3])))
    inner = n[step:-step, step:-step]   # (the borders use one-sided differences: half the base)
    assert np.median(NH.angles_deg(inner, np.broadcast_to(want, inner.shape))) <= np.degrees(np.arctan(2.0 / scale / base))
    NH.enough_normals(out)


@OPERATOR_SCALE
def test_depth_normals_host_holes_jumps_and_the_list_form(scale):
    rng = np.random.default_rng(5)
    d = NH.tilted_depth(NH.TILTS["A"][0], DIST, rows=33, cols=47, scale=scale)
    d[rng.random(d.shape) < 0.03] = 0
    d[:, 30:] = np.minimum(d[:, 30:].astype(np.int64) + int(0.3 * scale), 65535).astype(np.uint16)   # a 0.3 m step: beyond jump_m
    d[4:9, 5:12] = 65535
    plane = NH.normals(d, 2, 0.05, scale=scale)
    ref, has = NH.reference64(d, NH.CAM, 2, 0.05, scale=scale)
    got_has = plane["normals"].any(-1)
    assert (got_has == has).all() and plane["counts"].tolist() == [d.size, int((d > 0).sum()), int(has.sum())]
    assert 0 < int(has.sum()) < int((d > 0).sum()), "the step and the holes must cost some pixels their normal"
    assert (NH.angles_deg(plane["normals"][has], ref[has]) <= NH.ANGLE_BOUND_DEG).all()
    # a constant plane is exactly -z at every scale
    flat = NH.normals(np.full((9, 13), 700, np.uint16), scale=scale)["normals"]
    want = np.zeros((9, 13, 3), F32)
    want[..., 2] = -1.0
    assert np.array_equal(flat.view(np.uint32), want.view(np.uint32))
    # the comparison with jump_m is <=: 0.5 m is 2000 - 1500 units at 1000, 384 - 256 at 256 and 45000 - 30000 at 30000, all exact
    a, b = int(scale), int(1.5 * scale)
    edge = np.full((3, 3), a, np.uint16)
    edge[:, 2] = b
    assert int(NH.normals(edge, 1, 0.5, scale=scale)["counts"][2]) == 9
    assert int(NH.normals(edge, 1, float(np.nextafter(F32(0.5), F32(0))), scale=scale)["counts"][2]) == 6
    # the list form is the plane form gathered
    xs, ys = rng.integers(0, 47, 300), rng.integers(0, 33, 300)
    xs[7], ys[7] = 47, 3
    lst = NH.normals(d, 2, 0.05, scale=scale, pixel=(xs | (ys << 16)).astype(np.uint32))
    gathered = np.zeros((300, 3), F32)
    inside = xs < 47
    gathered[inside] = plane["normals"][ys[inside], xs[inside]]
    assert np.array_equal(lst["normals"].view(np.uint32), gathered.view(np.uint32))
