"""The conditioning measure of an ICP system and the joint stage's verdict on the host (vors_icp_condition_from_sums,
vors_map_icp_verdict_joint_host; needs no GPU). Scenes and constants are tests/test_icp_joint_host.py's: the 48x64 "corner"
(three planes) and "plane" (ONE tilted plane, the degenerate geometry of DESIGN.md 7n) under its texture, evaluated at P_TRUE with
iters = 0, the distance gate alone (no frame normals, no Huber weight).

Measured with the host twin (recorded in DESIGN.md 7p):

  | scene  | pass                                 | matched | flags | dilution_t | dilution_r, 1/m | cond(H)  |
  | corner | robust (photo_scale_m = 0)           | 2976    | 0     | 8.4509     | 8.2123          | 44.9     |
  | corner | joint, PHOTO_SCALE_M                 | 2976    | 0     | 6.8792     | 6.0297          | 30.5     |
  | plane  | robust                               | 2558    | 0     | 4.538e8    | 2941.5          | 2.9e18   |
  | plane  | joint, PHOTO_SCALE_M                 | 2558    | 0     | 9.8745     | 7.1880          | 170      |
  | plane  | joint, PHOTO_SCALE_M / 100 ("weak")  | 2558    | 0     | 783.34     | 644.56          | 1.29e6   |

  The single plane under the robust pass: the twin's Cholesky SUCCEEDS on rounding alone (the smallest eigenvalue of H in float64 is
  -3e-13 beside a largest of about 860) and gives dilution_t = 4.5e8, 5e7 times the corner's: of the two outcomes the issue allows
  (flag bit 1, or at least 100 x the corner's) the twin gives the second. Either fails any sensible bound.

BOUNDS = (80, 70): the geometric means of the corner's and the weak texture's values, sqrt(8.45 x 783) = 81.3 and sqrt(8.21 x 645) = 72.8,
rounded down to one digit. They separate "constrained" from "slides" with a factor of about ten to either side and are what
tests/test_gpu_trackers_map_icp_joint.py uses; they are not tuned on any trajectory.

ULP: the rule is compared with numpy.linalg.inv of the same H in float64, rounded to f32 — equal, or one f32 ulp apart. The test asserts
cond(H) < 1e6 for the systems compared, so the f64 error of either inverse is about cond x 2^-53 < 1.2e-10 relative, far below half an
f32 ulp (6e-8): the two can differ only where that error straddles a rounding boundary, by one ulp.
"""
import numpy as np
import pytest

import vors_amd as V
from test_icp_joint_host import PHOTO_SCALE_M, corner, joint_host, plane  # noqa: F401  (corner, plane: the module's fixtures)
from test_icp_robust_host import P_TRUE, bits

BOUNDS = dict(max_dilution_t=80.0, max_dilution_r=70.0)
VERDICT = dict(dist_m=0.05, min_match_ratio=0.5, max_rms=0.01, max_trans_m=0.02, max_rot_rad=0.1)


def sums_of(scene, photo_scale_m):
    return joint_host(scene, P_TRUE, iters=0, photo_scale_m=photo_scale_m)["sums29"]


def h_of(sums29):
    h = np.zeros((6, 6))
    k = 8
    for r in range(6):
        for c in range(r, 6):
            h[r, c] = h[c, r] = float(sums29[k])
            k += 1
    return h


def numpy_dilutions(sums29):
    c, n = np.linalg.inv(h_of(sums29)), float(sums29[1])
    return np.float32(np.sqrt(n * ((c[0, 0] + c[1, 1]) + c[2, 2]))), np.float32(np.sqrt(n * ((c[3, 3] + c[4, 4]) + c[5, 5])))


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.fixture(scope="module")
def systems(corner, plane):
    return {"corner robust": sums_of(corner, 0.0), "corner joint": sums_of(corner, PHOTO_SCALE_M), "plane robust": sums_of(plane, 0.0),
            "plane joint": sums_of(plane, PHOTO_SCALE_M), "plane weak": sums_of(plane, PHOTO_SCALE_M / 100)}


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", ["corner joint", "corner robust", "plane joint"])
def test_rule_against_numpy(systems, name):
    s = systems[name]
    assert np.linalg.cond(h_of(s)) < 1e6
    dt, dr, flags = V.icp_condition_from_sums(s)
    want = numpy_dilutions(s)
    print(f"\n{name}: matched {s[1]:.0f} dilution_t {dt!r} dilution_r {dr!r} numpy {want} cond {np.linalg.cond(h_of(s)):.4g}")
    assert flags == 0 and np.isfinite(dt) and np.isfinite(dr)
    assert ulps(dt, want[0]) <= 1 and ulps(dr, want[1]) <= 1


# ------------------------------------------------------------------------------------------------------------ 2
def test_separation(systems):
    got = {name: V.icp_condition_from_sums(s) for name, s in systems.items()}
    for name, (dt, dr, flags) in got.items():
        print(f"\n{name}: dilution_t {dt:.6g} dilution_r {dr:.6g} flags {flags}")
    corner_t = got["corner robust"][0]
    dt, dr, flags = got["plane robust"]
    assert (flags & 2) or dt >= 100.0 * corner_t, "one plane under point-to-plane rows alone must not look like the corner"
    if flags:
        assert np.isnan(dt) and np.isnan(dr)
    dt, dr, flags = got["plane joint"]
    assert flags == 0 and np.isfinite(dt) and np.isfinite(dr)
    weak = got["plane weak"]
    assert weak[2] == 0 and weak[0] > dt and weak[1] > dr, "a hundredth of the photometric weight must hold the plane less well"
    # the bounds lie between the constrained systems and the weak one, as their derivation says
    for name in ("corner robust", "corner joint", "plane joint"):
        assert got[name][0] <= BOUNDS["max_dilution_t"] and got[name][1] <= BOUNDS["max_dilution_r"]
    assert weak[0] > BOUNDS["max_dilution_t"] and weak[1] > BOUNDS["max_dilution_r"]


# ------------------------------------------------------------------------------------------------------------ 3
def stats(status=V.ICP_CONVERGED, matched=500, considered=1000, rms=0.01):
    s = np.zeros(1, V.ICP_STATS_DTYPE)[0]
    s["status"], s["iterations"], s["considered"], s["matched"], s["rms"] = status, 3, considered, matched, rms
    return s


BEFORE = np.array([0.1, -0.2, 0.3, 0, 0, 0, 1], np.float32)
FAR = BEFORE + np.array([0.05, 0, 0, 0, 0, 0, 0], np.float32)
BROKEN = np.array([0.1, -0.2, 0.3, np.nan, 0, 0, 1], np.float32)
# one row per existing failure, and one ACCEPTED row
ROWS = [("accepted", stats(), BEFORE, V.MAP_ICP_ACCEPTED), ("nonfinite", stats(), BROKEN, V.MAP_ICP_NONFINITE),
        ("icp status", stats(status=V.ICP_SINGULAR, matched=0, rms=np.nan), BEFORE, V.MAP_ICP_ICP_STATUS), ("few matches", stats(matched=499), BEFORE, V.MAP_ICP_FEW_MATCHES),
        ("rms", stats(rms=0.02), BEFORE, V.MAP_ICP_RMS), ("step", stats(), FAR, V.MAP_ICP_STEP)]


@pytest.mark.parametrize("name,st,after,want", ROWS, ids=[r[0] for r in ROWS])
def test_verdict_with_both_bounds_off_is_the_plain_verdict(name, st, after, want):
    assert V.map_icp_verdict_host(VERDICT, st, BEFORE, after) == want
    for dt, dr in ((1.0, 1.0), (1e30, 1e30), (np.nan, np.nan), (np.inf, 0.0)):
        assert V.map_icp_verdict_joint_host(VERDICT, st, BEFORE, after, dt, dr) == want, (dt, dr)


@pytest.mark.parametrize("name,st,after,want", ROWS, ids=[r[0] for r in ROWS])
def test_an_existing_failure_keeps_its_name(name, st, after, want):
    p = dict(VERDICT, max_dilution_t=1.0, max_dilution_r=1.0)
    for dt, dr in ((50.0, 50.0), (np.nan, np.nan)):
        assert V.map_icp_verdict_joint_host(p, st, BEFORE, after, dt, dr) == (V.MAP_ICP_CONDITION if want == V.MAP_ICP_ACCEPTED else want)
    assert V.map_icp_verdict_joint_host(p, st, BEFORE, after, 1.0, 1.0) == want   # equality on a bound holds


def test_verdict_on_the_scenes(systems):
    p = dict(VERDICT, **BOUNDS)
    verdict = lambda name: V.map_icp_verdict_joint_host(p, stats(), BEFORE, BEFORE, *V.icp_condition_from_sums(systems[name])[:2])
    assert verdict("corner robust") == V.MAP_ICP_ACCEPTED and verdict("corner joint") == V.MAP_ICP_ACCEPTED
    assert verdict("plane robust") == V.MAP_ICP_CONDITION
    assert verdict("plane joint") == V.MAP_ICP_ACCEPTED and verdict("plane weak") == V.MAP_ICP_CONDITION
    nan = float("nan")
    assert V.map_icp_verdict_joint_host(p, stats(), BEFORE, BEFORE, nan, 1.0) == V.MAP_ICP_CONDITION
    assert V.map_icp_verdict_joint_host(p, stats(), BEFORE, BEFORE, 1.0, nan) == V.MAP_ICP_CONDITION
    assert V.map_icp_verdict_joint_host(dict(p, max_dilution_r=0.0), stats(), BEFORE, BEFORE, 1.0, nan) == V.MAP_ICP_ACCEPTED
    assert V.map_icp_verdict_joint_host(dict(p, max_dilution_t=0.0), stats(), BEFORE, BEFORE, nan, 1.0) == V.MAP_ICP_ACCEPTED
    assert V.MAP_ICP_CONDITION == 7


# ------------------------------------------------------------------------------------------------------------ 4
def test_flags(systems):
    s = systems["corner joint"].copy()
    good = V.icp_condition_from_sums(s)
    for count, want in ((6.0, 1), (7.0, 0), (0.0, 1), (float("nan"), 1)):
        s[1] = count
        dt, dr, flags = V.icp_condition_from_sums(s)
        assert flags == want
        assert (np.isnan(dt) and np.isnan(dr)) if want else (np.isfinite(dt) and np.isfinite(dr))
    # the dilution is normalised by the count: the same H with a quarter of the count is half the dilution, up to the two roundings
    s[1] = good_count = systems["corner joint"][1]
    s[1] = np.float32(good_count / 4)
    dt, _, _ = V.icp_condition_from_sums(s)
    assert abs(float(dt) * 2 / float(good[0]) - 1) < 1e-6
    zero = np.zeros(29, np.float32)
    dt, dr, flags = V.icp_condition_from_sums(zero)
    assert flags == 3 and np.isnan(dt) and np.isnan(dr)
    zero[1] = 100.0
    dt, dr, flags = V.icp_condition_from_sums(zero)
    assert flags == 2 and np.isnan(dt) and np.isnan(dr)
    # slots 0 and 2..7 (energy and gradient) are not read
    s = systems["corner joint"].copy()
    s[[0, 2, 3, 4, 5, 6, 7]] = np.nan
    again = V.icp_condition_from_sums(s)
    assert bits(np.float32(again[0])) == bits(np.float32(good[0])) and bits(np.float32(again[1])) == bits(np.float32(good[1])) and again[2] == 0


# ------------------------------------------------------------------------------------------------------------ 5
def test_refusals():
    lib, p = V.lib(), np.zeros(64, np.float32).ctypes.data_as(V.C.c_void_p)
    for name in ("vors_icp_condition_from_sums", "vors_icp_condition", "vors_map_icp_verdict_joint_host", "vors_trackers_enable_map_icp_joint",
                 "vors_trackers_map_icp_joint", "vors_tracker_enable_map_icp_joint", "vors_tracker_read_map_icp_joint"):
        assert hasattr(lib, name) and name in V.EXPORTED_SYMBOLS
    assert lib.vors_icp_condition_from_sums(None, p, p, p) == -1 and lib.vors_last_error() == b"icp_condition_from_sums: sums29 is NULL"
    assert lib.vors_icp_condition_from_sums(p, None, None, None) == 0
    for args, sentence in (((0, p, p, p, None), b"icp_condition: n must be >= 1"), ((1, None, p, p, None), b"icp_condition: d_sums29 is NULL"),
                           ((1, p, None, p, None), b"icp_condition: d_dilution2 is NULL"),
                           ((1, V.C.c_void_p(p.value + 2), p, p, None), b"icp_condition: d_sums29, d_dilution2 and d_flags must be 4-byte aligned"),
                           ((1, p, p, V.C.c_void_p(p.value + 1), None), b"icp_condition: d_sums29, d_dilution2 and d_flags must be 4-byte aligned")):
        assert lib.vors_icp_condition(*args) == -1 and lib.vors_last_error() == sentence, sentence
    nan = float("nan")
    for kw, sentence in ((dict(max_dilution_t=-1.0), "map_icp_verdict_joint_host: max_dilution_t must be >= 0 (and not NaN; 0 = that bound is off)"),
                         (dict(max_dilution_t=nan), "map_icp_verdict_joint_host: max_dilution_t must be >= 0 (and not NaN; 0 = that bound is off)"),
                         (dict(max_dilution_r=-0.5), "map_icp_verdict_joint_host: max_dilution_r must be >= 0 (and not NaN; 0 = that bound is off)"),
                         (dict(max_dilution_r=nan), "map_icp_verdict_joint_host: max_dilution_r must be >= 0 (and not NaN; 0 = that bound is off)"),
                         (dict(max_rms=-1.0), "map_icp_verdict_joint_host: max_rms must be >= 0 (and not NaN)"),
                         (dict(min_match_ratio=1.5), "map_icp_verdict_joint_host: min_match_ratio must lie in [0, 1] (and not be NaN)")):
        with pytest.raises(V.VorsError) as e:
            V.map_icp_verdict_joint_host(dict(VERDICT, **kw), stats(), BEFORE, BEFORE, 1.0, 1.0)
        assert str(e.value).endswith(sentence), str(e.value)
    q = V.map_icp_joint_params(**VERDICT)
    st = np.zeros(1, V.ICP_STATS_DTYPE)
    v = V.C.c_uint32(0)
    ptr = lambda a: a.ctypes.data_as(V.C.c_void_p)
    for args in ((None, ptr(st), ptr(BEFORE), ptr(BEFORE)), (V.C.byref(q), None, ptr(BEFORE), ptr(BEFORE)), (V.C.byref(q), ptr(st), None, ptr(BEFORE)),
                 (V.C.byref(q), ptr(st), ptr(BEFORE), None)):
        assert lib.vors_map_icp_verdict_joint_host(*args, 1.0, 1.0, V.C.byref(v)) == -1
        assert lib.vors_last_error() == b"map_icp_verdict_joint_host: a NULL argument (params, stats, pose_before, pose_after, verdict)"
    assert lib.vors_map_icp_verdict_joint_host(V.C.byref(q), ptr(st), ptr(BEFORE), ptr(BEFORE), 1.0, 1.0, None) == -1
    # the handle entries refuse a NULL handle before anything else
    assert lib.vors_trackers_enable_map_icp_joint(None, V.C.byref(q)) == -1 and lib.vors_last_error() == b"enable_map_icp_joint: the handle t is NULL"
    assert lib.vors_trackers_map_icp_joint(None, None) == -1 and lib.vors_last_error() == b"map_icp_joint: the handle t is NULL"
    assert lib.vors_tracker_enable_map_icp_joint(None, V.C.byref(q)) == -1 and lib.vors_last_error() == b"enable_map_icp_joint: the handle t is NULL"
    assert lib.vors_tracker_read_map_icp_joint(None, None) == -1 and lib.vors_last_error() == b"read_map_icp_joint: the handle t is NULL"
    # the Python record: names and types only
    with pytest.raises(V.VorsError, match="map_icp: unknown parameter 'max_dilution'"):
        V.map_icp_joint_params(dist_m=0.05, max_dilution=3.0)
    with pytest.raises(V.VorsError, match="map_icp_joint: photo_scale_m must be a number"):
        V.map_icp_joint_params(dist_m=0.05, photo_scale_m="a lot")
    with pytest.raises(V.VorsError, match="map_icp: dist_m is required"):
        V.map_icp_joint_params(photo_scale_m=0.001)
    r = V.map_icp_joint_params(dist_m=0.05, iters=3, photo_scale_m=0.0005, photo_huber_grey=10, max_dilution_t=80)
    assert (r.icp.iters, r.icp.min_points) == (3, 6) and bits(np.float32(r.photo_scale_m)) == bits(np.float32(0.0005)) and r.max_dilution_r == 0.0


# ------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("name", ["corner joint", "corner robust", "plane joint", "plane weak"])
def test_the_two_texts_of_the_factorisation_agree(systems, name):
    """lie.h icp_condition repeats pose_information's mirror, Cholesky and L^-1 so that the latter's kernel keeps its listing; this keeps
    the two in step. cov = sigma2 * C there, so dilution^2 = n * tr(cov block) / sigma2. From the f32 outputs of
    vors_pose_information_from_sums: three positive cov entries, each within 2^-24 relative, hence their sum too; sigma2 within 2^-24;
    the square root halves both, 2^-24 together; the dilution's own rounding 2^-24 — 2^-23 to first order, the rest is of order 2^-48."""
    s = systems[name]
    info, cov, sigma2, flags = V.pose_information_from_sums(s)
    dt, dr, fl = V.icp_condition_from_sums(s)
    assert flags == 0 and fl == 0 and sigma2 > 0
    cov, n = np.asarray(cov, np.float64).reshape(6, 6), float(s[1])
    want_t = np.sqrt(n * ((cov[0, 0] + cov[1, 1]) + cov[2, 2]) / float(sigma2))
    want_r = np.sqrt(n * ((cov[3, 3] + cov[4, 4]) + cov[5, 5]) / float(sigma2))
    bound = 2.0 ** -23 * (1 + 1e-6)
    print(f"\n{name}: relative differences {abs(float(dt) / want_t - 1):.3g}, {abs(float(dr) / want_r - 1):.3g} (bound {bound:.3g})")
    assert abs(float(dt) / want_t - 1) <= bound and abs(float(dr) / want_r - 1) <= bound
    # and both refuse the same systems: too few points, no factor
    for bad in (np.zeros(29, np.float32), np.r_[s[:1], np.float32(6.0), s[2:]].astype(np.float32)):
        assert V.pose_information_from_sums(bad)[3] == V.icp_condition_from_sums(bad)[2] != 0
