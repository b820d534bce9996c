"""Config.depth_scale and Config.idepth_variance away from TUM's 5000 and 1e-4 (tests/depth_scales.py gives the values and why). GPU only.

The scenes are the synthetic ones, which quantise depth at 5000; their depth maps are re-quantised on the host (depth_scales.requantise),
so that the geometry stays consistent with the configured scale.

  1. the points of every keyframe form == oracle.Tracker's, bit for bit (coordinates, inverse depths, Jacobians, every level): the four
     dense inverse-depth forms and the halving kernel behind them, each as <true> / <false> (VORS_NO_FASTDIV unset: whatever the
     enumeration over the 65535 depths picks at that scale; set: <false>), coarse-to-fine and DSO; a third of the depths unknown and one
     quadrant entirely unknown, so that every child count occurs;
  2. track_pairs end to end, three modes x three arithmetics over the grid of scales and variances at 96x128 / 4 levels (dense level 0 =
     12288 points > 2500: FUSED's quad source runs): REFERENCE == the oracle's bits; EXACT and FUSED: statuses and point counts equal,
     every pair within POSE_TOL. Checked on the CPU beforehand with the oracle alone (seed 0x5EEDC0DE, 4 pairs, 6 scales x 3 variances x
     3 modes, Huber off and 8): every status is 0 and the oracle against its own float64-sum build differs by at most 2.7e-6, so no
     pair is left out;
  3. FUSED and EXACT sums of vors_batch_eval_pairs on dense level 0 at the tracked model against float64 sums over the ORACLE's points,
     under the bounds of test_gpu_eval_pairs.py;
  4. two handles of different scale and variance alive at once, tracked alternately: each equals its own oracle (a table or a flag
     that outlives or leaks between handles would show);
  5. (tests/test_gpu_depth_scale_products.py)
  6. the stand-alone operators == their host twins bit for bit: render_points (footprints 1 and 3), depth_normals, points_normals, on an
     aligned and an odd plane;
  7. sequence trackers at scale 1000 / variance 1: REFERENCE poses == oracle.track_sequences' bits; then with the depth filter, the map,
     its normals and render_map: the compositions of test_gpu_trackers_depth_filter.py, test_gpu_trackers_map.py,
     test_gpu_trackers_map_normals.py and test_gpu_render_map.py with the scale passed through, and the host helpers at that scale."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from oracle import oracle as O
from depth_scales import BLOCKY, GRID, SCALES, requantise, scale_id

POSE_TOL = 1e-4   # rad / metres (BASELINE.json north_star; tests/test_gpu_fuzz.py)
F32 = np.float32
ARITHS = {"reference": V.ARITH_REFERENCE, "exact": V.ARITH_EXACT, "fused": V.ARITH_FUSED}
MODE_NAMES = ("c2f", "dense", "dso")
# one variance per scale for the keyframe forms; all three occur in every mode
FORM_VARIANCE = {5000.0: 3e-7, 1000.0: 1.0, 256.0: 3e-7, 6553.5: 1.0, 3.0: 1e-4, 30000.0: 1.0}
assert set(FORM_VARIANCE) == set(SCALES) and len(set(FORM_VARIANCE.values())) == 3


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def vcfg(L, intr, mode, scale, variance, arith=V.ARITH_REFERENCE, huber=0.0):
    return V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, depth_scale=scale,
                    idepth_variance=variance, huber_delta=huber, arithmetic=arith)


def ocfg(L, intr, mode, scale, variance, huber=0.0):
    return O.make_config(L, intr, depth_scale=scale, idepth_variance=variance, candidates_mode=mode, huber_delta=huber)


def dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dtype) if dtype is not None else a).cuda()


def track(b, kg, kd, cg):
    """Batch.track_pairs on host arrays -> (poses, status, decoded stats, the stats tensor)."""
    import torch
    n = len(kg)
    poses = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    stats = V.stats_tensor(n)
    b.track_pairs(dev(kg), dev(kd, np.int16), dev(cg), poses, status, stats)
    torch.cuda.synchronize()
    return poses.cpu().numpy(), status.cpu().numpy(), V.decode_stats(stats), stats


# ------------------------------------------------------------------------------------------------------------ 1
FORMS = [("level123", 64, 96, 4, 1), ("level12", 36, 64, 4, 1), ("level1_wide", 50, 72, 3, 1), ("per_pixel", 51, 77, 3, 1),
         ("level123_then_halve", 80, 96, 5, 1), ("coarse_to_fine", 96, 128, 4, 0), ("dso", 96, 128, 4, 2)]


@functools.lru_cache(maxsize=None)
def form_scene(rows, cols, mode):
    """2 keyframes + current frames at 5000; a third of the depths unknown and the first quadrant of pair 1 entirely unknown; a corner at
    2.4 m, which re-quantises to the 65535 clamp at 30000 (the scenes themselves end just below it, at about 2.18 m)."""
    intr = O.scaled_intrinsics(rows, cols)
    kg, kd, cg, _, _ = O.synth_batch(2, rows, cols, seed0=(0x5EEDAB00 + rows) | (BLOCKY if mode == 2 else 0), intr=intr)
    rng = np.random.default_rng(rows + cols)
    kd[rng.random(kd.shape) < 0.33] = 0
    kd[1, : rows // 2, : cols // 2] = 0
    kd[:, rows - 5:, cols - 9:] = 12000
    return intr, kg, kd, cg


@functools.lru_cache(maxsize=None)
def form_oracle(rows, cols, L, mode, scale):
    """The oracle's points of every level of both pairs (shared by the two VORS_NO_FASTDIV settings)."""
    intr, kg, kd, _ = form_scene(rows, cols, mode)
    kds = requantise(kd, scale)
    out = []
    for p in range(2):
        tr = O.Tracker(ocfg(L, intr, mode, scale, FORM_VARIANCE[scale]), 0.0, kds[p], 0.0, kg[p])
        out.append([tr.points(l) for l in range(L)])
    return out


@pytest.mark.parametrize("no_fastdiv", [False, True], ids=["verified", "ieee_division"])
@pytest.mark.parametrize("scale", SCALES, ids=scale_id)
@pytest.mark.parametrize("form,rows,cols,L,mode", FORMS, ids=[f[0] for f in FORMS])
def test_points_of_every_keyframe_form_bit_for_bit(form, rows, cols, L, mode, scale, no_fastdiv, monkeypatch):
    # (the flag is read when the handle is created)
    if no_fastdiv:
        monkeypatch.setenv("VORS_NO_FASTDIV", "1")
    else:
        monkeypatch.delenv("VORS_NO_FASTDIV", raising=False)
    monkeypatch.delenv("VORS_IDEPTH_LEVEL12", raising=False)
    intr, kg, kd, cg = form_scene(rows, cols, mode)
    kds = requantise(kd, scale)
    assert (kds == 65535).any() == (scale == 30000.0)
    b = V.Batch(vcfg(L, intr, mode, scale, FORM_VARIANCE[scale]), 2, rows, cols)
    track(b, kg, kds, cg)
    want = form_oracle(rows, cols, L, mode, scale)
    total = 0
    for p in range(2):
        for l in range(L):
            xy, iz, jac, tm = b.points(p, l)
            oxy, oiz, ojac = want[p][l]
            where = f"{form} scale {scale} pair {p} level {l}"
            assert xy.shape == oxy.shape, f"{where}: {len(xy)} vs {len(oxy)} points"
            o1, o2 = np.lexsort((xy[:, 1], xy[:, 0])), np.lexsort((oxy[:, 1], oxy[:, 0]))
            assert (xy[o1] == oxy[o2]).all(), where
            bad = bits(iz[o1]) != bits(oiz[o2])
            assert not bad.any(), f"{where}: {int(bad.sum())} inverse depths differ, first {iz[o1][bad][:3]} vs {oiz[o2][bad][:3]}"
            assert (bits(jac[o1]) == bits(ojac[o2])).all(), where
            total += len(xy)
    assert total > 0
    if mode == 1:   # dense: every level is there, and the coarsest still has points
        assert len(want[0][L - 1][0]) > 0 and len(want[1][L - 1][0]) > 0


# ------------------------------------------------------------------------------------------------------------ 2
ROWS, COLS, LEVELS, N = 96, 128, 4, 4
SEED = 0x5EEDC0DE
INTR = O.scaled_intrinsics(ROWS, COLS)
HUBER_CASES = [(1000.0, 1.0, 8.0)]
TRACK_CASES = [(s, v, 0.0) for s, v in GRID] + HUBER_CASES


@functools.lru_cache(maxsize=None)
def pairs(mode):
    kg, kd, cg, cd, _ = O.synth_batch(N, ROWS, COLS, seed0=SEED | (BLOCKY if mode == 2 else 0), intr=INTR)
    return kg, kd, cg, cd


@functools.lru_cache(maxsize=None)
def oracle_track(mode, scale, variance, huber):
    kg, kd, cg, _ = pairs(mode)
    return O.track_pairs(ocfg(LEVELS, INTR, mode, scale, variance, huber), kg, requantise(kd, scale), cg, n_threads=4)


def assert_track_equals_oracle(got, ref, arith, what):
    p, status, st, _ = got
    assert (status == ref["status"]).all(), what
    assert (ref["status"] == 0).all(), f"{what}: the oracle alone was checked to track every pair"
    assert (st["n_points"][:, :LEVELS] == ref["n_points"]).all(), (what, st["n_points"][:, :LEVELS], ref["n_points"])
    err = np.abs(p - ref["poses"]).max(axis=1)
    print(f"{what}: max |pose - oracle| per pair {err}")
    assert (err < POSE_TOL).all(), f"{what}: pose error {err}"
    if arith == V.ARITH_REFERENCE:   # the reference's own summation order: the same LM path and the same bits
        assert (st["nb_iter"][:, :LEVELS] == ref["nb_iter"]).all(), f"{what}: iteration counts {st['nb_iter'][:, :LEVELS]} vs {ref['nb_iter']}"
        for name, a, w in (("poses", p, ref["poses"]), ("lm_model", st["lm_model"], ref["models"]), ("optical_flow", st["optical_flow"], ref["flow"])):
            assert (bits(a) == bits(w)).all(), f"{what}: {name} differ from the oracle's bits"


@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("scale,variance,huber", TRACK_CASES, ids=[scale_id(s, v) + ("-huber" if h else "") for s, v, h in TRACK_CASES])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=MODE_NAMES)
def test_track_pairs_against_the_oracle(mode, scale, variance, huber, arith):
    kg, kd, cg, _ = pairs(mode)
    ref = oracle_track(mode, scale, variance, huber)
    b = V.Batch(vcfg(LEVELS, INTR, mode, scale, variance, ARITHS[arith], huber), N, ROWS, COLS)
    got = track(b, kg, requantise(kd, scale), cg)
    if mode == 1:
        assert (ref["n_points"][:, 0] > 2500).all()   # FUSED's quad source runs at level 0
    assert_track_equals_oracle(got, ref, ARITHS[arith], f"{MODE_NAMES[mode]} {arith} scale {scale} variance {variance} huber {huber}")


@pytest.mark.parametrize("mode", [0, 1, 2], ids=MODE_NAMES)
def test_the_variance_and_the_scale_are_visible_in_the_bits(mode):
    """What the comparisons above can see: on the oracle alone, another variance changes the iteration counts or the poses, and a depth
    map read at the wrong scale does so grossly."""
    kg, kd, cg, _ = pairs(mode)
    base = oracle_track(mode, 1000.0, 1.0, 0.0)
    other = oracle_track(mode, 1000.0, 1e-4, 0.0)
    assert not (bits(base["poses"]) == bits(other["poses"])).all(), "the variance alone does not change a bit of the poses"
    wrong = O.track_pairs(ocfg(LEVELS, INTR, mode, 5000.0, 1.0), kg, requantise(kd, 1000.0), cg, n_threads=4)
    assert np.abs(wrong["poses"] - base["poses"]).max() > 100 * POSE_TOL


# ------------------------------------------------------------------------------------------------------------ 3
class OraclePoints:
    """What test_gpu_eval_pairs.float64_sums reads of a handle, answered by the oracle: points(pair, level) and current_image(pair, level)."""

    def __init__(self, cfg, kg, kd, cg, L):
        self.trackers = [O.Tracker(cfg, 0.0, kd[p], 0.0, kg[p]) for p in range(len(kg))]
        self.current = [O.mean_pyramid(cg[p], L) for p in range(len(kg))]

    def points(self, pair, lvl):
        tr = self.trackers[pair]
        xy, iz, jac = tr.points(lvl)
        return xy, iz, jac, tr.image(lvl)[xy[:, 1], xy[:, 0]]

    def current_image(self, pair, lvl):
        return self.current[pair][lvl]


class EvalScene:
    """The attributes of test_gpu_eval_pairs.Scene that float64_sums reads."""

    def __init__(self, intr, huber):
        self.intr, self.huber, self.level_data = intr, huber, {}


@pytest.mark.parametrize("scale,variance", [(1000.0, 1.0), (3.0, 3e-7), (30000.0, 1.0)], ids=lambda v: f"{v:g}")
def test_eval_pairs_sums_against_float64_sums_over_the_oracles_points(scale, variance):
    import torch
    from test_gpu_eval_pairs import assert_within_float64_bounds, float64_sums
    kg, kd, cg, _ = pairs(1)
    kds = requantise(kd, scale)
    src = OraclePoints(ocfg(LEVELS, INTR, 1, scale, variance), kg, kds, cg, LEVELS)
    sc = EvalScene(INTR, 0.0)
    for name in ("fused", "exact"):
        b = V.Batch(vcfg(LEVELS, INTR, 1, scale, variance, ARITHS[name]), N, ROWS, COLS)
        _, status, st, stats = track(b, kg, kds, cg)
        assert (status == 0).all()
        out = b.eval_pairs(0, stats, arithmetic=ARITHS[name])
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert out.shape == (N, 1, 29)
        for p in range(N):
            ref, slack, scale_g = float64_sums(sc, src, p, 0, st["lm_model"][p])
            assert ref[1] > 2500
            assert_within_float64_bounds(out[p, 0], ref, slack, scale_g, f"{name} scale {scale} pair {p}")


# ------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("mode", [1, 0], ids=["dense", "c2f"])
def test_two_handles_of_different_scale_alive_at_once(mode):
    kg, kd, cg, _ = pairs(mode)
    settings = ((1000.0, 1.0), (5000.0, 1e-4))
    handles = [V.Batch(vcfg(LEVELS, INTR, mode, s, v, V.ARITH_REFERENCE), N, ROWS, COLS) for s, v in settings]   # both before any track
    for turn in range(2):
        for (s, v), b in zip(settings, handles):
            got = track(b, kg, requantise(kd, s), cg)
            assert_track_equals_oracle(got, oracle_track(mode, s, v, 0.0), V.ARITH_REFERENCE, f"{MODE_NAMES[mode]} turn {turn} scale {s}")
    # ... and the keyframe records each handle is left with are its own
    for (s, v), b in zip(settings, handles):
        tr = O.Tracker(ocfg(LEVELS, INTR, mode, s, v), 0.0, requantise(kd, s)[0], 0.0, kg[0])
        for l in range(LEVELS):
            xy, iz, _, _ = b.points(0, l)
            oxy, oiz, _ = tr.points(l)
            o1, o2 = np.lexsort((xy[:, 1], xy[:, 0])), np.lexsort((oxy[:, 1], oxy[:, 0]))
            assert xy.shape == oxy.shape and (xy[o1] == oxy[o2]).all() and (bits(iz[o1]) == bits(oiz[o2])).all(), (s, l)


# ------------------------------------------------------------------------------------------------------------ 6
OPERATOR_SCALES = (1000.0, 256.0, 30000.0)
PLANES = {"aligned": (48, 64), "odd": (47, 63)}
PLANE = pytest.mark.parametrize("plane", list(PLANES))
OPERATOR_SCALE = pytest.mark.parametrize("scale", OPERATOR_SCALES, ids=scale_id)


def cam_of(rows, cols):
    return np.array([0.5 * cols - 0.5, 0.5 * rows - 0.5, 0.9 * cols, -0.95 * cols, 0.3], F32)   # fv < 0 and a skew


@functools.lru_cache(maxsize=None)
def operator_poses(n):
    rng = np.random.default_rng(11)
    p = np.empty((n, 7), F32)
    p[:, :3] = rng.uniform(-0.2, 0.2, (n, 3))
    q = np.concatenate([rng.uniform(-0.08, 0.08, (n, 3)), np.ones((n, 1))], 1)
    p[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return p


@functools.lru_cache(maxsize=None)
def point_lists(plane):
    """n = 2 world-frame lists seen by the cameras at operator_poses: points over and around the plane at 0.5 .. 6 m, some behind the
    camera, some at 1e-5 m (a depth that rounds to 0) and some at 70 and 300 m (300 m * 256 > 65535: a depth that saturates at every scale
    used here), those in the lower part of the image, which the nearer points leave empty."""
    rows, cols = PLANES[plane]
    rng = np.random.default_rng(rows)
    k, poses = cam_of(rows, cols), operator_poses(2)
    lists = []
    for i in range(2):
        m = 3000
        xy = [np.stack([rng.uniform(-3, cols + 3, m), rng.uniform(-3, 0.7 * rows, m)], 1)]
        z = [rng.uniform(0.5, 6.0, m)]
        xy.append(np.stack([rng.uniform(0, cols, 60), rng.uniform(0, rows, 60)], 1)); z.append(-rng.uniform(0.5, 3.0, 60))
        xy.append(np.stack([rng.uniform(5, cols - 5, 60), rng.uniform(0.75 * rows, rows - 1, 60)], 1)); z.append(np.full(60, 1e-5))
        xy.append(np.stack([rng.uniform(0, cols, 200), rng.uniform(0.75 * rows, rows, 200)], 1)); z.append(np.where(np.arange(200) % 2 == 0, 70.0, 300.0))
        lists.append(V.camera_back_project(k, poses[i], np.concatenate(xy).astype(F32), np.concatenate(z).astype(F32)))
    xyz = np.ascontiguousarray(np.stack(lists), F32)
    gray = rng.integers(1, 256, xyz.shape[:2]).astype(np.uint8)
    return xyz, gray


@OPERATOR_SCALE
@PLANE
@pytest.mark.parametrize("footprint", [1, 3])
def test_render_points_equals_the_host_entry(plane, scale, footprint):
    from test_gpu_render_map import assert_same, check_identities, host_render, to_host
    rows, cols = PLANES[plane]
    xyz, gray = point_lists(plane)
    cap = xyz.shape[1]
    counts = np.array([cap, cap - 37], np.uint32)
    k, poses = cam_of(rows, cols), operator_poses(2)
    for ranges in (None, np.array([[0, cap], [500, 2600]], np.uint32)):
        want = host_render(xyz, gray, counts, k, rows, cols, scale, poses, ranges, footprint)
        got = to_host(V.render_points(dev(xyz), dev(gray), dev(counts, np.int32), k, rows, cols, scale, poses=dev(poses),
                                      ranges=None if ranges is None else dev(ranges, np.int32), footprint=footprint, counts=True, zkey=True))
        assert_same(got, want, f"{plane} scale {scale} footprint {footprint}")
        check_identities(want["counts"], want["zkey"], footprint, "host entry")
    covered = want["zkey"] != np.uint64(V.ZKEY_EMPTY)
    assert (want["depth"][covered] == 65535).any(), "no pixel whose depth saturates"
    assert (want["depth"][covered] == 0).any(), "no covered pixel whose depth rounds to 0"
    assert ((want["depth"][covered] > 0) & (want["depth"][covered] < 65535)).any()


@functools.lru_cache(maxsize=None)
def depth_planes(plane, scale):
    """depth [2, rows, cols] u16 at `scale`: a tilted plane per map, the right third 0.4 m further away (beyond 65535 / 30000 m it sits
    on the clamp), a blob of zeros, 2 % zeros."""
    rows, cols = PLANES[plane]
    rng = np.random.default_rng(rows)
    y, x = np.mgrid[0:rows, 0:cols]
    d = np.empty((2, rows, cols), np.uint16)
    for i in range(2):
        z = 1.2 + 0.3 * i + 0.003 * (1 + i) * x - 0.004 * y
        z[:, 2 * cols // 3:] += 0.4
        q = np.clip(np.rint(z * scale), 1, 65535)
        q[rows // 4:rows // 4 + 5, cols // 5:cols // 5 + 6] = 0
        q[rng.random(q.shape) < 0.02] = 0
        d[i] = q
    return d


JUMP_M = 0.08


@OPERATOR_SCALE
@PLANE
@pytest.mark.parametrize("posed", [False, True], ids=["camera_frame", "posed"])
def test_depth_normals_and_points_normals_equal_the_host_entry(plane, scale, posed):
    import torch
    rows, cols = PLANES[plane]
    depth, k = depth_planes(plane, scale), cam_of(rows, cols)
    poses = operator_poses(2) if posed else None
    d_depth, d_poses = dev(depth, np.int16), (dev(poses) if posed else None)
    for step in (1, 3):
        host = [V.depth_normals_host(depth[i], k, scale, step, JUMP_M, pose7=poses[i] if posed else None) for i in range(2)]
        for o in host:
            assert 2 * int(o["counts"][2]) >= int(o["counts"][1]) > 0 and int(o["counts"][2]) < int(o["counts"][1]), o["counts"]
        out = V.depth_normals(d_depth, k, scale, step, JUMP_M, poses=d_poses, counts=True)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out["normals"].cpu().numpy()), np.stack([o["normals"] for o in host]).view(np.uint32)), (plane, scale, step)
        assert np.array_equal(out["counts"].cpu().numpy().view(np.uint32), np.stack([o["counts"] for o in host]))
    # the list form: a count above capacity and a prefix, a range that overruns the prefix, a pixel outside the plane
    step, cap = 3, 700
    rng = np.random.default_rng(3)
    xs, ys = rng.integers(0, cols, (2, cap)), rng.integers(0, rows, (2, cap))
    xs[:, 5], ys[:, 5] = cols, 1
    pixel = (xs | (ys << 16)).astype(np.uint32)
    list_counts = np.array([cap + 50, 300], np.uint32)
    for rg in (None, np.array([[650, 500], [100, 4000]], np.uint32)):
        want, want_c = np.full((2, cap, 3), -7.0, F32), np.zeros((2, 3), np.uint32)
        for i in range(2):
            want_c[i] = V.depth_normals_host(depth[i], k, scale, step, JUMP_M, pose7=poses[i] if posed else None, pixel=pixel[i],
                                             count=int(list_counts[i]), range2=None if rg is None else rg[i], normals=want[i])["counts"]
        out = V.points_normals(d_depth, dev(pixel, np.int32), dev(list_counts, np.int32), k, scale, step, JUMP_M, poses=d_poses,
                               ranges=None if rg is None else dev(rg, np.int32), normals=torch.full((2, cap, 3), -7.0, device="cuda"), counts=True)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out["normals"].cpu().numpy()), want.view(np.uint32)), (plane, scale)
        assert np.array_equal(out["counts"].cpu().numpy().view(np.uint32), want_c)
        assert (want[1, 300:] == -7.0).all() and (want_c[:, 2] > 0).all()


# ------------------------------------------------------------------------------------------------------------ 7
SEQ_ROWS, SEQ_COLS, SEQ_L, N_SEQ, N_FRAMES = 60, 80, 3, 2, 12
SEQ_SCALE, SEQ_VARIANCE = 1000.0, 1.0
SEQ_INTR = O.scaled_intrinsics(SEQ_ROWS, SEQ_COLS)
STEP_TWIST = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001])   # the motion of test_gpu_fused.py's sequence test, per frame ...
SPEED = (1.0, 3.0)                                                     # ... times this, per sequence
FILTER = (0.02, 255, 1)
NORMALS = (2, 0.05)
MAX_KF = 16
SEQ_MODE = pytest.mark.parametrize("mode", [1, 0], ids=["dense", "c2f"])


@functools.lru_cache(maxsize=None)
def sequences():
    """gray [F, n, rows, cols] u8 and depth u16 re-quantised at SEQ_SCALE. Checked with the oracle alone: sequence 0 promotes at frame 9,
    sequence 1 at frames 3, 6 and 9 (asserted below on the oracle's own run)."""
    gray = np.empty((N_FRAMES, N_SEQ, SEQ_ROWS, SEQ_COLS), np.uint8)
    depth = np.empty((N_FRAMES, N_SEQ, SEQ_ROWS, SEQ_COLS), np.uint16)
    for k in range(N_FRAMES):
        for q in range(N_SEQ):
            g, d = O.synth_frame(77 + q, STEP_TWIST * k * SPEED[q], SEQ_ROWS, SEQ_COLS, SEQ_INTR, frame_salt=k)
            gray[k, q], depth[k, q] = g, requantise(d, SEQ_SCALE)
    return gray, depth


def seq_config(mode, arith):
    return vcfg(SEQ_L, SEQ_INTR, mode, SEQ_SCALE, SEQ_VARIANCE, arith)


@SEQ_MODE
def test_sequence_trackers_reference_poses_equal_the_oracle(mode):
    gray, depth = sequences()
    ref = O.track_sequences(ocfg(SEQ_L, SEQ_INTR, mode, SEQ_SCALE, SEQ_VARIANCE), gray, depth, n_threads=N_SEQ)
    assert (ref["status"] == 0).all() and ref["changed_keyframe"].any(axis=1).all(), "every sequence promotes at least once"
    tr = V.Trackers(seq_config(mode, V.ARITH_REFERENCE), N_SEQ, SEQ_ROWS, SEQ_COLS)
    frames = [(dev(gray[k]), dev(depth[k], np.int16)) for k in range(N_FRAMES)]
    tr.init(*frames[0])
    for k in range(1, N_FRAMES):
        tr.track(*frames[k])
        poses, status, kf = tr.current_frames()
        st = tr.stats()
        assert (status == ref["status"][:, k - 1]).all(), k
        assert (bits(poses) == bits(ref["poses"][:, k - 1])).all(), f"frame {k}: poses differ from the oracle's bits"
        assert (st["change_keyframe"] == ref["changed_keyframe"][:, k - 1]).all(), k


@functools.lru_cache(maxsize=None)
def mapped_run(mode):
    """The same sequences with the depth filter, the map at level 0, its normals, and a rendering of the map after every frame."""
    import torch
    from test_gpu_render_map import to_host
    from test_gpu_trackers_map import read_map
    gray, depth = sequences()
    cap = SEQ_ROWS * SEQ_COLS * N_FRAMES
    tr = V.Trackers(seq_config(mode, V.ARITH_REFERENCE), N_SEQ, SEQ_ROWS, SEQ_COLS)
    tr.enable_depth_filter(*FILTER)
    tr.enable_map(0, cap, MAX_KF, 0)
    tr.enable_map_normals(*NORMALS)
    frames = [(dev(gray[k]), dev(depth[k], np.int16)) for k in range(N_FRAMES)]
    rec = []
    for k, (g, d) in enumerate(frames):
        if k == 0:
            tr.init(g, d)
        else:
            tr.track(g, d)
        poses, status, kf = tr.current_frames()
        dd, ww = tr.keyframe_depth()
        r = dict(poses=poses, status=status, kf=kf, stats=tr.stats().copy() if k else None, depth=dd.cpu().numpy().view(np.uint16), weight=ww.cpu().numpy())
        if k in (N_FRAMES // 2, N_FRAMES - 1):
            r["map"] = read_map(tr)
            r["render"] = {f: to_host(tr.render_map(level=0, footprint=f, counts=True, zkey=True)) for f in (1, 3)}
        rec.append(r)
    normals = tr.map_normals().cpu().numpy()
    torch.cuda.synchronize()
    return rec, frames, read_map(tr), normals, cap


@SEQ_MODE
def test_sequence_trackers_depth_filter_at_scale_1000(mode):
    """test_gpu_trackers_depth_filter.py's shadow fusion with the scale passed through, and the host merge at that scale on the shadow's keys."""
    import torch
    rec, frames, _, _, _ = mapped_run(mode)
    _, depth = sequences()
    assert all((r["status"] == 0).all() for r in rec)
    assert np.array_equal(rec[0]["depth"], depth[0]) and np.array_equal(rec[0]["weight"], (depth[0] != 0).astype(np.uint8))
    shadow = V.Batch(seq_config(mode, V.ARITH_REFERENCE), N_SEQ, SEQ_ROWS, SEQ_COLS)
    counts, promoted_any = np.zeros(6, np.int64), 0
    for k in range(1, N_FRAMES):
        before, after = rec[k - 1], rec[k]
        promoted = np.nonzero(after["kf"] != before["kf"])[0]
        for s in np.nonzero(after["kf"] == before["kf"])[0]:
            assert np.array_equal(after["depth"][s], before["depth"][s]) and np.array_equal(after["weight"][s], before["weight"][s]), (k, s)
        if len(promoted) == 0:
            continue
        promoted_any += len(promoted)
        kf_gray = torch.stack([frames[before["kf"][s]][0][s] for s in promoted]).contiguous()
        shadow.prepare_keyframes(kf_gray, dev(before["depth"][promoted], np.int16))
        m = shadow.fuse_depth(dev(after["stats"]["lm_model"][promoted]), frames[k][1][promoted].contiguous(), FILTER[0], kf_weight=dev(before["weight"][promoted]),
                              max_weight=FILTER[1], fill_min_weight=FILTER[2], zkey=True, counts=True)
        torch.cuda.synchronize()
        assert np.array_equal(m["depth"].cpu().numpy().view(np.uint16), after["depth"][promoted]), f"frame {k}: fused depth differs from the shadow batch"
        assert np.array_equal(m["weight"].cpu().numpy(), after["weight"][promoted]), f"frame {k}: fused weight differs from the shadow batch"
        zkey = m["zkey"].cpu().numpy().view(np.uint64)
        for i, s in enumerate(promoted):
            d, w, c = V.fuse_depth_pixels(SEQ_SCALE, FILTER[0], zkey[i], depth[k, s], before["weight"][s], FILTER[1], FILTER[2])
            assert np.array_equal(d, after["depth"][s]) and np.array_equal(w, after["weight"][s]), f"frame {k} sequence {s}: host merge at scale {SEQ_SCALE}"
            assert c.tolist() == m["counts"].cpu().numpy()[i].tolist()
            counts += c
    assert promoted_any >= 2 and counts[0] > 0 and counts[3] > 0, f"promotions {promoted_any}, cases {counts}"
    assert max(r["weight"].max() for r in rec) >= 2


@SEQ_MODE
def test_sequence_trackers_map_and_normals_at_scale_1000(mode):
    """test_gpu_trackers_map.py's shadow point clouds and test_gpu_trackers_map_normals.py's host normals with the scale passed through; the
    map's points are also the host back-projection of their pixels' keyframe depth at that scale."""
    import torch
    rec, frames, m, normals, cap = mapped_run(mode)
    k5 = np.asarray(SEQ_INTR, F32)
    shadow = V.Batch(seq_config(mode, V.ARITH_REFERENCE), N_SEQ, SEQ_ROWS, SEQ_COLS)
    seen, total = np.zeros(N_SEQ, np.int64), np.zeros(N_SEQ, np.int64)
    for k in range(N_FRAMES):
        new = np.arange(N_SEQ) if k == 0 else np.nonzero(rec[k]["kf"] != rec[k - 1]["kf"])[0]
        if len(new) == 0:
            continue
        shadow.prepare_keyframes(frames[k][0][new].contiguous(), dev(rec[k]["depth"][new], np.int16))
        out = shadow.point_cloud(0, poses=dev(rec[k]["poses"][new]), capacity=cap, gray=True)
        torch.cuda.synchronize()
        out = {name: t.cpu().numpy() for name, t in out.items()}
        for i, s in enumerate(new):
            seg, count = m["segments"][s, int(seen[s])], int(out["counts"][i])
            where = f"frame {k} sequence {s}"
            assert seg["frame"] == k and seg["first"] == total[s] and seg["count"] == count and count > 0, (where, seg, count, total[s])
            assert bits(seg["pose7"]).tolist() == bits(rec[k]["poses"][s]).tolist(), where
            a, b = int(total[s]), int(total[s]) + count
            assert np.array_equal(bits(m["xyz"][s, a:b]), bits(out["xyz"][i, :count])), f"{where}: xyz differs from the shadow batch"
            assert np.array_equal(m["pixel"][s, a:b], out["pixel"][i, :count].view(np.uint32)) and np.array_equal(m["gray"][s, a:b], out["gray"][i, :count]), where
            # the host statement at this scale: back_project(pixel, 1 / from_depth(scale, keyframe depth)) through the keyframe's pose
            x, y = (m["pixel"][s, a:b] & 0xffff).astype(np.int64), (m["pixel"][s, a:b] >> 16).astype(np.int64)
            plane = rec[k]["depth"][s]
            assert (plane[y, x] > 0).all(), where
            if mode == 1:
                assert count == int((plane > 0).sum()), f"{where}: dense level 0 lists every pixel with a depth"
            host = V.camera_back_project(k5, rec[k]["poses"][s], np.stack([x, y], 1).astype(F32), F32(1.0) / V.from_depth(SEQ_SCALE, plane[y, x]))
            assert np.array_equal(bits(m["xyz"][s, a:b]), bits(host)), f"{where}: xyz differs from the host back-projection at scale {SEQ_SCALE}"
            want = V.depth_normals_host(plane, k5, SEQ_SCALE, NORMALS[0], NORMALS[1], pose7=seg["pose7"], pixel=m["pixel"][s, a:b])["normals"]
            assert np.array_equal(bits(normals[s, a:b]), bits(want)), f"{where}: normals differ from the host entry at scale {SEQ_SCALE}"
            assert 2 * int(want.any(-1).sum()) >= count, f"{where}: fewer than half of the points get a normal"
            seen[s] += 1
            total[s] += count
    assert (m["n_segments"] == seen).all() and (m["counts"] == total).all() and (seen >= 2).all() and total.max() <= cap


@SEQ_MODE
def test_sequence_trackers_render_map_at_scale_1000(mode):
    """test_gpu_render_map.py's composition: the handle's own map rendered from the current poses == the host entry at that scale."""
    from test_gpu_render_map import assert_same, check_identities, host_render
    rec = mapped_run(mode)[0]
    k5 = np.asarray(SEQ_INTR, F32)
    checked = 0
    for r in rec:
        if "render" not in r:
            continue
        st = r["map"]
        for f, got in r["render"].items():
            want = host_render(st["xyz"], st["gray"], st["counts"], k5, SEQ_ROWS, SEQ_COLS, SEQ_SCALE, r["poses"], None, f)
            assert_same(got, want, f"footprint {f}")
            check_identities(want["counts"], want["zkey"], f, "host entry")
            # (dense: every pixel with a depth is a map point; coarse-to-fine: the candidates only, a sparse map)
            assert (want["counts"][:, 3] > (SEQ_ROWS * SEQ_COLS // 2 if mode == 1 else 500)).all(), "the map covers too little of the view"
            wrong = host_render(st["xyz"], st["gray"], st["counts"], k5, SEQ_ROWS, SEQ_COLS, 5000.0, r["poses"], None, f)
            assert not np.array_equal(wrong["depth"], want["depth"])   # (the comparison can tell the scales apart)
            checked += 1
    assert checked == 4
