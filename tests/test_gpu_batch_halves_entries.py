"""A dense step run as two overlapped slices (batch.cpp plan_halves / make_slice / slice_lm / track_pairs_halves), through every entry that
takes one or reads the handle after one. tests/test_gpu_batch_halves.py pins the call's own outputs without an initial guess; this module
pins what that one cannot notice: host-side pointer arithmetic that only shows with per-pair guesses, with absent outputs, in the state
the two slices leave in the handle, in the calls that follow on the same handle, and in the other entries that build a handle with the plan.

Both sides of every comparison live in this process: VORS_BATCH_HALVES (0 = plan off, 1 = plan from 2 pairs on) is read when a handle is
created and is set right before each creation; VORS_LM_SPLIT_LEVELS=2 makes the small images take the evaluation rounds of 640x480.
Every comparison is of BYTES, plan on against plan off — no tolerance appears in this file. Dense mode everywhere, FUSED and REFERENCE
everywhere, EXACT once per family, huber_delta 0 and 10 at 60x80. Pair i of a scene is rendered from seed + i, so no two pairs are alike.

Shapes and cuts (the first slice holds h pairs; restated from plan_halves in cut() below and asserted against this table):
  60x80,   3 levels, capacity 8:  n = 8 -> h = 4, n = 7 -> h = 4, n = 3 -> h = 2
  61x83,   3 levels, capacity 40: rows * cols is odd, the cut is rounded up to 16 pairs: n = 40 -> h = 32, n = 23 -> h = 16
  120x160, 4 levels, capacity 8:  n = 8 -> h = 4 (the only four-level case)

Entries covered:
  1. vors_batch_track_pairs with a prev_poses7 of its own per pair: poses, status, every vors_pair_stats field, prediction log; REFERENCE
     also against the oracle started from the same guesses (test_gpu_reference's pair check). The guesses matter with the plan off alone.
  2. the same call without out_stats, without prev_poses7, without both; sentinel bands behind every output buffer stay untouched.
  3. every reader of the handle after a halved step, every level: eval_level, eval_pairs (full / energy, two models per pair),
     pose_information, residual_maps, reproject_depth, point_cloud (with and without a keep mask), fuse_depth, keyframe_image,
     current_image, points; pyramids and points of pairs h and n - 1 also against the oracle; pair h's products differ from pair 0's.
  4. follow-on calls on one handle: track_current against the keyframes two slices prepared; prepare_keyframes + track_current of another
     scene, then the first scene again (same bits as the first time); n = 1 (plain path), n = capacity (halved), n = 1 again.
  5. caller buffers that are not 16-byte aligned (5 bytes / 2 uint16 elements into their allocations), against the aligned run as well.
  6. vors_multi_* (one device suffices: the handle is asked for one device so that its shard holds all 8 pairs), the one-shot host entry
     vors_track_pairs in both layouts, and vors_pipeline_*, whose ring slots opt out of the plan.
  7. vors_batch_workspace_bytes with the plan on.
  8. the default threshold with no knob: 4096 pairs (the plan) against 4095 pairs (the plain path) on one 4096-pair handle.

What could not be built: the Python Pipeline wrapper (and the C ABI behind it) exposes no workspace figure, so the pipeline's opt-out is
asserted through bit equality with the plain batch steps only; the figure is compared if a later wrapper exposes it. GPU only."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from oracle import oracle as O

import test_gpu_large_batches as LB
import test_gpu_reference as TR

# rows, cols, levels, capacity
SHAPES = {"60x80": (60, 80, 3, 8), "61x83": (61, 83, 3, 40), "120x160": (120, 160, 4, 8)}
CUTS = {("60x80", 8): 4, ("60x80", 7): 4, ("60x80", 3): 2, ("61x83", 40): 32, ("61x83", 23): 16, ("120x160", 8): 4}
SEEDS = {"60x80": 0x5EED4E000, "61x83": 0x5EED4E400, "120x160": 0x5EED4E800}
ARITHS = {"fused": V.ARITH_FUSED, "reference": V.ARITH_REFERENCE, "exact": V.ARITH_EXACT}
STAT_FIELDS = ("lm_model", "optical_flow", "change_keyframe", "nb_iter", "n_points", "energy", "nb_grad_evals")
ITEM = V.PAIR_STATS_DTYPE.itemsize
GUARD = 16                      # pairs of sentinel behind every output buffer
SENT_F, SENT_I, SENT_B = 7.0, -77, 0xA5
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1], np.float32)

# (shape, n, arithmetic, huber): every shape and cut in FUSED and REFERENCE, Huber at 60x80, EXACT once
ALL_CASES = ([("60x80", n, a, hub) for n in (8, 7, 3) for a in ("fused", "reference") for hub in (0.0, 10.0)] + [("60x80", 8, "exact", 0.0)] +
             [("61x83", n, a, 0.0) for n in (40, 23) for a in ("fused", "reference")] + [("120x160", 8, a, 0.0) for a in ("fused", "reference")])
# one count per shape: an odd second slice at 60x80, a count below the capacity at 61x83
ONE_PER_SHAPE = ([(s, n, a, 0.0) for s, n in (("60x80", 7), ("61x83", 23), ("120x160", 8)) for a in ("fused", "reference")] +
                 [("60x80", 8, "fused", 10.0), ("60x80", 8, "reference", 10.0), ("60x80", 8, "exact", 0.0)])


def ids(cases):
    return [f"{s}_n{n}_{a}_h{hub:g}" for s, n, a, hub in cases]


def cut(shape, n):
    """plan_halves' rule with the plan forced: half the pairs, rounded up to the count that keeps a slice's level-0 images 16-byte aligned."""
    rows, cols = SHAPES[shape][:2]
    align = 1
    while align < 16 and (rows * cols * align) % 16:
        align *= 2
    h = ((n + 1) // 2 + align - 1) // align * align
    return h if 1 <= h < n else 0


# ---------------------------------------------------------------------------------------------- scenes, guesses and the oracle, once per module
@functools.lru_cache(maxsize=None)
def scene(shape, motion=1.0, seed_off=0):
    """capacity pairs of a shape on the device (never written to): kf gray, kf depth, cur gray, cur depth, ground-truth models. The
    keyframe depends on the seed alone; `motion` scales the twist of the current frame, so another motion is another current frame of the
    same keyframe."""
    import torch
    rows, cols, _, cap = SHAPES[shape]
    out = V.synth_render_pairs(SEEDS[shape] + seed_off, cap, rows, cols, V.scaled_intrinsics(rows, cols), motion_scale=motion, want_cur_depth=True)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def host_scene(shape, motion=1.0, seed_off=0):
    kg, kd, cg = scene(shape, motion, seed_off)[:3]
    return kg.cpu().numpy(), kd.cpu().numpy().view(np.uint16), cg.cpu().numpy()


@functools.lru_cache(maxsize=None)
def guesses(shape):
    """prev_poses7 of every pair of scene(shape): the pair's ground-truth pose (the inverse of the rendered keyframe -> current model) times
    a seeded rotation of 0.01 .. 0.02 rad about a random axis and a shift of 0.01 .. 0.02 m in a random direction, another for each pair."""
    cap = SHAPES[shape][3]
    gt = scene(shape)[4].cpu().numpy()
    rng = np.random.default_rng(SEEDS[shape])
    prev = np.empty((cap, 7), np.float32)
    for p in range(cap):
        axis, shift = rng.normal(size=3), rng.normal(size=3)
        angle = rng.uniform(0.01, 0.02)
        axis *= np.sin(angle / 2) / np.linalg.norm(axis)
        shift *= rng.uniform(0.01, 0.02) / np.linalg.norm(shift)
        delta = np.concatenate([shift, axis, [np.cos(angle / 2)]]).astype(np.float32)
        prev[p] = O.iso_mul(O.iso_inverse(gt[p]), delta)
    prev.setflags(write=False)
    return prev


@functools.lru_cache(maxsize=None)
def oracle_from_guesses(shape, n, huber):
    rows, cols, L, _ = SHAPES[shape]
    kg, kd, cg = host_scene(shape)
    cfg = O.make_config(L, V.scaled_intrinsics(rows, cols), candidates_mode=1, huber_delta=huber)
    return O.track_pairs(cfg, kg[:n], kd[:n], cg[:n], init_poses7=guesses(shape)[:n], n_threads=8)


# ---------------------------------------------------------------------------------------------- handles, calls, comparisons
def config(shape, arith, huber=0.0):
    rows, cols, L, _ = SHAPES[shape]
    intr = V.scaled_intrinsics(rows, cols)
    return V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), huber_delta=huber, arithmetic=ARITHS[arith],
                    candidates_mode=V.CANDIDATES_DENSE)


def knobs(monkeypatch, knob):
    LB.set_knobs(monkeypatch, {"VORS_LM_SPLIT_LEVELS": "2", "VORS_BATCH_HALVES": knob})


def handle(monkeypatch, knob, shape, arith, huber=0.0, cap=None):
    knobs(monkeypatch, knob)
    rows, cols, _, c = SHAPES[shape]
    return V.Batch(config(shape, arith, huber), cap or c, rows, cols)


def out_buffers(n, stats=True):
    """Output buffers of n pairs with GUARD pairs of sentinel behind each (the statistics start as V.stats_tensor's zeros)."""
    import torch
    poses = torch.full((n + GUARD, 7), SENT_F, dtype=torch.float32, device="cuda")
    status = torch.full((n + GUARD,), SENT_I, dtype=torch.int32, device="cuda")
    st = None
    if stats:
        st = torch.zeros((n + GUARD) * ITEM, dtype=torch.uint8, device="cuda")
        st[n * ITEM:] = SENT_B
    return poses, status, st


def collect(b, n, bufs, what):
    """-> the outputs of a call as numpy + the device tensors (for the readers); the sentinel bands must have stayed as they were."""
    import torch
    torch.cuda.synchronize()
    poses, status, st = bufs
    assert (poses[n:] == SENT_F).all() and (status[n:] == SENT_I).all(), f"{what}: the call wrote behind out_poses7 / out_status"
    assert (status[:n] != SENT_I).all(), f"{what}: a status was not written"
    res = dict(poses=poses[:n].cpu().numpy(), status=status[:n].cpu().numpy(), pred_log=b.lm_predict_log(n) if b is not None else np.zeros(n, np.int32),
               t_poses=poses[:n], t_stats=None, stats=None)
    if st is not None:
        assert (st[n * ITEM:] == SENT_B).all(), f"{what}: the call wrote behind out_stats"
        res["t_stats"] = st[:n * ITEM]
        res["stats"] = V.decode_stats(res["t_stats"])
    return res


def to_device(prev, n):
    import torch
    return None if prev is None else torch.from_numpy(np.array(prev[:n], np.float32)).cuda()


def track(b, images, n, prev=None, stats=True, what="track_pairs"):
    bufs = out_buffers(n, stats)
    b.track_pairs(images[0][:n], images[1][:n], images[2][:n], *bufs, prev_poses7=to_device(prev, n))
    return collect(b, n, bufs, what)


def track_current(b, cur_gray, n, prev=None, what="track_current"):
    bufs = out_buffers(n)
    b.track_current(cur_gray[:n], *bufs, prev_poses7=to_device(prev, n))
    return collect(b, n, bufs, what)


def fields(res, levels=None):
    """name -> array of every output of a call. `levels`: the per-level statistics are cut to the levels of the pyramid (for an entry whose
    statistics do not start from zeros: the entries of the levels a pyramid does not have are not written)."""
    out = {f: res[f] for f in ("poses", "status", "pred_log")}
    if res["stats"] is not None:
        out.update({f: np.ascontiguousarray(res["stats"][f]) for f in STAT_FIELDS})
        if levels is not None:
            out.update({f: np.ascontiguousarray(out[f][:, :levels]) for f in ("nb_iter", "n_points", "energy", "nb_grad_evals")})
    return out


def assert_same(got, want, what, only=None, levels=None):
    a, b = fields(got, levels), fields(want, levels)
    for f in (only or sorted(set(a) & set(b))):
        x, y = a[f], b[f]
        assert x.shape == y.shape, f"{what}: {f} has shapes {x.shape} and {y.shape}"
        if x.tobytes() != y.tobytes():
            rows = np.flatnonzero((x.reshape(len(x), -1).view(np.uint8) != y.reshape(len(y), -1).view(np.uint8)).any(axis=1))
            raise AssertionError(f"{what}: {f} differs in pairs {rows[:12].tolist()} ({len(rows)} of {len(x)})")


def assert_same_arrays(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in got:
        x, y = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: {k} differs"


def test_the_cuts_are_the_ones_this_module_is_named_after():
    for (shape, n), h in CUTS.items():
        assert cut(shape, n) == h, (shape, n)
    assert cut("60x80", 1) == 0 and cut("60x80", 4096) == 2048 and cut("61x83", 16) == 0


# ---------------------------------------------------------------------------------------------- 1. initial guesses
@pytest.mark.parametrize("shape,n,arith,huber", ALL_CASES, ids=ids(ALL_CASES))
def test_every_pair_starts_from_its_own_guess(monkeypatch, shape, n, arith, huber):
    """prev_poses7 reaches the second slice advanced by h pairs. The guesses are guesses(shape): ground truth times a rotation of 0.01 ..
    0.02 rad and a shift of 0.01 .. 0.02 m per pair (nothing had to be raised). Not vacuous, with the plan off alone: handing every pair
    the guess of the pair h places before it (np.roll by h, what an un-advanced pointer gives the second slice) changes the iteration
    counts or the pose bits of at least half of the second slice's pairs."""
    h = CUTS[shape, n]
    L = SHAPES[shape][2]
    images, prev = scene(shape), guesses(shape)[:n]
    b_off, b_on = handle(monkeypatch, "0", shape, arith, huber), handle(monkeypatch, "1", shape, arith, huber)
    off, on = track(b_off, images, n, prev), track(b_on, images, n, prev)
    assert_same(on, off, f"{shape} n={n} {arith}: plan on against plan off")
    rolled = track(b_off, images, n, np.roll(prev, h, axis=0))
    changed = ((rolled["stats"]["nb_iter"] != off["stats"]["nb_iter"]).any(axis=1) |
               (rolled["poses"].view(np.uint32) != off["poses"].view(np.uint32)).any(axis=1))[h:]
    assert 2 * int(changed.sum()) >= len(changed), f"the guesses decide {int(changed.sum())} of the second slice's {len(changed)} pairs only"
    no_guess = track(b_off, images, n)
    assert (no_guess["poses"].view(np.uint32) != off["poses"].view(np.uint32)).any(axis=1)[:h].any(), "the first slice's guesses do not matter"
    if arith == "reference":
        ref = oracle_from_guesses(shape, n, huber)
        TR.assert_pairs_identical(ref, on["poses"], on["status"], on["stats"], L, f"{shape} n={n} huber {huber}: plan on against the oracle from the same guesses")


# ---------------------------------------------------------------------------------------------- 2. nullable outputs
@pytest.mark.parametrize("shape,n,arith,huber", ONE_PER_SHAPE + [("60x80", 3, "fused", 0.0), ("61x83", 40, "reference", 0.0)],
                         ids=ids(ONE_PER_SHAPE + [("60x80", 3, "fused", 0.0), ("61x83", 40, "reference", 0.0)]))
def test_absent_statistics_and_absent_guesses(monkeypatch, shape, n, arith, huber):
    """out_stats and prev_poses7 are nullable and slice_lm advances each only where it is there: every combination gives the poses and
    statuses of the call that has both sides of it, and (collect) nothing is written behind any output buffer."""
    images, prev = scene(shape), guesses(shape)[:n]
    b_off, b_on = handle(monkeypatch, "0", shape, arith, huber), handle(monkeypatch, "1", shape, arith, huber)
    full = track(b_on, images, n, prev)
    assert_same(full, track(b_off, images, n, prev), "guesses and statistics")
    assert_same(track(b_on, images, n, prev, stats=False), full, "no statistics", only=("poses", "status", "pred_log"))
    plain = track(b_on, images, n)
    assert_same(plain, track(b_off, images, n), "statistics, no guesses")
    assert_same(track(b_on, images, n, stats=False), plain, "neither", only=("poses", "status", "pred_log"))
    assert_same(track(b_off, images, n, stats=False), plain, "neither, plan off", only=("poses", "status", "pred_log"))
    assert plain["poses"].tobytes() != full["poses"].tobytes()
    assert_same(track(b_on, images, n, prev), full, "the full call again")


# ---------------------------------------------------------------------------------------------- 3. every reader of the handle
def read_everything(b, res, shape, n, h, arith):
    """Every product and inspection entry of handle b after the step that gave `res` -> name -> numpy array."""
    import torch
    rows, cols, L, _ = SHAPES[shape]
    cd = scene(shape)[3][:n]
    out = {}
    t_stats, t_poses = res["t_stats"], res["t_poses"]
    tracked = np.ascontiguousarray(res["stats"]["lm_model"])
    two = torch.from_numpy(np.stack([tracked, np.tile(IDENTITY, (n, 1))], axis=1).copy()).cuda()
    rng = np.random.default_rng(n * 1000 + rows)
    watched, inspected = sorted({0, h - 1, h, n - 1}), sorted({h - 1, h, n - 1})

    def put(prefix, d):
        for k, t in d.items():
            out[f"{prefix}/{k}"] = t.cpu().numpy()

    for l in range(L):
        rl, cl = rows >> l, cols >> l
        for p in watched:
            for name, m in (("tracked", tracked[p]), ("identity", IDENTITY)):
                e, cnt, g, H = b.eval_level(p, l, m, ARITHS[arith])
                out[f"eval_level/l{l}/p{p}/{name}"] = np.concatenate([np.array([e, cnt], np.float64), g.astype(np.float64), H.astype(np.float64).ravel()])
        out[f"eval_pairs/l{l}/full"] = b.eval_pairs(l, two, what="full").cpu().numpy()
        out[f"eval_pairs/l{l}/energy"] = b.eval_pairs(l, two, what="energy").cpu().numpy()
        out[f"eval_pairs/l{l}/at_stats"] = b.eval_pairs(l, t_stats).cpu().numpy()
        put(f"pose_information/l{l}", dict(zip(("info", "cov", "sigma2", "flags"), b.pose_information(l, t_stats))))
        put(f"residual_maps/l{l}", b.residual_maps(l, t_stats, residuals=True, warp=True, hist=True, scale=True))
        put(f"reproject_depth/l{l}", b.reproject_depth(l, t_stats, cur_depth=cd if l == 0 else None, tol_m=0.05, pred_z=True, pred_depth=True,
                                                       residual=l == 0, counts=True))
        keep = torch.from_numpy(rng.integers(0, 2, (n, rl, cl), dtype=np.uint8)).cuda()
        for name, mask in (("all", None), ("masked", keep)):
            # a list is written up to its count only: the buffers start from sentinels, so that whole buffers can be compared
            bufs = dict(xyz=torch.full((n, rl * cl, 3), SENT_F, dtype=torch.float32, device="cuda"),
                        pixel=torch.full((n, rl * cl), -1, dtype=torch.int32, device="cuda"),
                        gray=torch.full((n, rl * cl), SENT_B, dtype=torch.uint8, device="cuda"), counts=torch.full((n,), -1, dtype=torch.int32, device="cuda"))
            put(f"point_cloud/l{l}/{name}", b.point_cloud(l, poses=t_poses, keep=mask, **bufs))
        for p in inspected:
            out[f"keyframe_image/l{l}/p{p}"] = b.keyframe_image(p, l)
            out[f"current_image/l{l}/p{p}"] = b.current_image(p, l)
            for k, a in zip(("xy", "idepth", "jac", "tmpl"), b.points(p, l)):
                out[f"points/l{l}/p{p}/{k}"] = a
    put("fuse_depth", b.fuse_depth(t_stats, cd, 0.05, depth=True, weight=True, zkey=True, counts=True))
    return out


@pytest.mark.parametrize("shape,n,arith,huber", ONE_PER_SHAPE, ids=ids(ONE_PER_SHAPE))
def test_every_reader_of_the_handle_after_a_halved_step(monkeypatch, shape, n, arith, huber):
    """The state two slices wrote through advanced Records and pyramids is the state the plain step writes, for every entry that documents
    "the handle as it is after prepare + track"; the pyramids and the points of pairs h and n - 1 are also the oracle's, so that plan on
    and plan off do not agree on something wrong. Not vacuous: at level 0 pair h's products are not pair 0's (the scenes differ, so a
    pointer that was not advanced would show pair 0's bits in pair h's place)."""
    h = CUTS[shape, n]
    rows, cols, L, _ = SHAPES[shape]
    images, prev = scene(shape), guesses(shape)[:n]
    got = {}
    for knob in ("0", "1"):
        b = handle(monkeypatch, knob, shape, arith, huber)
        got[knob] = read_everything(b, track(b, images, n, prev), shape, n, h, arith)
    assert_same_arrays(got["1"], got["0"], f"{shape} n={n} {arith}: readers after a halved step against the plain step")
    on = got["1"]
    for key in ("eval_pairs/l0/full", "pose_information/l0/info", "residual_maps/l0/residuals", "residual_maps/l0/hist", "reproject_depth/l0/pred_z",
                "reproject_depth/l0/residual", "point_cloud/l0/all/xyz", "point_cloud/l0/masked/pixel", "fuse_depth/depth", "fuse_depth/zkey"):
        assert on[key][h].tobytes() != on[key][0].tobytes(), f"{key}: pair {h} shows pair 0's bits"
    kg, kd, cg = host_scene(shape)
    ocfg = O.make_config(L, V.scaled_intrinsics(rows, cols), candidates_mode=1, huber_delta=huber)
    for p in sorted({h, n - 1}):
        want_k, want_c = O.mean_pyramid(kg[p], L), O.mean_pyramid(cg[p], L)
        tr = O.Tracker(ocfg, 0.0, kd[p], 0.0, kg[p])
        for l in range(L):
            assert (on[f"keyframe_image/l{l}/p{p}"] == want_k[l]).all() and (on[f"current_image/l{l}/p{p}"] == want_c[l]).all(), f"pyramids of pair {p}, level {l}"
            xy, iz, jac = (on[f"points/l{l}/p{p}/{k}"] for k in ("xy", "idepth", "jac"))
            oxy, oiz, ojac = tr.points(l)
            assert xy.shape == oxy.shape and len(xy) > 0, f"pair {p} level {l}: {len(xy)} vs {len(oxy)} points"
            o1, o2 = np.lexsort((xy[:, 1], xy[:, 0])), np.lexsort((oxy[:, 1], oxy[:, 0]))
            assert (xy[o1] == oxy[o2]).all() and TR.same_bits(iz[o1], oiz[o2]) and TR.same_bits(jac[o1], ojac[o2]), f"points of pair {p}, level {l}"


# ---------------------------------------------------------------------------------------------- 4. follow-on calls on one handle
def eval0(b, res):
    return {"eval_pairs/l0": b.eval_pairs(0, res["t_stats"]).cpu().numpy()}


def both_plans(monkeypatch, shape, arith, huber, script):
    """script(handle) -> list of (name, result, eval_pairs at level 0) per step, run with the plan off and on; every step equal."""
    got = {knob: script(handle(monkeypatch, knob, shape, arith, huber)) for knob in ("0", "1")}
    for (name, r_off, e_off), (_, r_on, e_on) in zip(got["0"], got["1"]):
        assert_same(r_on, r_off, f"{shape} {arith} {name}: plan on against plan off")
        assert_same_arrays(e_on, e_off, f"{shape} {arith} {name}: eval_pairs at level 0")
    return got


@pytest.mark.parametrize("shape,n,arith,huber", ONE_PER_SHAPE, ids=ids(ONE_PER_SHAPE))
def test_track_current_against_the_keyframes_two_slices_prepared(monkeypatch, shape, n, arith, huber):
    """(a) a halved track_pairs, then track_current of other current frames of the same keyframes (the scene rendered at half the motion)
    from the first call's poses: one launch over the records, pyramids and workspace that two slices on two streams left behind."""
    images, other_cur = scene(shape), scene(shape, motion=0.5)[2]

    def script(b):
        first = track(b, images, n, guesses(shape)[:n])
        e_first = eval0(b, first)
        second = track_current(b, other_cur, n, prev=first["poses"])
        return [("track_pairs", first, e_first), ("track_current", second, eval0(b, second))]

    got = both_plans(monkeypatch, shape, arith, huber, script)
    assert got["1"][0][1]["poses"].tobytes() != got["1"][1][1]["poses"].tobytes(), "the second set of current frames is the first"


@pytest.mark.parametrize("shape,n,arith,huber", ONE_PER_SHAPE, ids=ids(ONE_PER_SHAPE))
def test_the_plain_entries_between_two_halved_steps(monkeypatch, shape, n, arith, huber):
    """(b) halved track_pairs, prepare_keyframes + track_current of another scene (the first slice's workspace and hand-over counters after
    the second slice used its own), then the first scene again: the third result is the first, bit for bit."""
    images, other = scene(shape), scene(shape, seed_off=500)

    def script(b):
        first = track(b, images, n, guesses(shape)[:n])
        e_first = eval0(b, first)
        b.prepare_keyframes(other[0][:n], other[1][:n])
        second = track_current(b, other[2], n)
        e_second = eval0(b, second)
        third = track(b, images, n, guesses(shape)[:n])
        return [("first", first, e_first), ("other scene", second, e_second), ("first scene again", third, eval0(b, third))]

    got = both_plans(monkeypatch, shape, arith, huber, script)
    for knob in ("0", "1"):
        steps = got[knob]
        assert_same(steps[2][1], steps[0][1], f"plan {knob}: the first scene again")
        assert_same_arrays(steps[2][2], steps[0][2], f"plan {knob}: the first scene again, eval_pairs")
        assert steps[1][1]["poses"].tobytes() != steps[0][1]["poses"].tobytes()


@pytest.mark.parametrize("shape,arith", [(s, a) for s in SHAPES for a in ("fused", "reference")], ids=[f"{s}_{a}" for s in SHAPES for a in ("fused", "reference")])
def test_one_pair_then_the_capacity_then_one_pair(monkeypatch, shape, arith):
    """(c) n = 1 is below the forced threshold and takes the plain path on a handle that has the plan; n = capacity is halved; n = 1 again."""
    n = SHAPES[shape][3]
    assert cut(shape, 1) == 0 and cut(shape, n) > 0
    images, prev = scene(shape), guesses(shape)

    def script(b):
        steps = []
        for name, k in (("one pair", 1), ("the capacity", n), ("one pair again", 1)):
            r = track(b, images, k, prev[:k])
            steps.append((name, r, eval0(b, r)))
        return steps

    got = both_plans(monkeypatch, shape, arith, 0.0, script)
    for knob in ("0", "1"):
        assert_same(got[knob][2][1], got[knob][0][1], f"plan {knob}: one pair again")
        assert_same(got[knob][0][1], {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in got[knob][1][1].items()}, f"plan {knob}: pair 0 alone and in the batch",
                    only=("poses", "status"))


# ---------------------------------------------------------------------------------------------- 5. unaligned caller buffers
def unaligned(images, n):
    """The three level-0 inputs 5 bytes (2 uint16 elements) into their allocations, as test_gpu_pyramid.py places them."""
    import torch
    kg, kd, cg = (t[:n] for t in images[:3])
    raw_k = torch.zeros(kg.numel() + 5, dtype=torch.uint8, device="cuda")
    raw_c = torch.zeros(cg.numel() + 5, dtype=torch.uint8, device="cuda")
    raw_d = torch.zeros(kd.numel() + 2, dtype=torch.int16, device="cuda")
    out = (raw_k[5:].view(kg.shape), raw_d[2:].view(kd.shape), raw_c[5:].view(cg.shape))
    for dst, src in zip(out, (kg, kd, cg)):
        dst.copy_(src)
        assert dst.data_ptr() % 16 != 0
    return out


UNALIGNED = [(s, n, a) for s, n in (("60x80", 8), ("60x80", 7), ("61x83", 40), ("61x83", 23)) for a in ("fused", "reference")]


@pytest.mark.parametrize("shape,n,arith", UNALIGNED, ids=[f"{s}_n{n}_{a}" for s, n, a in UNALIGNED])
def test_caller_buffers_that_are_not_16_byte_aligned(monkeypatch, shape, n, arith):
    """plan_halves' `align` keeps the alignment a call HAS; a call that has none takes the narrow forms of the pyramid and keyframe
    kernels in both slices: the plain call's bits, which are the aligned run's. At 60x80 the aligned run takes the dense quad source
    (four pixels per unit) in the LM stage; an unaligned run must take it too, since another source sums in another order: launch_geom
    (lm_sources.h) decides from the handle's own planes and DenseQuadSrc::load reads the caller's planes with loads of any address.
    61x83 never takes the quad source."""
    L = SHAPES[shape][2]
    images, prev = scene(shape), guesses(shape)[:n]
    moved = unaligned(images, n)
    b_off, b_on = handle(monkeypatch, "0", shape, arith), handle(monkeypatch, "1", shape, arith)
    aligned = track(b_off, images, n, prev)
    off, on = track(b_off, moved, n, prev), track(b_on, moved, n, prev)
    ok = aligned["status"] == 0
    print(f"[unaligned {shape} n={n} {arith}] against the aligned run, plan off: poses of {int((off['poses'].view(np.uint32) != aligned['poses'].view(np.uint32)).any(axis=1).sum())}"
          f" of {n} pairs differ, max |pose difference| {np.abs(off['poses'] - aligned['poses']).max():.3e}, statuses equal {bool((off['status'] == aligned['status']).all())},"
          f" iteration counts equal {bool((off['stats']['nb_iter'] == aligned['stats']['nb_iter']).all())}, max relative energy difference"
          f" {np.abs(off['stats']['energy'][ok][:, :L] / aligned['stats']['energy'][ok][:, :L] - 1).max():.3e}")
    assert_same(on, off, f"{shape} n={n} {arith}, unaligned: plan on against plan off")
    assert_same(on, aligned, f"{shape} n={n} {arith}: unaligned, plan on, against aligned, plan off")
    assert_same(track(b_on, images, n, prev), aligned, f"{shape} n={n} {arith}: aligned again on the handle that ran unaligned")


# ---------------------------------------------------------------------------------------------- 6. other entries that reach the plan
@pytest.mark.parametrize("shape,arith", [(s, a) for s in ("60x80", "120x160") for a in ("fused", "reference")],
                         ids=[f"{s}_{a}" for s in ("60x80", "120x160") for a in ("fused", "reference")])
def test_multi_gpu_handle_with_the_plan(monkeypatch, shape, arith):
    """vors_multi_create builds its per-device handles with vors_batch_create_on: the plan is allowed. One device is asked for, so that its
    shard is the whole batch of 8 pairs and is halved whatever the number of visible devices. Both entries, knob at 1 against 0 and
    against a plain V.Batch of the same capacity, as test_gpu_multi.py compares."""
    n = 8
    rows, cols = SHAPES[shape][:2]
    images = scene(shape)
    kg, kd, cg = (a[:n] for a in host_scene(shape))
    plain = track(handle(monkeypatch, "0", shape, arith, cap=n), images, n, stats=False)
    got = {}
    for knob in ("0", "1"):
        knobs(monkeypatch, knob)
        m = V.MultiGpu(config(shape, arith), n, rows, cols, n_devices=1)
        assert m.device_count() == 1 and m.shard(n, 0) == (0, n)
        got[knob] = dict(host=m.track_pairs_host(kg, kd, cg), device=m.track_pairs([images[0][:n]], [images[1][:n]], [images[2][:n]], n))
    for knob in ("0", "1"):
        for entry, (poses, status) in got[knob].items():
            assert poses.tobytes() == plain["poses"].tobytes() and status.tobytes() == plain["status"].tobytes(), f"multi {entry}, VORS_BATCH_HALVES={knob}"


ONE_SHOT = [(s, n, a) for s, n in (("60x80", 8), ("60x80", 7), ("61x83", 23), ("120x160", 8)) for a in ("fused", "reference")]


@pytest.mark.parametrize("shape,n,arith", ONE_SHOT, ids=[f"{s}_n{n}_{a}" for s, n, a in ONE_SHOT])
def test_one_shot_host_entry_with_the_plan(monkeypatch, shape, n, arith):
    """vors_track_pairs creates its handle with vors_batch_create and runs the step on the NULL stream: the second slice's stream forks
    from and joins the legacy stream. V.track_pairs is the wrapper test_gpu_parity.py::test_optional_outputs_and_host_buffer_entry uses;
    row-major and column-major, with guesses and statistics, knob at 1 against 0 and against the device-resident call."""
    kg, kd, cg = (a[:n] for a in host_scene(shape))
    prev = guesses(shape)[:n]
    T = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1))
    want = track(handle(monkeypatch, "0", shape, arith, cap=n), scene(shape), n, prev)
    for knob in ("0", "1"):
        knobs(monkeypatch, knob)
        for layout, arrays in ((V.ROW_MAJOR, (kg, kd, cg)), (V.COL_MAJOR, (T(kg), T(kd), T(cg)))):
            poses, status, stats = V.track_pairs(config(shape, arith), *arrays, prev_poses7=prev, layout=layout)
            got = dict(poses=poses, status=status, stats=stats, pred_log=want["pred_log"])
            assert_same(got, want, f"one-shot entry, layout {layout}, VORS_BATCH_HALVES={knob}", levels=SHAPES[shape][2])
            poses2, status2, none = V.track_pairs(config(shape, arith), *arrays, prev_poses7=prev, layout=layout, want_stats=False)
            assert none is None and poses2.tobytes() == poses.tobytes() and status2.tobytes() == status.tobytes()


@pytest.mark.parametrize("shape,arith", [(s, a) for s in ("60x80", "61x83") for a in ("fused", "reference")],
                         ids=[f"{s}_{a}" for s in ("60x80", "61x83") for a in ("fused", "reference")])
def test_pipeline_slots_keep_the_plain_path(monkeypatch, shape, arith):
    """Ring slots are created with allow_halves = false. With the knob at 1, three steps of a ring of two equal the plain batch's steps
    (knob at 0) bit for bit. The wrapper exposes no workspace figure of a pipeline (nor does the C ABI), so the opt-out itself is asserted
    through the results only; should a later wrapper expose one, it must be the figure with the knob at 0."""
    rows, cols, _, cap = SHAPES[shape]
    steps = [(scene(shape), cap, guesses(shape)), (scene(shape, seed_off=500), cap - 1, None), (scene(shape, motion=0.5), cap, None)]
    b = handle(monkeypatch, "0", shape, arith)
    want = [track(b, images, n, prev) for images, n, prev in steps]
    figures = {}
    for knob in ("0", "1"):
        knobs(monkeypatch, knob)
        pipe = V.Pipeline(config(shape, arith), cap, rows, cols, depth=2)
        bufs = []
        for images, n, prev in steps:
            bufs.append(out_buffers(n))
            pipe.submit(images[0][:n], images[1][:n], images[2][:n], *bufs[-1], prev_poses7=to_device(prev, n))
        pipe.drain()
        for k, (images, n, prev) in enumerate(steps):
            got = collect(None, n, bufs[k], f"pipeline step {k}")
            got["pred_log"] = want[k]["pred_log"]   # (a pipeline exposes no prediction log)
            assert_same(got, want[k], f"pipeline step {k}, VORS_BATCH_HALVES={knob}")
        if hasattr(pipe, "workspace_bytes"):
            figures[knob] = pipe.workspace_bytes()
    assert figures.get("0") == figures.get("1")


# ---------------------------------------------------------------------------------------------- 7. workspace accounting
@pytest.mark.parametrize("shape,arith", [(s, a) for s in SHAPES for a in ("fused", "reference")], ids=[f"{s}_{a}" for s in SHAPES for a in ("fused", "reference")])
def test_workspace_bytes_counts_the_second_slice(monkeypatch, shape, arith):
    """The plan's workspace (the second slice's LM workspace, REFERENCE: its hand-over counters) is allocated when the handle is created,
    counted by vors_batch_workspace_bytes, the same for every handle of a kind, and no halved call allocates."""
    n = SHAPES[shape][3]
    off, on, on2 = handle(monkeypatch, "0", shape, arith), handle(monkeypatch, "1", shape, arith), handle(monkeypatch, "1", shape, arith)
    assert on.workspace_bytes() > off.workspace_bytes()
    assert on.workspace_bytes() == on2.workspace_bytes()
    before, before_off = on.workspace_bytes(), off.workspace_bytes()
    for k in (n, max(2, n - 1), 1):
        track(on, scene(shape), k, guesses(shape)[:k])
        track(off, scene(shape), k, guesses(shape)[:k])
    assert on.workspace_bytes() == before and off.workspace_bytes() == before_off


# ---------------------------------------------------------------------------------------------- 8. the default threshold, no knob
def test_default_threshold_without_a_knob(monkeypatch):
    """A 4096-pair handle with VORS_BATCH_HALVES unset has the plan (its workspace figure exceeds the plan-off handle's): a call of 4096
    pairs is halved at 2048, a call of 4095 is below the threshold and takes the plain path. The 8-pair scene is tiled, every replica with
    its pair's guess: pairs on both sides of the cut carry the same bits in both calls, and all replicas of a pair are alike."""
    import torch
    shape, cap = "60x80", 4096
    rows, cols = SHAPES[shape][:2]
    assert cut(shape, cap) == 2048
    LB.set_knobs(monkeypatch, LB.dense_env(cap))
    monkeypatch.setenv("VORS_BATCH_HALVES", "0")
    plain_bytes = V.Batch(config(shape, "fused"), cap, rows, cols).workspace_bytes()
    monkeypatch.delenv("VORS_BATCH_HALVES")
    b = V.Batch(config(shape, "fused"), cap, rows, cols)
    assert b.workspace_bytes() > plain_bytes, "the handle has no plan"
    idx = np.arange(cap) % 8
    t_idx = torch.from_numpy(idx).cuda()
    images = tuple(t.index_select(0, t_idx).contiguous() for t in scene(shape)[:3])
    prev = guesses(shape)[idx]
    full, less = track(b, images, cap, prev), track(b, images, cap - 1, prev)
    a, c = fields(full), fields(less)
    for f in a:
        for k in (0, 2047, 2048, 4094):
            assert a[f][k].tobytes() == c[f][k].tobytes(), f"{f} of pair {k}: the call of 4096 pairs against the call of 4095"
        assert a[f].tobytes() == np.ascontiguousarray(a[f][idx]).tobytes(), f"{f}: replicas of a pair differ within the call of 4096 pairs"
    assert (full["status"] == 0).any()
