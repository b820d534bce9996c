"""One dense vors_batch_track_pairs call as two overlapped slices (batch.cpp plan_halves / track_pairs_halves) computes the plain call's bits.

The plan is decided when a handle is created (VORS_BATCH_HALVES: 0 = off, 1 = from 2 pairs on), so the two sides of every comparison come
from two child processes, one per value, started ONCE per module: each runs the same list of cases on the same seeded pairs and writes
every output array (poses, status, every vors_pair_stats field, the prediction log) to one .npz; the tests compare them bit for bit.
VORS_LM_SPLIT_LEVELS=2 in both makes the small images take the two-level evaluation rounds of 640x480, and the side lane from 2048 pairs.

What needs no second process is computed inside each child and reported as flags: a captured step replayed three times against the
eager one (asserted for the plan-on child), two handles on two caller streams against serial runs, and the stage times.

The hostile batch needs the oracle and no comparison across processes: test_gpu_large_batches' tiled outcome batch (2048 pairs, replicas of
56 pairs that hold Cholesky failures, pairs at the iteration limit and rejected candidates) runs in this process with the plan forced on,
every failure kind on both sides of the cut, against the plan-off run bit for bit and against the oracle as the failure-path tests do.
GPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# 61x83: rows * cols is odd, so the cut is rounded to 16 pairs (batch.cpp plan_halves `align`); the other two keep any cut
SHAPES = {"120x160": (120, 160, 4), "60x80": (60, 80, 3), "61x83": (61, 83, 3)}
SEED = 0x5EED4A00
STAT_FIELDS = ("lm_model", "optical_flow", "change_keyframe", "nb_iter", "n_points", "energy", "nb_grad_evals")


def case_list():
    """(key, shape, arithmetic name, huber, candidates, capacity, n_pairs of each consecutive call)"""
    cases = []
    for shape in ("120x160", "60x80"):
        for arith in ("fused", "reference"):
            for huber in (0.0, 10.0):
                # 2, 3, an odd count, the capacity; 1 is below the forced threshold of 2: the plain path on a handle that has the plan
                for n in (2, 3, 7, 8, 1):
                    cases.append((f"{shape}_{arith}_h{huber:g}_cap8_n{n}", shape, arith, huber, "dense", 8, (n,)))
    cases.append(("120x160_exact_h0_cap8_n5", "120x160", "exact", 0.0, "dense", 8, (5,)))
    cases.append(("120x160_fused_h0_cap2048_n2048", "120x160", "fused", 0.0, "dense", 2048, (2048,)))   # side lane in both slices
    cases.append(("120x160_fused_h0_cap2048_n2047", "120x160", "fused", 0.0, "dense", 2048, (2047,)))
    cases.append(("60x80_reference_h0_cap2048_n2048", "60x80", "reference", 0.0, "dense", 2048, (2048,)))
    cases.append(("120x160_fused_h0_cap8_twice", "120x160", "fused", 0.0, "dense", 8, (8, 5)))           # two consecutive calls on one handle
    cases.append(("120x160_fused_h0_c2f_cap8_n8", "120x160", "fused", 0.0, "c2f", 8, (8,)))             # not dense: the plan is not taken
    for arith in ("fused", "reference"):
        cases.append((f"61x83_{arith}_h0_cap40_n40", "61x83", arith, 0.0, "dense", 40, (40,)))   # cut rounded from 20 up to 32: slices of 32 and 8
        cases.append((f"61x83_{arith}_h0_cap40_n23", "61x83", arith, 0.0, "dense", 40, (23,)))   # cut 16: slices of 16 and 7
        cases.append((f"61x83_{arith}_h0_cap40_n16", "61x83", arith, 0.0, "dense", 40, (16,)))   # the rounded cut reaches n_pairs: the plain path
    return cases


# ------------------------------------------------------------------------------------------------------------ the child process
def child(out_path):
    import torch
    import vors_amd as V
    plan_on = os.environ.get("VORS_BATCH_HALVES") == "1"
    ariths = {"fused": V.ARITH_FUSED, "exact": V.ARITH_EXACT, "reference": V.ARITH_REFERENCE}
    out = {}
    scenes = {}

    def scene(shape, n):
        rows, cols, _ = SHAPES[shape]
        if (shape, n) not in scenes:
            scenes[(shape, n)] = V.synth_render_pairs(SEED, n, rows, cols, V.scaled_intrinsics(rows, cols))[:3]
        return scenes[(shape, n)]

    def config(shape, arith, huber, cand):
        rows, cols, L = SHAPES[shape]
        intr = V.scaled_intrinsics(rows, cols)
        return V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), huber_delta=huber, arithmetic=ariths[arith],
                        candidates_mode=V.CANDIDATES_DENSE if cand == "dense" else V.CANDIDATES_COARSE_TO_FINE)

    def run(batch, kg, kd, cg, n):
        poses = torch.full((n, 7), 7.0, dtype=torch.float32, device="cuda")
        status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        stats = V.stats_tensor(n, device="cuda")
        batch.track_pairs(kg[:n], kd[:n], cg[:n], poses, status, stats)
        torch.cuda.synchronize()
        return poses, status, stats

    def record(key, batch, poses, status, stats, n):
        out[key + "/poses"] = poses.cpu().numpy()
        out[key + "/status"] = status.cpu().numpy()
        st = V.decode_stats(stats)
        for f in STAT_FIELDS:
            out[key + "/" + f] = np.ascontiguousarray(st[f])
        out[key + "/pred_log"] = batch.lm_predict_log(n)

    for key, shape, arith, huber, cand, cap, counts in case_list():
        rows, cols, _ = SHAPES[shape]
        kg, kd, cg = scene(shape, cap)
        batch = V.Batch(config(shape, arith, huber, cand), cap, rows, cols)
        for n in counts:
            res = run(batch, kg, kd, cg, n)
        record(key, batch, *res, counts[-1])
        del batch

    # ---- with the plan on: capture, concurrency, stage times (flags; with the plan off the same code runs the plain path)
    rows, cols, _ = SHAPES["120x160"]
    kg, kd, cg = scene("120x160", 8)
    cfg = config("120x160", "fused", 0.0, "dense")
    batch = V.Batch(cfg, 8, rows, cols)
    eager = run(batch, kg, kd, cg, 8)
    poses = torch.zeros((8, 7), dtype=torch.float32, device="cuda")
    status = torch.zeros(8, dtype=torch.int32, device="cuda")
    stats = V.stats_tensor(8, device="cuda")
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            batch.track_pairs(kg, kd, cg, poses, status, stats)
    same = True
    for _ in range(3):
        poses.fill_(3.0)
        status.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        differ = [name for name, a, b in (("poses", poses, eager[0]), ("status", status, eager[1])) if not torch.equal(a.view(torch.uint8), b.view(torch.uint8))]
        st_a, st_b = V.decode_stats(stats), V.decode_stats(eager[2])
        differ += [f for f in STAT_FIELDS if st_a[f].tobytes() != st_b[f].tobytes()]
        same = same and not differ
    out["flags/graph_replays_equal_eager"] = np.array(same)
    out["flags/graph_differing_fields"] = np.array(",".join(differ))
    out["flags/graph_n_points_replay"], out["flags/graph_n_points_eager"] = st_a["n_points"].copy(), st_b["n_points"].copy()
    del g

    # two handles on two caller streams at once against the serial runs
    kg2, kd2, cg2 = V.synth_render_pairs(SEED + 1000, 8, rows, cols, V.scaled_intrinsics(rows, cols))[:3]
    b1, b2 = V.Batch(cfg, 8, rows, cols), V.Batch(cfg, 8, rows, cols)
    serial1, serial2 = run(b1, kg, kd, cg, 8), run(b2, kg2, kd2, cg2, 7)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [(torch.zeros((8, 7), device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"), V.stats_tensor(8, device="cuda")),
            (torch.zeros((7, 7), device="cuda"), torch.zeros(7, dtype=torch.int32, device="cuda"), V.stats_tensor(7, device="cuda"))]
    torch.cuda.synchronize()
    for _ in range(2):
        with torch.cuda.stream(s1):
            b1.track_pairs(kg, kd, cg, *outs[0])
        with torch.cuda.stream(s2):
            b2.track_pairs(kg2[:7], kd2[:7], cg2[:7], *outs[1])
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for got, want in zip(outs, (serial1, serial2)) for a, b in zip(got, want))
    out["flags/two_streams_equal_serial"] = np.array(same)

    # stage times of three 2048-pair steps, each between two events of the caller's stream (the step's own device time)
    del batch, b1, b2
    kg, kd, cg = scene("120x160", 2048)
    batch = V.Batch(cfg, 2048, rows, cols)
    run(batch, kg, kd, cg, 2048)
    batch.enable_kernel_timing(4)
    poses, status = torch.zeros((2048, 7), device="cuda"), torch.zeros(2048, dtype=torch.int32, device="cuda")
    step_ms = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        batch.track_pairs(kg, kd, cg, poses, status)
        e1.record()
        torch.cuda.synchronize()
        step_ms.append(e0.elapsed_time(e1))
    times = np.stack([batch.kernel_times(s) for s in ("pyramid_keyframe", "keyframe", "pyramid_current", "lm")])
    out["flags/kernel_times"] = times
    out["flags/step_ms"] = np.array(step_ms, np.float32)
    out["flags/last_kernel_ms"] = np.array(list(batch.last_kernel_ms().values()), np.float32)
    out["flags/plan_on"] = np.array(plan_on)
    np.savez(out_path, **out)


# ------------------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_halves")
    res = {}
    for knob in ("0", "1"):
        path = str(d / f"halves{knob}.npz")
        env = dict(os.environ, VORS_BATCH_HALVES=knob, VORS_LM_SPLIT_LEVELS="2")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, f"child with VORS_BATCH_HALVES={knob} failed:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
        res[knob] = dict(np.load(path))
    return res


def test_children_ran_what_they_should(runs):
    assert not bool(runs["0"]["flags/plan_on"]) and bool(runs["1"]["flags/plan_on"])
    assert set(runs["0"]) == set(runs["1"])


@pytest.mark.parametrize("case", [c[0] for c in case_list()])
def test_plan_on_equals_plan_off_bit_for_bit(runs, case):
    off, on = runs["0"], runs["1"]
    for f in ("poses", "status", "pred_log") + STAT_FIELDS:
        a, b = off[f"{case}/{f}"], on[f"{case}/{f}"]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{case}: {f} differs between VORS_BATCH_HALVES=0 and =1"
    assert (off[f"{case}/status"] >= 0).all(), "the outputs were written"


def test_prediction_log_is_used_and_equal(runs):
    key = "120x160_fused_h0_cap2048_n2048/pred_log"
    assert runs["1"][key].any(), "the batch exercises the go-on prediction"
    assert np.array_equal(runs["0"][key], runs["1"][key])


def test_graph_capture_with_the_plan_on(runs):
    assert bool(runs["1"]["flags/graph_replays_equal_eager"]), f"three replays of a captured step equal the eager step; differing: {runs['1']['flags/graph_differing_fields']}"


@pytest.mark.parametrize("knob", ["0", "1"])
def test_two_handles_on_two_streams(runs, knob):
    assert bool(runs[knob]["flags/two_streams_equal_serial"]), "two handles on two caller streams equal their serial runs"


@pytest.mark.parametrize("knob", ["0", "1"])
def test_stage_times(runs, knob):
    t = runs[knob]["flags/kernel_times"]
    assert t.shape == (4, 3) and np.isfinite(t).all() and (t >= 0).all(), t
    assert (t[3] > 0).all(), "the LM stage took time"
    last = runs[knob]["flags/last_kernel_ms"]
    assert np.isfinite(last).all() and (last >= 0).all()
    # The documented meaning, as inequalities that hold by construction on either path (2 % and 20 us for the events' own resolution). The
    # LM stage lies inside the step. Plain path: the four stages follow one another on the caller's stream and make up the step. Two
    # halves: the step ends with the last LM end of either slice (the join) and the first LM start comes no later than the end of the
    # first slice's own pre-LM intervals, which the three pre-LM figures contain as summands — so `lm` as the SPAN of both slices plus
    # the pre-LM SUMS covers the step; an `lm` that left a slice out, or pre-LM figures without one slice's share, would fall short.
    step = runs[knob]["flags/step_ms"]
    print(f"[stage times, VORS_BATCH_HALVES={knob}] step {step}, stages {t.tolist()}")
    assert (t[3] <= step * 1.02 + 0.02).all(), (t[3], step)
    assert (t.sum(axis=0) >= step * 0.98 - 0.02).all(), (t.sum(axis=0), step)
    if knob == "0":
        assert (t.sum(axis=0) <= step * 1.02 + 0.02).all(), "plain path: the stages add up to the step"


# ------------------------------------------------------------------------------------------------------------ the hostile batch
@pytest.mark.parametrize("arith", ["fused", "reference"])
def test_tiled_hostile_batch_with_every_failure_kind_in_each_slice(monkeypatch, arith):
    import adversarial as A
    import test_gpu_adversarial as TA
    import test_gpu_large_batches as LB
    import vors_amd as V
    n, h = LB.HOSTILE_N, LB.HOSTILE_N // 2   # 96x128: rows * cols is a multiple of 16, the cut is half the pairs
    n_unique = len(TA.outcome_scene(1)[0])
    ref, cls = LB.hostile_oracle(1)
    LB.assert_hostile_targets(cls)
    for name, kind in (("Cholesky failures / outcome 1", cls["o1"]), ("outcome 2", cls["o2"]), ("outcome 3", cls["o3"]),
                       ("failures at level 1", cls["fail_level"] == 1), ("failures at level 0", cls["fail_level"] == 0),
                       ("pairs at the iteration limit", (ref["nb_iter"] >= ref["nb_iter"].max()).any(axis=1))):
        assert kind[:h].any() and kind[h:].any(), f"{name}: not in both slices"
    images = LB.on_device("hostile", 1)
    arith_id = V.ARITH_FUSED if arith == "fused" else V.ARITH_REFERENCE

    def run(knob):
        LB.set_knobs(monkeypatch, dict(LB.dense_env(n) if arith == "fused" else {}, VORS_BATCH_HALVES=knob))
        return LB.track(V.Batch(LB.vcfg(1, arith_id, levels=LB.HL, intr=TA.INTR), n, TA.ROWS, TA.COLS), images, levels=LB.HL)

    on, off = run("1"), run("0")
    LB.assert_same_bits(on, off, f"hostile dense {arith}: plan on against plan off")
    assert not np.isnan(on["poses"]).any()
    assert (on["poses"][on["status"] != 0] == A.identity7()).all(), "a failed pair did not keep its (identity) pose"
    LB.assert_replicas_identical(on, n_unique, f"hostile dense {arith}, plan on")
    if arith == "reference":   # the oracle's bits, as test_reference_default_hand_over_on_the_tiled_hostile_batch asks
        assert (on["poses"].view(np.uint32) == ref["poses"].view(np.uint32)).all() and (on["status"] == ref["status"]).all()
        assert (on["nb_iter"] == ref["nb_iter"]).all()
        return
    # FUSED: the counting gate of test_dense_tiled_hostile_batch_through_the_side_lane on the distinct pairs
    ref64, _ = LB.hostile_oracle(1, variant="acc64")

    def n_off(p, s):
        return int(((s != ref["status"]) | (np.abs(p - ref["poses"]).max(axis=1) > LB.POSE_TOL))[:n_unique].sum())

    floor = n_off(ref64["poses"], ref64["status"])
    assert n_off(on["poses"], on["status"]) <= floor + 2 + 2 * np.sqrt(floor)
    structural = cls["o1"] & ~cls["o2"]
    assert (on["status"][structural] == ref["status"][structural]).all()
    assert (on["status"][cls["o3"]] == ref["status"][cls["o3"]]).all(), "outcome 3: statuses differ from the oracle's"


if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "visual-odometry-rs_amd"))
    assert sys.argv[1] == "--child"
    child(sys.argv[2])
