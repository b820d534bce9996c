"""Dense FUSED evaluation rounds with the go-on prediction (batch.cpp plan_split `predict`, lm_kernels.hip lm_split_step_kernel) against the
plain schedule (VORS_LM_PREDICT=0): the prediction chooses which kernel produces a candidate's energy and in which round its g and H are
formed, never a number — poses, statuses and every statistic are the same bits, with and without Huber weights, below the side-lane
limit and above it, on the plain batch of tests/test_gpu_large_batches.py and on its tiled hostile batch (pairs whose Cholesky fails at a
level solved by rounds, pairs that run into the iteration limit, rejected candidates). The knob is read when the handle is created, so
both schedules run in one process. Each test asserts from the oracle that its batch holds what it targets.

The prediction leaves no trace in any result, so what it did with each pair comes from the handle's own log (vors_batch_lm_predict_log):
the tests assert from it that candidates were predicted on the device, and were predicted wrongly in both directions — on pairs the CPU
oracle names (tests/golden/lm_predict/plain_160x120_L4.csv, written by tools/lm_predict_probe.cpp: the promise and the verdict of every
candidate of the plain batch's first 512 pairs), and, with the threshold VORS_LM_PREDICT_TAU moved out of the way in either direction, on
every candidate of the hostile batch. GPU only."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V

import test_gpu_adversarial as TA
import test_gpu_large_batches as LB

FIELDS = LB.FIELDS + ("nb_grad_evals", "n_points")


def track(b, images, levels):
    import torch
    n = images[0].shape[0]
    poses = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    status = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    stats = V.stats_tensor(n)
    b.track_pairs(*images, poses, status, stats)
    torch.cuda.synchronize()
    st = V.decode_stats(stats)
    return dict(log=b.lm_predict_log(n), poses=poses.cpu().numpy(), status=status.cpu().numpy(), lm_model=st["lm_model"].copy(), nb_iter=st["nb_iter"][:, :levels].copy(),
                energy=st["energy"][:, :levels].copy(), optical_flow=st["optical_flow"].copy(), nb_grad_evals=st["nb_grad_evals"][:, :levels].copy(),
                n_points=st["n_points"][:, :levels].copy())


def both_schedules(monkeypatch, cfg, cap, rows, cols, images, levels, **more):
    """-> (prediction on, VORS_LM_PREDICT=0): two handles of the same shape on the same device tensors."""
    out = []
    for knob in ({}, {"VORS_LM_PREDICT": "0"}):
        env = {"VORS_LM_SPLIT_LEVELS": "2"}
        env.update(more)
        env.update(knob)
        LB.set_knobs(monkeypatch, env, knobs=LB.LM_KNOBS + LB.REF_KNOBS + ("VORS_LM_PREDICT", "VORS_LM_PREDICT_TAU"))
        out.append(track(V.Batch(cfg, cap, rows, cols), images, levels))
    assert not out[1]["log"].any(), "VORS_LM_PREDICT=0 still predicts"
    return out


FULL, FULL_GO_ON, FULL_STOP, FULL_REJECTED, MISSED = 1, 2, 4, 8, 16  # include/vors_hip.h VORS_PREDICT_*


def count(log, bit):
    return int(((log & bit) != 0).sum())


def assert_same_bits(got, want, what):
    for f in FIELDS:
        diff = LB.raw(got[f]) != LB.raw(want[f])
        bad = np.flatnonzero(diff.reshape(len(diff), -1).any(axis=1))
        assert len(bad) == 0, f"{what}: {f} differs in {len(bad)} of {len(diff)} pairs, first {bad[:8]}"


@pytest.mark.parametrize("cap", [512, 2048], ids=["cap512-no-side-lane", "cap2048-side-lane"])
@pytest.mark.parametrize("huber", [0.0, 10.0], ids=["plain", "huber10"])
def test_prediction_leaves_every_bit_of_the_plain_batch(monkeypatch, huber, cap):
    """The plain pairs: at level 0 some go on after their first candidate (the ones the prediction is for) and most stop."""
    what = f"dense fused huber {huber} capacity {cap}"
    ref = LB.plain_oracle(1, cap, huber)
    ok = ref["status"] == 0
    go_on, stop = int((ok & (ref["nb_iter"][:, 0] >= 2)).sum()), int((ok & (ref["nb_iter"][:, 0] == 1)).sum())
    print(f"[{what}] level 0 goes on after the first candidate: {go_on} pairs; stops there: {stop}")
    assert go_on >= LB.MIN_GROUP and stop >= LB.MIN_GROUP
    on, off = both_schedules(monkeypatch, LB.vcfg(1, V.ARITH_FUSED, huber), cap, LB.ROWS, LB.COLS, LB.prefix(LB.on_device("plain", False), cap), LB.L)
    assert_same_bits(on, off, what)
    print(f"[{what}] device log: predicted {count(on['log'], FULL)} pairs, of them went on {count(on['log'], FULL_GO_ON)}, stopped "
          f"{count(on['log'], FULL_STOP)}, rejected {count(on['log'], FULL_REJECTED)}; missed go-ons {count(on['log'], MISSED)}")
    assert count(on["log"], FULL_GO_ON) >= LB.MIN_GROUP, f"{what}: the prediction did not fire on the device"
    assert (on["status"] == ref["status"]).all()
    err = np.abs(on["poses"] - ref["poses"]).max(axis=1)
    ref64 = LB.plain_oracle(1, cap, huber, variant="acc64")
    floor = int((np.abs(ref64["poses"] - ref["poses"]).max(axis=1) > LB.POSE_TOL).sum())
    assert int((err > LB.POSE_TOL).sum()) <= floor + 2 + 2 * np.sqrt(floor), f"{what}: {int((err > LB.POSE_TOL).sum())} pairs beyond 1e-4, floor {floor}"


@pytest.mark.parametrize("cap", [512, LB.HOSTILE_N], ids=["cap512-no-side-lane", "cap2048-side-lane"])
@pytest.mark.parametrize("rounds", [None, "5"], ids=["default-rounds", "5-rounds"])
def test_prediction_leaves_every_bit_of_the_hostile_batch(monkeypatch, cap, rounds):
    """The tiled outcome batch: pairs whose Cholesky fails at level 1 and at level 0, pairs that use all 21 iterations of level 0, pairs
    with rejected candidates there (more iterations than accepted candidates). Five rounds leave pairs to the stragglers' kernel in the
    middle of level 0."""
    what = f"hostile dense fused capacity {cap} rounds {rounds}"
    ref, cls = LB.hostile_oracle(1)
    ref = {k: v[:cap] for k, v in ref.items()}
    cls = {k: v[:cap] for k, v in cls.items()}
    ok = ref["status"] == 0
    n_fail0, n_fail1 = int((cls["fail_level"] == 0).sum()), int((cls["fail_level"] == 1).sum())
    n_limit = int((ok & (ref["nb_iter"][:, 0] == 21)).sum())
    n_long = int((ok & (ref["nb_iter"][:, 0] >= 4)).sum())
    print(f"[{what}] Cholesky fails at level 0: {n_fail0} pairs, at level 1: {n_fail1}; 21 iterations at level 0: {n_limit}; 4 or more: {n_long}")
    assert n_fail0 >= 1 and n_fail1 >= 1 and n_limit >= 1 and n_long >= 1
    images = LB.prefix(LB.on_device("hostile", 1), cap)
    more = {} if rounds is None else {"VORS_LM_SPLIT_ROUNDS": rounds}
    on, off = both_schedules(monkeypatch, LB.vcfg(1, V.ARITH_FUSED, levels=LB.HL, intr=TA.INTR), cap, TA.ROWS, TA.COLS, images, LB.HL, **more)
    assert_same_bits(on, off, what)
    rejected = int(((on["nb_iter"][:, 0] + 1 > on["nb_grad_evals"][:, 0]) & (on["status"] == 0)).sum())
    print(f"[{what}] pairs with a rejected candidate at level 0 (device statistics): {rejected}")
    assert rejected >= 1


# ---------------------------------------------------------------------------------------------- wrong in both directions
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm_predict", "plain_160x120_L4.csv")
MARGIN = 0.03  # clear of the threshold and of stop_criterion's 1.0 by this much, in the oracle's own arithmetic (FUSED moves an energy by ~1e-3)
NAMED_FALSE_POSITIVES, NAMED_FALSE_NEGATIVES = (100, 314, 463), (128, 356, 404)


def oracle_first_candidates():
    """-> pair, promise, verdict, energy decrease of the FIRST level-0 candidate of each pair, from the oracle (the fixture)."""
    d = np.genfromtxt(FIXTURE, delimiter=",", names=True)
    d = d[(d["level"] == 0) & (d["nb_iter"] == 1)]
    return d["pair"].astype(int), d["predicted_decrease"], d["verdict"].astype(int), d["cur_energy"] - d["cand_energy"]


def test_named_pairs_are_predicted_wrongly_in_both_directions_and_keep_their_bits(monkeypatch):
    """Level 0 alone by rounds, so that every pair's first level-0 candidate comes from the step of round 0, where candidates may be
    predicted. From the oracle: a false positive promises more than 1 + MARGIN and is accepted with the level ending (decrease below
    1 - MARGIN); a false negative promises less than 1 - MARGIN and goes on with a decrease above 1 + MARGIN. The device's log must say
    the same of each of them, of the clear true positives and of the clear true negatives — and every bit equals VORS_LM_PREDICT=0."""
    cap = 512
    pair, promise, verdict, decrease = oracle_first_candidates()
    assert len(pair) == cap and (pair == np.arange(cap)).all()
    fp = (promise > 1 + MARGIN) & (verdict == 3) & (decrease < 1 - MARGIN)
    fn = (promise < 1 - MARGIN) & (verdict == 2) & (decrease > 1 + MARGIN)
    tp = (promise > 1 + 3 * MARGIN) & (verdict == 2) & (decrease > 1 + 3 * MARGIN)
    tn = (promise < 1 - 3 * MARGIN) & (verdict == 3) & (decrease < 1 - 3 * MARGIN)
    print(f"[oracle] false positives {pair[fp]}, false negatives {pair[fn]}, clear true positives {tp.sum()}, clear true negatives {tn.sum()}")
    assert set(NAMED_FALSE_POSITIVES) <= set(pair[fp]) and set(NAMED_FALSE_NEGATIVES) <= set(pair[fn])
    assert tp.sum() >= LB.MIN_GROUP and tn.sum() >= LB.MIN_GROUP
    on, off = both_schedules(monkeypatch, LB.vcfg(1, V.ARITH_FUSED), cap, LB.ROWS, LB.COLS, LB.prefix(LB.on_device("plain", False), cap), LB.L,
                             VORS_LM_SPLIT_LEVELS="1")
    assert_same_bits(on, off, "named pairs")
    log = on["log"]
    print(f"[device] log of the false positives {log[fp]}, of the false negatives {log[fn]}")
    assert (log[fp] == (FULL | FULL_STOP)).all(), "a false positive: predicted, evaluated in full, and the level ended there"
    assert ((log[fn] & MISSED) != 0).all(), "a false negative: not predicted, and the level went on"
    assert ((log[tp] & (FULL | FULL_GO_ON)) == (FULL | FULL_GO_ON)).all() and ((log[tp] & MISSED) == 0).all()
    assert (log[tn] == 0).all()


@pytest.mark.parametrize("cap", [512, LB.HOSTILE_N], ids=["cap512", "cap2048"])
@pytest.mark.parametrize("tau", ["-1e30", "1e30"], ids=["predict-everything", "predict-nothing"])
def test_threshold_out_of_the_way_on_the_hostile_batch(monkeypatch, tau, cap):
    """Every level-0 candidate that may be predicted IS (threshold far below): the full evaluation of candidates that are rejected, of
    candidates that end the level, and of steps after which the Cholesky factorisation fails — or NONE is (far above): every go-on is a
    missed one. The log shows each case on the device; the bits are those of VORS_LM_PREDICT=0. Level 0 alone by rounds: the hostile pairs
    spend so many rounds at level 1 that with two levels by rounds none of their level-0 candidates comes early enough to be predicted
    (the log of test_prediction_leaves_every_bit_of_the_hostile_batch is empty)."""
    what = f"hostile dense fused capacity {cap} tau {tau}"
    ref, cls = LB.hostile_oracle(1)
    assert int((cls["fail_level"][:cap] == 0).sum()) >= 1 and int(((ref["status"][:cap] == 0) & (ref["nb_iter"][:cap, 0] >= 4)).sum()) >= 1
    images = LB.prefix(LB.on_device("hostile", 1), cap)
    on, off = both_schedules(monkeypatch, LB.vcfg(1, V.ARITH_FUSED, levels=LB.HL, intr=TA.INTR), cap, TA.ROWS, TA.COLS, images, LB.HL,
                             VORS_LM_PREDICT_TAU=tau, VORS_LM_SPLIT_LEVELS="1")
    assert_same_bits(on, off, what)
    log = on["log"]
    print(f"[{what}] device log: predicted {count(log, FULL)} pairs: went on {count(log, FULL_GO_ON)}, stopped {count(log, FULL_STOP)}, rejected "
          f"{count(log, FULL_REJECTED)}; missed go-ons {count(log, MISSED)}")
    if tau == "-1e30":
        assert count(log, FULL_REJECTED) >= 1 and count(log, FULL_STOP) >= 1 and count(log, FULL_GO_ON) >= 1 and count(log, MISSED) == 0
    else:
        assert count(log, FULL) == 0 and count(log, MISSED) >= 1
