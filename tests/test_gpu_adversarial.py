"""Hostile scenes and the LM loop's rarer outcomes (tests/adversarial.py) against the oracle, in every form the device runs them.

The plain synthetic scene only ever converges, or fails at the first step of the coarsest level. Here the batches also hold pairs that
fail at a finer level after the coarser levels moved the model (outcome 1), that fail after accepted steps of the failing level
(outcome 2), and that accept an evaluation with no point inside (energy NaN, outcome 3); each test asserts, from the oracle's own
replay (adversarial.classify), that its batch really contains what it targets. All three are reached through whole pairs
(track_pairs), not at the operator level. REFERENCE must equal the oracle bit for bit — statuses, point and iteration counts, per-level
energies, final models, poses and optical flow — in every kernel form; EXACT and FUSED are gated like tests/test_gpu_fused.py. GPU only."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from oracle import oracle as O

import adversarial as A

ROWS, COLS, L, N = 96, 128, 3, 8
INTR = O.scaled_intrinsics(ROWS, COLS)
POSE_TOL = 1e-4
MODES = {0: "coarse_to_fine", 1: "dense", 2: "dso"}
SEED = {name: 0xADD0000 + 0x100 * k for k, name in enumerate(A.FAMILIES)}  # (pinned: the outcome counts below were searched on them)
SEED_SEQ = 0x5E90000
N_OUTCOME = 48  # rank-deficient pairs of the outcome batch (its seed holds all three outcomes in every mode, with and without Huber)


def vcfg(mode, huber=0.0, arith=V.ARITH_REFERENCE, L=L, intr=INTR, thresh=7):
    return V.Config(nb_levels=L, candidates_diff_threshold=thresh, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]),
                    candidates_mode=mode, huber_delta=huber, arithmetic=arith)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def seeded(family, mode):
    return SEED[family] | (A.BLOCKY if mode == 2 else 0)  # (the DSO selector needs the piecewise-constant texture)


@functools.lru_cache(maxsize=None)
def family_scene(family, mode):
    if family == "rank_deficient":
        return A.rank_deficient(seeded(family, mode), N, ROWS, COLS, INTR, mode=mode, L=L)
    return A.FAMILIES[family](seeded(family, mode), N, ROWS, COLS, INTR)


@functools.lru_cache(maxsize=None)
def outcome_scene(mode):
    """Outcome batch: 6 mid-pyramid pairs (outcome 1), N_OUTCOME rank-deficient pairs (outcomes 1, 2, 3) and 2 pairs without any usable
    depth (they fail at their first step: the first pairs to finish, so the hand-over forms queue the others early)."""
    parts = [A.mid_pyramid(seeded("mid_pyramid", mode), 6, ROWS, COLS, INTR),
             A.rank_deficient(seeded("rank_deficient", mode), N_OUTCOME, ROWS, COLS, INTR, mode=mode, L=L)]
    kg, kd, cg = (np.concatenate([p[k] for p in parts]) for k in range(3))
    kg, kd, cg = np.concatenate([kg, kg[:2]]), np.concatenate([kd, np.zeros_like(kd[:2])]), np.concatenate([cg, cg[:2]])
    return kg, kd, cg, None


def scene_of(family, mode):
    return outcome_scene(mode) if family == "outcomes" else family_scene(family, mode)


@functools.lru_cache(maxsize=None)
def oracle(family, mode, huber, variant=None):
    """-> (oracle.track_pairs, adversarial.classify) on scene_of(family, mode); variant: a sensitivity build, no replay."""
    kg, kd, cg, init = scene_of(family, mode)
    cfg = O.make_config(L, INTR, candidates_mode=mode, huber_delta=huber)
    ref = O.track_pairs(cfg, kg, kd, cg, init_poses7=init, n_threads=8, variant=variant)
    if variant:
        return ref, None
    cls = A.classify(cfg, kg, kd, cg, init)
    A.check_replay(ref, cls)
    return ref, cls


def run_batch(cfg, kg, kd, cg, prev=None):
    import torch
    n, rows, cols = kg.shape
    b = V.Batch(cfg, n, rows, cols)
    t = (torch.from_numpy(np.ascontiguousarray(kg)).cuda(), torch.from_numpy(np.ascontiguousarray(kd).view(np.int16)).cuda(),
         torch.from_numpy(np.ascontiguousarray(cg)).cuda())
    poses = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    stats = V.stats_tensor(n)
    if prev is not None:
        b.track_pairs(*t, poses, status, stats, prev_poses7=torch.from_numpy(np.ascontiguousarray(prev, np.float32)).cuda())
    else:
        b.track_pairs(*t, poses, status, stats)
    torch.cuda.synchronize()
    return poses.cpu().numpy(), status.cpu().numpy(), V.decode_stats(stats)


def prev_of(init, n):
    return np.tile(A.identity7(), (n, 1)) if init is None else init


def assert_identical(ref, cls, init, poses, status, st, what):
    n = len(status)
    assert (status == ref["status"]).all(), f"{what}: statuses differ in pairs {np.flatnonzero(status != ref['status'])[:8]}"
    assert (st["n_points"][:, :L] == ref["n_points"]).all(), what
    bad = np.flatnonzero((st["nb_iter"][:, :L] != ref["nb_iter"]).any(axis=1))
    assert len(bad) == 0, f"{what}: iteration counts differ in pairs {bad[:8]}"
    bad = np.flatnonzero(~np.array([A.same_energy(st["energy"][p, :L], cls["energy"][p]) for p in range(n)]))
    assert len(bad) == 0, f"{what}: per-level energies differ in pairs {bad[:8]}: {st['energy'][bad[:2], :L]} vs {cls['energy'][bad[:2]]}"
    bad = np.flatnonzero((bits(st["lm_model"]) != bits(ref["models"])).any(axis=1))
    assert len(bad) == 0, f"{what}: final models differ in pairs {bad[:8]} (outcomes 1/2/3 there: {cls['o1'][bad[:8]]} {cls['o2'][bad[:8]]} " \
                          f"{cls['o3'][bad[:8]]})"
    assert (bits(poses) == bits(ref["poses"])).all(), f"{what}: poses differ by {np.nanmax(np.abs(poses - ref['poses'])):.3e}"
    bad = np.flatnonzero(bits(st["optical_flow"]) != bits(ref["flow"]))
    assert len(bad) == 0, f"{what}: optical flow differs in pairs {bad[:8]}"
    assert (st["change_keyframe"] == (ref["flow"] >= 1.0)).all(), what
    failed = status != 0
    assert (bits(poses[failed]) == bits(prev_of(init, n)[failed])).all(), f"{what}: a failed pair did not keep its previous pose"


# ---------------------------------------------------------------------------------------------- REFERENCE, every family
@pytest.mark.parametrize("huber", [0.0, 10.0], ids=["l2", "huber10"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=list(MODES.values()))
@pytest.mark.parametrize("family", list(A.FAMILIES))
def test_reference_equals_the_oracle_on_every_family(family, mode, huber):
    kg, kd, cg, init = family_scene(family, mode)
    ref, cls = oracle(family, mode, huber)
    if family == "mid_pyramid":
        assert cls["o1"].all(), "every mid-pyramid pair was meant to fail at level 0 after the coarser levels converged"
    poses, status, st = run_batch(vcfg(mode, huber), kg, kd, cg, prev=init)
    assert_identical(ref, cls, init, poses, status, st, f"{family}, {MODES[mode]}, huber {huber}")


@pytest.mark.parametrize("thresh", [0, 7, 65535])
def test_full_size_saturated_checkerboards_equal_the_oracle(thresh):
    """640 x 480 x 6 levels: the keyframe kernel's u16 gradient norm wraps (gradient.rs:38-44) and so does `third + thresh`
    (coarse_to_fine.rs:85) at thresh 65535."""
    rows, cols, L6, n = 480, 640, 6, 3
    intr = O.scaled_intrinsics(rows, cols)
    kg, kd, cg, _ = A.saturated(0xADDF000 + thresh, n, rows, cols, intr)
    cfg = O.make_config(L6, intr, thresh=thresh)
    ref = O.track_pairs(cfg, kg, kd, cg, n_threads=8)
    poses, status, st = run_batch(vcfg(0, L=L6, intr=intr, thresh=thresh), kg, kd, cg)
    assert (status == ref["status"]).all() and (st["n_points"][:, :L6] == ref["n_points"]).all()
    assert (st["nb_iter"][:, :L6] == ref["nb_iter"]).all()
    assert (bits(st["lm_model"]) == bits(ref["models"])).all() and (bits(poses) == bits(ref["poses"])).all()
    assert (bits(st["optical_flow"]) == bits(ref["flow"])).all()
    assert ref["n_points"][:, 0].min() > 0


# ---------------------------------------------------------------------------------------------- every REFERENCE kernel form
FORMS = {"one wavefront per pair": {"VORS_REF_COOP": "0"},
         "workgroup of 2": {"VORS_REF_COOP": "2"}, "workgroup of 4": {"VORS_REF_COOP": "4"}, "workgroup of 8": {"VORS_REF_COOP": "8"},
         "hand-over after 25 % to workgroups of 4": {"VORS_REF_COOP": "0", "VORS_REF_HANDOFF_MIN_PAIRS": "1", "VORS_REF_HANDOFF": "25"},
         "hand-over after 1 pair to workgroups of 2": {"VORS_REF_COOP": "0", "VORS_REF_HANDOFF_MIN_PAIRS": "1", "VORS_REF_HANDOFF": "2",
                                                       "VORS_REF_HANDOFF_WAVES": "2"}}


def set_env(monkeypatch, env):
    for k in ("VORS_REF_COOP", "VORS_REF_HANDOFF_MIN_PAIRS", "VORS_REF_HANDOFF", "VORS_REF_HANDOFF_WAVES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("huber", [0.0, 10.0], ids=["l2", "huber10"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=list(MODES.values()))
def test_every_reference_kernel_form_on_the_failure_outcomes(monkeypatch, mode, huber):
    """The pairs that fail after accepted steps are the long ones: the hand-over forms queue them (after the first pair — one without
    depth — has finished) and a workgroup finishes their level from the saved LM state. Whatever form finishes a failing level, the
    keyframe test must warp with the model the level STARTED from (Tracker::track breaks out before `lm_model = ...`)."""
    kg, kd, cg, _ = outcome_scene(mode)
    ref, cls = oracle("outcomes", mode, huber)
    assert cls["o1"].sum() >= 1 and cls["o2"].sum() >= 1 and cls["o3"].sum() >= 1, \
        f"the outcome batch lost an outcome: {cls['o1'].sum()} / {cls['o2'].sum()} / {cls['o3'].sum()}"
    # an outcome-2 pair whose model moved in the failing level: the one whose result differs when the level's progress is kept
    moved = cls["o2"] & (cls["accepted_in_fail"] > 0)
    assert moved.any()
    for name, env in FORMS.items():
        set_env(monkeypatch, env)
        poses, status, st = run_batch(vcfg(mode, huber), kg, kd, cg)
        assert_identical(ref, cls, None, poses, status, st, f"{MODES[mode]}, huber {huber}, {name}")


# ---------------------------------------------------------------------------------------------- EXACT and FUSED
SPLIT_FORMS = [{}, {"VORS_LM_SPLIT": "0"}, {"VORS_LM_SPLIT_ROUNDS": "1"}, {"VORS_LM_SPLIT_LEVELS": "1"},
               {"VORS_LM_SPLIT_LEVELS": "2", "VORS_LM_CHUNKS": "7"}]


@pytest.mark.parametrize("arith", [V.ARITH_EXACT, V.ARITH_FUSED], ids=["exact", "fused"])
@pytest.mark.parametrize("mode,env", [(0, {}), (2, {})] + [(1, e) for e in SPLIT_FORMS],
                         ids=["coarse_to_fine", "dso"] + ["dense-" + ("-".join(f"{k}={v}" for k, v in e.items()) or "default") for e in SPLIT_FORMS])
def test_exact_and_fused_on_the_failure_outcomes(monkeypatch, mode, env, arith):
    """Outcome 1 is structural (a singular level 0): those statuses must equal the oracle's in any arithmetic. Outcome 2 hangs on the
    rounding of nearly singular pivots, so the rest is gated like tests/test_gpu_fused.py: pairs whose status differs from the oracle's,
    or whose pose differs by more than 1e-4, may not exceed the oracle's own summation-order floor (its f64-accumulation build on the
    same batch) + 2 + 2 sqrt(floor). A failed pair keeps its pose exactly; no pose is NaN."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kg, kd, cg, _ = outcome_scene(mode)
    ref, cls = oracle("outcomes", mode, 0.0)
    ref64, _ = oracle("outcomes", mode, 0.0, variant="acc64")
    poses, status, st = run_batch(vcfg(mode, 0.0, arith), kg, kd, cg)
    assert not np.isnan(poses).any()
    structural = cls["o1"] & ~cls["o2"]
    assert structural.sum() >= 6 and (status[structural] == ref["status"][structural]).all()
    assert (poses[status != 0] == A.identity7()).all(), "a failed pair did not keep its (identity) pose"

    def off(p, s):
        return int(((s != ref["status"]) | (np.abs(p - ref["poses"]).max(axis=1) > POSE_TOL)).sum())

    floor = off(ref64["poses"], ref64["status"])
    gate = floor + 2 + 2 * np.sqrt(floor)
    assert off(poses, status) <= gate, f"{off(poses, status)} pairs off the oracle (status or pose beyond 1e-4), floor {floor}"
    # Outcomes 2 and 3 by what they leave behind. A pair that accepted an evaluation with no point inside must end like the oracle's (the
    # NaN energy stops the level as a success; measured: every such pair takes the oracle's path in both arithmetics, final models within
    # 1e-5). A failing outcome-2 pair that took the oracle's path (same status, same iteration counts) must end with the oracle's final
    # model: the model its failing level STARTED from, not the level's last kept model.
    o3 = cls["o3"]
    assert (status[o3] == ref["status"][o3]).all(), "outcome 3: statuses differ from the oracle's"
    same_path = (status == ref["status"]) & (st["nb_iter"][:, :L] == ref["nb_iter"]).all(axis=1)
    check = o3 | (cls["o2"] & same_path)
    dm = np.abs(st["lm_model"][check] - ref["models"][check]).max(axis=1)
    assert (dm < 1e-3).all(), f"final models of outcome-2/3 pairs differ from the oracle's by {dm}"


# ---------------------------------------------------------------------------------------------- sequences
def sequence_frames(mode, n_seq=6, n_frames=8):
    g, d = A.mid_pyramid_sequences(SEED_SEQ | (A.BLOCKY if mode == 2 else 0), n_seq, n_frames, ROWS, COLS, INTR)
    ref = O.track_sequences(O.make_config(L, INTR, candidates_mode=mode), g, d, n_threads=n_seq)
    on_failed = ref["changed_keyframe"].astype(bool) & (ref["status"] == 1)
    assert on_failed.sum() >= 1, "no keyframe switch on a failed frame: the sequences lost their point"
    return g, d, ref


@pytest.mark.parametrize("arith", [V.ARITH_REFERENCE, V.ARITH_FUSED], ids=["reference", "fused"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=list(MODES.values()))
def test_lock_step_sequences_switch_keyframes_on_failed_frames_like_the_oracle(mode, arith):
    import torch
    g, d, ref = sequence_frames(mode)
    n_frames, n_seq = g.shape[:2]
    tg = torch.from_numpy(g).cuda()
    td = torch.from_numpy(d.view(np.int16)).cuda()
    many = V.Trackers(vcfg(mode, arith=arith), n_seq, ROWS, COLS)
    many.init(tg[0].contiguous(), td[0].contiguous())
    for k in range(1, n_frames):
        many.track(tg[k].contiguous(), td[k].contiguous())
        poses, status, _ = many.current_frames()
        st = many.stats()
        assert (status == ref["status"][:, k - 1]).all(), f"frame {k}: statuses differ"
        if arith == V.ARITH_REFERENCE:
            assert (st["change_keyframe"] == ref["changed_keyframe"][:, k - 1]).all(), f"frame {k}: keyframe decisions differ"
            assert (bits(poses) == bits(ref["poses"][:, k - 1])).all(), f"frame {k}: poses differ"
        else:
            assert np.abs(poses - ref["poses"][:, k - 1]).max() < POSE_TOL, f"frame {k}"


@pytest.mark.parametrize("mode", [0, 2], ids=["coarse_to_fine", "dso"])
def test_single_tracker_switches_keyframes_on_failed_frames_like_the_oracle(mode):
    g, d, ref = sequence_frames(mode)
    for s in range(g.shape[1]):
        vt = vcfg(mode).init(0.0, d[0, s], 0.0, g[0, s])
        for k in range(1, g.shape[0]):
            assert vt.track(0.1 * k, d[k, s], 0.1 * k, g[k, s]) == ref["status"][s, k - 1]
            assert bool(vt.last_stats()["change_keyframe"]) == bool(ref["changed_keyframe"][s, k - 1]), f"sequence {s} frame {k}"
            assert (bits(vt.current_frame()[1]) == bits(ref["poses"][s, k - 1])).all(), f"sequence {s} frame {k}"
