"""The LM schedules that only LARGE batches pick, on small images, against the oracle.

The LM stage plans from the handle's capacity and the pair count, never from the image size (batch.cpp plan_split, lm_kernels.hip
VORS_LAUNCH_LM_TRACK, lm_reference.hip launch_lm_track_reference): 256-thread workgroups and 128 chunks from 512 pairs, 64 chunks and the
eight-pairs-per-workgroup step kernel from 1024, the side lane (second stream, fork after round 1, event join three rounds later, merge
through atomics) and 10 rounds from 2048, the straggler cap of max(256, n / 8) workgroups; REFERENCE: workgroups of 8 / 5 / 4 / 3
wavefronts, one wavefront per pair beyond 1280 pairs, the hand-over from 2048. At 120x160 a 4096-pair handle costs milliseconds, so the
whole production decision tree runs here against the oracle:

  * dense EXACT / FUSED at capacities 512 / 1024 (side lane forced) and 2048 / 4096 (default plan): gated against the oracle like
    tests/test_gpu_fused.py, and bit-identical from run to run, on a fresh handle, on the reversed batch, for a count below the capacity
    and after the handle tracked another batch; the schedule forms at capacity 2048; a batch that leaves more pairs iterating after the
    last round than the straggler cap; a tiled hostile batch whose pairs fail inside the level the side lane finishes;
  * REFERENCE with no knob set at every pair count where the launcher takes another form: the oracle's bits.

Each test asserts, from the oracle, that its batch holds what it targets. GPU only."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from oracle import oracle as O

import adversarial as A
import test_gpu_adversarial as TA
import test_gpu_reference as TR

ROWS, COLS, L = 120, 160, 4
INTR = O.scaled_intrinsics(ROWS, COLS)
SEED = 0x5EED7700
N_MAX = 4096
POSE_TOL = 1e-4
N_THREADS = 16
MIN_GROUP = 16  # pairs that must stay in the rounds / go to the side lane in every plain batch
LM_KNOBS = ("VORS_LM_SIDE", "VORS_LM_SPLIT", "VORS_LM_SPLIT_LEVELS", "VORS_LM_SPLIT_ROUNDS", "VORS_LM_CHUNKS", "VORS_LM_BLOCK")
REF_KNOBS = ("VORS_REF_WPB", "VORS_REF_COOP", "VORS_REF_HANDOFF_MIN_PAIRS", "VORS_REF_HANDOFF", "VORS_REF_HANDOFF_WAVES",
             "VORS_REF_RECORDS_GENERIC", "VORS_REF_SORT_REGCAP", "VORS_REF_RANK", "VORS_PIPELINE_INFLIGHT")
ARITHS = [V.ARITH_EXACT, V.ARITH_FUSED]
ARITH_IDS = ["exact", "fused"]
FIELDS = ("poses", "status", "lm_model", "nb_iter", "energy", "optical_flow")


def set_knobs(monkeypatch, env, knobs=LM_KNOBS + REF_KNOBS):
    """The plan is read when the handle is created: every scheduling knob is unset, then `env` is set."""
    for k in knobs:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def dense_env(cap, **more):
    """Levels 1 and 0 by rounds (as at 640x480); the side lane by default from 2048 pairs, forced below."""
    env = {"VORS_LM_SPLIT_LEVELS": "2"}
    if cap < 2048:
        env["VORS_LM_SIDE"] = "1"
    env.update(more)
    return env


# ---------------------------------------------------------------------------------------------- scenes and the oracle, once per module
@functools.lru_cache(maxsize=None)
def plain_scene(blocky=False):
    """N_MAX pairs; pair i depends on SEED + i alone, so every batch of the module is a slice of this one."""
    kg, kd, cg, _, _ = O.synth_batch(N_MAX, ROWS, COLS, seed0=(A.BLOCKY if blocky else 0) | SEED, intr=INTR, motion_scale=1.0)
    return kg, kd, cg


@functools.lru_cache(maxsize=None)
def on_device(scene, arg):
    import torch
    kg, kd, cg = {"plain": plain_scene, "hostile": hostile_scene}[scene](arg)
    return (torch.from_numpy(np.ascontiguousarray(kg)).cuda(), torch.from_numpy(np.ascontiguousarray(kd).view(np.int16)).cuda(),
            torch.from_numpy(np.ascontiguousarray(cg)).cuda())


@functools.lru_cache(maxsize=None)
def _oracle_run(mode, huber, variant, n):
    kg, kd, cg = plain_scene(mode == 2)
    return O.track_pairs(O.make_config(L, INTR, candidates_mode=mode, huber_delta=huber), kg[:n], kd[:n], cg[:n], n_threads=N_THREADS,
                         variant=variant)


def plain_oracle(mode, n, huber=0.0, variant=None):
    """The oracle on the first n plain pairs (a pair's result does not depend on its batch: the L2 runs are slices of one run)."""
    if huber:
        return _oracle_run(mode, huber, variant, n)
    return {k: v[:n] for k, v in _oracle_run(mode, 0.0, variant, N_MAX).items()}


HOSTILE_N = 2048


@functools.lru_cache(maxsize=None)
def hostile_scene(mode):
    """test_gpu_adversarial's outcome batch (96x128, 3 levels; 56 pairs) tiled to HOSTILE_N pairs: pair i is a replica of pair i % 56."""
    kg, kd, cg, _ = TA.outcome_scene(mode)
    idx = np.arange(HOSTILE_N) % len(kg)
    return kg[idx], kd[idx], cg[idx]


def hostile_oracle(mode, variant=None):
    """-> (oracle.track_pairs, adversarial.classify) of the tiled batch: the 56 pairs' results, tiled (classify: None for a variant)."""
    ref, cls = TA.oracle("outcomes", mode, 0.0, variant=variant) if variant else TA.oracle("outcomes", mode, 0.0)
    idx = np.arange(HOSTILE_N) % len(ref["status"])
    return {k: v[idx] for k, v in ref.items()}, (None if cls is None else {k: v[idx] for k, v in cls.items()})


# ---------------------------------------------------------------------------------------------- running and comparing
def vcfg(mode, arith, huber=0.0, levels=L, intr=INTR):
    return V.Config(nb_levels=levels, candidates_diff_threshold=7, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]),
                    candidates_mode=mode, huber_delta=huber, arithmetic=arith)


def track(b, images, levels=L):
    """One track_pairs of handle b on the device tensors `images` -> dict of FIELDS (numpy), n_points."""
    import torch
    n = images[0].shape[0]
    poses = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    status = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    stats = V.stats_tensor(n)
    b.track_pairs(*images, poses, status, stats)
    torch.cuda.synchronize()
    st = V.decode_stats(stats)
    return dict(poses=poses.cpu().numpy(), status=status.cpu().numpy(), lm_model=st["lm_model"].copy(), nb_iter=st["nb_iter"][:, :levels].copy(),
                energy=st["energy"][:, :levels].copy(), optical_flow=st["optical_flow"].copy(), n_points=st["n_points"][:, :levels].copy())


def prefix(images, n):
    return tuple(t[:n] for t in images)


def permuted(images, idx):
    import torch
    i = torch.from_numpy(np.ascontiguousarray(idx)).cuda()
    return tuple(t.index_select(0, i).contiguous() for t in images)


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_bits(got, want, what, idx=None):
    """Every output field of `got` equals `want` (taken at pairs `idx`) bit for bit — NaN payloads included."""
    for f in FIELDS:
        w = want[f] if idx is None else want[f][idx]
        diff = raw(got[f]) != raw(w)
        bad = np.flatnonzero(diff.reshape(len(diff), -1).any(axis=1))
        assert len(bad) == 0, f"{what}: {f} differs in {len(bad)} of {len(diff)} pairs, first {bad[:8]}"


def gate_against_oracle(res, ref, ref64, what, levels=L):
    """tests/test_gpu_fused.py's gate: statuses and point counts equal, a failed pair keeps its (identity) pose, no NaN pose, the pairs
    beyond 1e-4 within the oracle's own summation-order floor (its f64-accumulation build on the same batch) + 2 + 2 sqrt(floor), and the
    99th percentile of the pose error within twice that of the oracle's f32-vs-f64-accumulation difference (two summation orders are two
    independent draws of the same noise)."""
    poses, status = res["poses"], res["status"]
    assert (status == ref["status"]).all(), f"{what}: statuses differ in pairs {np.flatnonzero(status != ref['status'])[:8]}"
    assert (res["n_points"] == ref["n_points"]).all(), what
    assert not np.isnan(poses).any(), what
    assert (poses[status != 0] == A.identity7()).all(), f"{what}: a failed pair did not keep its previous pose"
    err = np.abs(poses - ref["poses"]).max(axis=1)
    err64 = np.abs(ref64["poses"] - ref["poses"]).max(axis=1)
    beyond, floor = int((err > POSE_TOL).sum()), int((err64 > POSE_TOL).sum())
    gate = floor + 2 + 2 * np.sqrt(floor)
    p99, p99_64 = float(np.quantile(err, 0.99)), float(np.quantile(err64, 0.99))
    print(f"[{what}] {len(status)} pairs: beyond 1e-4 {beyond} (floor {floor}, gate {gate:.1f}); p99 {p99:.3e} (oracle f32 vs acc64 {p99_64:.3e}); "
          f"max {err.max():.3e}")
    assert beyond <= gate, f"{what}: {beyond} pairs beyond 1e-4, floor {floor}"
    assert p99 <= 2 * p99_64, f"{what}: p99 of the pose error {p99:.3e} vs {p99_64:.3e} for the oracle's own summation-order probe"


def assert_side_lane_groups(ref, what):
    """The step of round 1 keeps a pair in the rounds when its level 1 is over after ONE iteration and hands every other pair to the
    side lane: both groups must be there, or the test does not run what it is named after."""
    ok = ref["status"] == 0
    stay, side = int((ok & (ref["nb_iter"][:, 1] == 1)).sum()), int((ok & (ref["nb_iter"][:, 1] >= 2)).sum())
    print(f"[{what}] level 1 over after one iteration (stay in the rounds): {stay} pairs; two or more (side lane): {side}")
    assert stay >= MIN_GROUP and side >= MIN_GROUP, f"{what}: {stay} / {side} pairs in the two groups"


_dense_full = {}


def dense_full(monkeypatch, arith, cap):
    """The first `cap` plain pairs on a handle of that capacity (forced side lane below 2048), once per module -> (result, env)."""
    env = dense_env(cap)
    set_knobs(monkeypatch, env)
    if (arith, cap) not in _dense_full:
        _dense_full[arith, cap] = track(V.Batch(vcfg(1, arith), cap, ROWS, COLS), prefix(on_device("plain", False), cap))
    return _dense_full[arith, cap]


CAPS = [512, 1024, 2048, 4096]
CAP_IDS = ["cap512-side", "cap1024-side", "cap2048", "cap4096"]


# ---------------------------------------------------------------------------------------------- dense EXACT / FUSED, plain scene
@pytest.mark.parametrize("cap", CAPS, ids=CAP_IDS)
@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
def test_dense_large_batch_against_the_oracle_deterministic_and_position_independent(monkeypatch, arith, cap):
    what = f"dense {ARITH_IDS[ARITHS.index(arith)]} capacity {cap}"
    ref, ref64 = plain_oracle(1, cap), plain_oracle(1, cap, variant="acc64")
    assert_side_lane_groups(ref, what)
    first = dense_full(monkeypatch, arith, cap)
    gate_against_oracle(first, ref, ref64, what)
    images = prefix(on_device("plain", False), cap)
    b = V.Batch(vcfg(1, arith), cap, ROWS, COLS)
    once = track(b, images)
    assert_same_bits(once, first, f"{what}: a fresh handle")
    assert_same_bits(track(b, images), first, f"{what}: the same handle again")
    rev = np.arange(cap)[::-1]
    assert_same_bits(track(b, permuted(images, rev)), first, f"{what}: the reversed batch", idx=rev)


@pytest.mark.parametrize("cap", CAPS, ids=CAP_IDS)
@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
def test_dense_count_below_capacity_gives_the_bits_of_the_full_batch(monkeypatch, arith, cap):
    what = f"dense {ARITH_IDS[ARITHS.index(arith)]} capacity {cap}"
    full = dense_full(monkeypatch, arith, cap)
    images = on_device("plain", False)
    b = V.Batch(vcfg(1, arith), cap, ROWS, COLS)
    for k in (1500, 1, 300):
        if k < cap:
            assert_same_bits(track(b, prefix(images, k)), full, f"{what}: the first {k} pairs", idx=np.arange(k))


@pytest.mark.parametrize("cap", CAPS, ids=CAP_IDS)
@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
def test_dense_handle_state_is_reset_between_batches(monkeypatch, arith, cap):
    """Batch A, then another batch B (other pairs in every slot, fewer of them: A's side, join and active lists are longer than B's) on
    the same handle: the bits a fresh handle gives for B — side and join counters, lists and events start over with every track."""
    what = f"dense {ARITH_IDS[ARITHS.index(arith)]} capacity {cap}"
    full = dense_full(monkeypatch, arith, cap)
    images = prefix(on_device("plain", False), cap)
    idx_b = np.roll(np.arange(cap), 211)[: cap - 101]
    images_b = permuted(images, idx_b)
    fresh = track(V.Batch(vcfg(1, arith), cap, ROWS, COLS), images_b)
    b = V.Batch(vcfg(1, arith), cap, ROWS, COLS)
    assert_same_bits(track(b, images), full, f"{what}: batch A")
    after = track(b, images_b)
    assert_same_bits(after, fresh, f"{what}: batch B after batch A vs a fresh handle")
    assert_same_bits(after, full, f"{what}: batch B vs its pairs in batch A", idx=idx_b)


# ---------------------------------------------------------------------------------------------- schedule forms at capacity 2048
SCHEDULES = [{}, {"VORS_LM_SIDE": "0"}, {"VORS_LM_SPLIT_ROUNDS": "1"}, {"VORS_LM_SPLIT_ROUNDS": "2"}, {"VORS_LM_SPLIT_ROUNDS": "3"},
             {"VORS_LM_CHUNKS": "64"}]


@pytest.mark.parametrize("env", SCHEDULES, ids=[("-".join(f"{k}={v}" for k, v in e.items()) or "default") for e in SCHEDULES])
@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
def test_dense_schedule_forms_at_capacity_2048(monkeypatch, arith, env):
    """Side lane off; 1, 2 and 3 rounds with the side lane on (the join after the last round; with 1 round a fork that is never
    reached); the production chunk count. Every form is gated against the oracle, whose statuses all forms therefore share."""
    cap = 2048
    what = f"dense {ARITH_IDS[ARITHS.index(arith)]} capacity {cap} {env or 'default'}"
    ref, ref64 = plain_oracle(1, cap), plain_oracle(1, cap, variant="acc64")
    assert_side_lane_groups(ref, what)
    set_knobs(monkeypatch, dense_env(cap, **env))
    gate_against_oracle(track(V.Batch(vcfg(1, arith), cap, ROWS, COLS), prefix(on_device("plain", False), cap)), ref, ref64, what)


@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
def test_dense_more_stragglers_than_the_straggler_grid(monkeypatch, arith):
    """Three rounds at 2048 pairs. A level solved by rounds takes one round for its first evaluation and one per iteration, and two
    levels are solved by rounds: a pair needs (1 + nb_iter[1]) + (1 + nb_iter[0]) >= 4 evaluations, so after three rounds (on the side
    lane or not) every pair that has not failed is still iterating — far more than max(256, n / 8). Whatever finishes them, the result
    of a pair may depend neither on the run nor on where the pair stands in the active list, whose order comes from atomics."""
    cap = 2048
    what = f"dense {ARITH_IDS[ARITHS.index(arith)]} capacity {cap}, 3 rounds"
    ref, ref64 = plain_oracle(1, cap), plain_oracle(1, cap, variant="acc64")
    left = int(((ref["status"] == 0) & ((1 + ref["nb_iter"][:, 1]) + (1 + ref["nb_iter"][:, 0]) > 3)).sum())
    print(f"[{what}] still iterating after three rounds: {left} pairs; straggler grid {max(256, cap // 8)}")
    assert left > max(256, cap // 8)
    assert_side_lane_groups(ref, what)
    set_knobs(monkeypatch, dense_env(cap, VORS_LM_SPLIT_ROUNDS="3"))
    images = prefix(on_device("plain", False), cap)
    b = V.Batch(vcfg(1, arith), cap, ROWS, COLS)
    first = track(b, images)
    gate_against_oracle(first, ref, ref64, what)
    assert_same_bits(track(b, images), first, f"{what}: the same handle again")
    assert_same_bits(track(V.Batch(vcfg(1, arith), cap, ROWS, COLS), images), first, f"{what}: a fresh handle")
    rev = np.arange(cap)[::-1]
    assert_same_bits(track(b, permuted(images, rev)), first, f"{what}: the reversed batch", idx=rev)


# ---------------------------------------------------------------------------------------------- dense EXACT / FUSED, hostile scene
HL = TA.L  # 3 levels of 96 x 128: level 1 has 48 x 64 = 3072 pixels, above FUSED's 2500-point exact rule, so both arithmetics solve it by rounds


def assert_hostile_targets(cls):
    n1, n0 = int((cls["fail_level"] == 1).sum()), int((cls["fail_level"] == 0).sum())
    print(f"[hostile] {len(cls['status'])} pairs: {n1} fail at level 1 (the level the side lane finishes), {n0} at level 0")
    assert n1 >= 1 and n0 >= 1


def assert_replicas_identical(res, n_unique, what):
    assert_same_bits(res, res, f"{what}: replicas of a pair", idx=np.arange(len(res["status"])) % n_unique)


@pytest.mark.parametrize("side", ["default", "VORS_LM_SIDE=0"])
@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
def test_dense_tiled_hostile_batch_through_the_side_lane(monkeypatch, arith, side):
    """test_exact_and_fused_on_the_failure_outcomes on the outcome batch tiled to 2048 pairs: pairs that fail at level 1 fail on the side
    lane, pairs that fail at level 0 after they came back from it, and the long rank-deficient pairs outnumber the straggler grid.
    Replicas of a pair are bit-identical; the counting gate is then that test's, on the 56 distinct pairs (the replicas are not further
    draws)."""
    what = f"hostile dense {ARITH_IDS[ARITHS.index(arith)]} {side}"
    n_unique = len(TA.outcome_scene(1)[0])
    ref, cls = hostile_oracle(1)
    ref64, _ = hostile_oracle(1, variant="acc64")
    assert_hostile_targets(cls)
    set_knobs(monkeypatch, dense_env(HOSTILE_N, **({} if side == "default" else {"VORS_LM_SIDE": "0"})))
    images = on_device("hostile", 1)
    res = track(V.Batch(vcfg(1, arith, levels=HL, intr=TA.INTR), HOSTILE_N, TA.ROWS, TA.COLS), images, levels=HL)
    poses, status = res["poses"], res["status"]
    assert not np.isnan(poses).any()
    structural = cls["o1"] & ~cls["o2"]
    assert structural[:n_unique].sum() >= 6 and (status[structural] == ref["status"][structural]).all()
    assert (poses[status != 0] == A.identity7()).all(), "a failed pair did not keep its (identity) pose"
    assert_replicas_identical(res, n_unique, what)

    def off(p, s):
        return int(((s != ref["status"]) | (np.abs(p - ref["poses"]).max(axis=1) > POSE_TOL))[:n_unique].sum())

    floor = off(ref64["poses"], ref64["status"])
    gate = floor + 2 + 2 * np.sqrt(floor)
    print(f"[{what}] off the oracle (status or pose beyond 1e-4) among the {n_unique} distinct pairs: {off(poses, status)}, floor {floor}, gate {gate:.1f}")
    assert off(poses, status) <= gate, f"{off(poses, status)} pairs off the oracle (status or pose beyond 1e-4), floor {floor}"
    o3 = cls["o3"]
    assert (status[o3] == ref["status"][o3]).all(), "outcome 3: statuses differ from the oracle's"
    same_path = (status == ref["status"]) & (res["nb_iter"] == ref["nb_iter"]).all(axis=1)
    check = o3 | (cls["o2"] & same_path)
    dm = np.abs(res["lm_model"][check] - ref["models"][check]).max(axis=1)
    assert (dm < 1e-3).all(), f"final models of outcome-2/3 pairs differ from the oracle's by {dm.max()}"


# ---------------------------------------------------------------------------------------------- REFERENCE, default environment
REF_SIZES = [257, 513, 769, 1281, 2048, 4096]
HUBER_AT = {0: 513, 1: 1281, 2: 769}  # one size per mode also runs the Huber extension


def run_reference(monkeypatch, mode, n, huber):
    set_knobs(monkeypatch, {})
    res = track(V.Batch(vcfg(mode, V.ARITH_REFERENCE, huber), n, ROWS, COLS), prefix(on_device("plain", mode == 2), n))
    st = dict(n_points=res["n_points"], nb_iter=res["nb_iter"], lm_model=res["lm_model"], optical_flow=res["optical_flow"])
    TR.assert_pairs_identical(plain_oracle(mode, n, huber), res["poses"], res["status"], st, L, f"REFERENCE {TR.MODES[mode]} {n} pairs huber {huber}")


@pytest.mark.parametrize("n", REF_SIZES)
@pytest.mark.parametrize("mode", [0, 1, 2], ids=list(TR.MODES.values()))
def test_reference_default_forms_equal_the_oracle_bit_for_bit(monkeypatch, mode, n):
    run_reference(monkeypatch, mode, n, 0.0)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=list(TR.MODES.values()))
def test_reference_default_forms_with_huber_equal_the_oracle_bit_for_bit(monkeypatch, mode):
    run_reference(monkeypatch, mode, HUBER_AT[mode], 10.0)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=list(TR.MODES.values()))
def test_reference_default_hand_over_on_the_tiled_hostile_batch(monkeypatch, mode):
    """2048 pairs: the hand-over is on by default, and what it queues are the long pairs — here the ones that fail after accepted steps."""
    ref, cls = hostile_oracle(mode)
    assert cls["o1"].sum() >= 1 and cls["o2"].sum() >= 1 and cls["o3"].sum() >= 1
    if mode == 1:
        assert_hostile_targets(cls)
    set_knobs(monkeypatch, {})
    import torch
    images = on_device("hostile", mode)
    n = HOSTILE_N
    poses = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    status = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    stats = V.stats_tensor(n)
    V.Batch(TA.vcfg(mode), n, TA.ROWS, TA.COLS).track_pairs(*images, poses, status, stats)
    torch.cuda.synchronize()
    TA.assert_identical(ref, cls, None, poses.cpu().numpy(), status.cpu().numpy(), V.decode_stats(stats), f"REFERENCE hostile {TR.MODES[mode]}")


@pytest.mark.parametrize("mode", [0, 1], ids=["coarse_to_fine", "dense"])
def test_reference_ring_of_1000_pair_steps_equals_the_oracle_bit_for_bit(monkeypatch, mode):
    """A slot of a ring of depth 3 sizes for 1.5x its step: 1000-pair steps run one wavefront per pair where a lone handle of 1000
    pairs runs workgroups."""
    import torch
    set_knobs(monkeypatch, {})
    n, steps = 1000, 4
    images = on_device("plain", False)
    ref = plain_oracle(mode, n * steps)
    pipe = V.Pipeline(vcfg(mode, V.ARITH_REFERENCE), n, ROWS, COLS, depth=3)
    outs = []
    for k in range(steps):
        out = (torch.zeros((n, 7), dtype=torch.float32, device="cuda"), torch.full((n,), -9, dtype=torch.int32, device="cuda"), V.stats_tensor(n))
        pipe.submit(*(t[k * n:(k + 1) * n] for t in images), *out)
        outs.append(out)
    pipe.drain()
    torch.cuda.synchronize()
    for k, (poses, status, stats) in enumerate(outs):
        TR.assert_pairs_identical({f: v[k * n:(k + 1) * n] for f, v in ref.items()}, poses.cpu().numpy(), status.cpu().numpy(), V.decode_stats(stats), L,
                                  f"REFERENCE ring {TR.MODES[mode]} step {k}")
