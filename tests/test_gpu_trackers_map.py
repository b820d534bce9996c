"""The keyframe map of the lock-step trackers (vors_trackers_enable_map, vors_trackers_map, vors_tracker_enable_map,
vors_tracker_read_map): every new keyframe's cloud is appended on the device to a list per sequence, with a segment record per
keyframe. GPU only.

  1. the inputs reach the cases (partial promotions, >= 3 promotions, none, first and last sequence, a partly kept keyframe)
  2. shadow batch: every segment equals a separate Batch's point_cloud on (keyframe gray, keyframe depth, keyframe pose, weight mask), bytewise
  3. the map only reads: poses, statuses, keyframes, stats and the filter's planes are those of the run without it
  4. clipping by capacity and by max_keyframes: totals and records as unclipped, the written prefix as unclipped
  5. independence of the other sequences and of the stream; two runs are bitwise equal
  6. Tracker(map=...) + read_map() == sequence 0 of an N = 1 handle     7. contracts     8. hostile scenes, no faults

Sequences, twists and seeds are those of tests/test_gpu_trackers_depth_filter.py. The dense shape is 120x160 / 4 levels here (19 200
pixels = two chunks of the pass) against 60x80 / 3 there: intrinsics scale with the image, and the keyframe test reads the flow at the
coarsest level, which is 15x20 in both, so the flow in pixels — and with it the promotion pattern — is that of the smaller shape. The
oracle's tracker on the CPU (oracle.track_sequences on oracle.synth_frame's renderings of the same seeds and twists, dense, 120x160 / 4)
confirms it: promotions per sequence 3, 0, 3, 1, 4, 4 and per frame 0, 3, 1, 3, 1, 3, 1, 2, 1, the same figures as at 60x80 / 3 — the
pattern asserted below — so BASE and SPEED are unchanged.
"""
import functools
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V

BLOCKY = 1 << 63
N_SEQ, N_FRAMES = 6, 10
BASE = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001])
SPEED = np.array([4.0, 0.05, 9.0, 2.0, 6.0, 5.0])
FILTER = (0.02, 255, 1)
SHAPES = {V.CANDIDATES_DENSE: (120, 160, 4), V.CANDIDATES_COARSE_TO_FINE: (96, 128, 4), V.CANDIDATES_DSO: (96, 128, 4)}
MODES = pytest.mark.parametrize("mode", [V.CANDIDATES_DENSE, V.CANDIDATES_COARSE_TO_FINE, V.CANDIDATES_DSO], ids=["dense", "coarse_to_fine", "dso"])
ARITHS = pytest.mark.parametrize("arith", [V.ARITH_REFERENCE, V.ARITH_FUSED], ids=["reference", "fused"])
# (depth filter, min_weight) of a mapped run
VARIANTS = {"plain": (None, 0), "filter0": (FILTER, 0), "filter2": (FILTER, 2)}
VARIANT = pytest.mark.parametrize("variant", list(VARIANTS))
MAX_KF = 16   # > N_FRAMES: nothing is clipped unless a test asks for it


def config(mode, arith):
    rows, cols, L = SHAPES[mode]
    intr = V.scaled_intrinsics(rows, cols)
    return V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, arithmetic=arith)


def large_capacity(mode, level=0):
    rows, cols, _ = SHAPES[mode]
    return (rows >> level) * (cols >> level) * N_FRAMES   # every pixel of every frame


@functools.lru_cache(maxsize=None)
def frames_of(mode):
    """[N_FRAMES] of (gray [N_SEQ, rows, cols] u8, depth int16 holding u16) on the device: 2 % of the depth pixels are 0."""
    import torch
    rows, cols, _ = SHAPES[mode]
    intr = V.scaled_intrinsics(rows, cols)
    out = [V.synth_render_frames([(BLOCKY if mode == V.CANDIDATES_DSO else 0) | (1000 + s) for s in range(N_SEQ)], [k] * N_SEQ,
                                 [BASE * SPEED[s] * k for s in range(N_SEQ)], rows, cols, intr, invalid_percent=2) for k in range(N_FRAMES)]
    torch.cuda.synchronize()
    return out


def read_map(tr):
    """Trackers.map() on the host: counts / n_segments as u32, segments structured; the lists whole (entries past the totals are not data)."""
    import torch
    m = tr.map()
    torch.cuda.synchronize()
    return dict(xyz=m["xyz"].cpu().numpy(), pixel=m["pixel"].cpu().numpy().view(np.uint32), gray=m["gray"].cpu().numpy(),
                counts=m["counts"].cpu().numpy().view(np.uint32), n_segments=m["n_segments"].cpu().numpy().view(np.uint32),
                segments=V.decode_map_segments(m["segments"]))


def run(cfg, frames, rows, cols, map_args=None, depth_filter=None, seqs=None):
    """A Trackers run over `frames` (of the sequences `seqs`) -> (per frame a dict of host arrays: poses, status, kf, stats (k >= 1), with
    a filter depth and weight; the map read after the last frame, or None)."""
    sel = (lambda t: t) if seqs is None else (lambda t: t[seqs].contiguous())
    n = N_SEQ if seqs is None else len(seqs)
    tr = V.Trackers(cfg, n, rows, cols)
    if depth_filter is not None:
        tr.enable_depth_filter(*depth_filter)
    if map_args is not None:
        tr.enable_map(*map_args)
    rec = []
    for k, (g, d) in enumerate(frames):
        g, d = sel(g), sel(d)
        if k == 0:
            tr.init(g, d)
        else:
            tr.track(g, d)
        poses, status, kf = tr.current_frames()
        r = dict(poses=poses, status=status, kf=kf, stats=tr.stats().copy() if k else None)
        if depth_filter is not None:
            dd, ww = tr.keyframe_depth()
            r["depth"], r["weight"] = dd.cpu().numpy().view(np.uint16), ww.cpu().numpy()
        rec.append(r)
    return rec, (read_map(tr) if map_args is not None else None)


@functools.lru_cache(maxsize=None)
def mapped_run(mode, arith, variant, level=0):
    rows, cols, _ = SHAPES[mode]
    depth_filter, min_weight = VARIANTS[variant]
    return run(config(mode, arith), frames_of(mode), rows, cols, (level, large_capacity(mode, level), MAX_KF, min_weight), depth_filter)


@functools.lru_cache(maxsize=None)
def unmapped_run(mode, arith, filtered):
    rows, cols, _ = SHAPES[mode]
    return run(config(mode, arith), frames_of(mode), rows, cols, None, FILTER if filtered else None)[0]


def promotions(rec):
    """[F-1, n] bool: sequence s promoted at frame k (the keyframe index moved)."""
    return np.stack([rec[k]["kf"] != rec[k - 1]["kf"] for k in range(1, len(rec))])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def written(m, s, capacity):
    """The written entries of sequence s's lists, as bytes per list."""
    k = min(int(m["counts"][s]), capacity)
    return {name: m[name][s, :k].tobytes() for name in ("xyz", "pixel", "gray")}


# ------------------------------------------------------------------------------------------------------------ 1
@MODES
@ARITHS
def test_inputs_reach_the_cases(mode, arith):
    rec, m0 = mapped_run(mode, arith, "filter0")
    _, m2 = mapped_run(mode, arith, "filter2")
    for r in (rec, mapped_run(mode, arith, "plain")[0]):
        p = promotions(r)
        per_frame = p.sum(axis=1)
        assert ((per_frame > 0) & (per_frame < N_SEQ)).any(), "no frame on which some but not all sequences promote"
        assert (p.sum(axis=0) >= 3).any(), "no sequence promotes three times"
        assert (p.sum(axis=0) == 0).any(), "every sequence promotes"
        assert p[:, 0].any() and p[:, N_SEQ - 1].any(), "the first and the last sequence must promote"
        assert all((q["status"] == 0).all() for q in r)
    # min_weight = 2 on the same filtered run: the same keyframes, and one of them keeps some but not all of its usable points
    assert same_bits(m0["n_segments"], m2["n_segments"])
    partly = [(s, j) for s in range(N_SEQ) for j in range(int(m0["n_segments"][s])) if 0 < m2["segments"][s, j]["count"] < m0["segments"][s, j]["count"]]
    assert partly, "no keyframe keeps some but not all of its usable points at min_weight 2"
    assert (m2["segments"][:, 0]["count"] == 0).all(), "at init every weight is 1: nothing reaches min_weight 2"


# ------------------------------------------------------------------------------------------------------------ 2
def check_against_shadow(mode, arith, variant, level):
    import torch
    rows, cols, _ = SHAPES[mode]
    depth_filter, min_weight = VARIANTS[variant]
    (rec, m), frames, cap = mapped_run(mode, arith, variant, level), frames_of(mode), large_capacity(mode, level)
    shadow = V.Batch(config(mode, arith), N_SEQ, rows, cols)
    seen = np.zeros(N_SEQ, np.int64)     # segments checked per sequence
    total = np.zeros(N_SEQ, np.int64)    # points of the segments checked
    for k in range(N_FRAMES):
        new = np.arange(N_SEQ) if k == 0 else np.nonzero(rec[k]["kf"] != rec[k - 1]["kf"])[0]
        if len(new) == 0:
            continue
        assert (rec[k]["kf"][new] == k).all()
        gray = frames[k][0][new].contiguous()
        depth = torch.from_numpy(rec[k]["depth"][new].view(np.int16)).cuda() if depth_filter is not None else frames[k][1][new].contiguous()
        keep = torch.from_numpy((rec[k]["weight"][new] >= min_weight).astype(np.uint8)).cuda() if min_weight >= 2 else None
        shadow.prepare_keyframes(gray, depth)
        out = shadow.point_cloud(level, poses=torch.from_numpy(np.ascontiguousarray(rec[k]["poses"][new])).cuda(), keep=keep, capacity=cap, gray=True)
        torch.cuda.synchronize()
        out = {name: t.cpu().numpy() for name, t in out.items()}
        for i, s in enumerate(new):
            j = int(seen[s])
            seg = m["segments"][s, j]
            count = int(out["counts"][i])
            where = f"frame {k} sequence {s} (its keyframe {j})"
            assert seg["frame"] == k and seg["first"] == total[s] and seg["count"] == count, f"{where}: record {seg} against count {count}, first {total[s]}"
            assert same_bits(seg["pose7"], rec[k]["poses"][s]), f"{where}: pose bits"
            a, b = int(total[s]), int(total[s]) + count
            assert same_bits(m["xyz"][s, a:b], out["xyz"][i, :count]), f"{where}: xyz differs from the shadow batch"
            assert same_bits(m["pixel"][s, a:b], out["pixel"][i, :count].view(np.uint32)), f"{where}: pixel differs from the shadow batch"
            assert same_bits(m["gray"][s, a:b], out["gray"][i, :count]), f"{where}: gray differs from the shadow batch"
            seen[s] += 1
            total[s] += count
    assert (m["n_segments"] == seen).all() and (m["counts"] == total).all(), f"totals {m['counts']} / {m['n_segments']} against {total} / {seen}"
    assert total.max() <= cap, "the capacity of this run was meant to clip nothing"
    assert min_weight >= 2 or (total > 0).all()


@MODES
@ARITHS
@VARIANT
def test_shadow_batch_bit_for_bit(mode, arith, variant):
    check_against_shadow(mode, arith, variant, 0)


@ARITHS
def test_shadow_batch_dense_level_1(arith):
    check_against_shadow(V.CANDIDATES_DENSE, arith, "plain", 1)


# ------------------------------------------------------------------------------------------------------------ 3
@MODES
@ARITHS
def test_the_map_only_reads(mode, arith):
    for variant, filtered in (("plain", False), ("filter0", True), ("filter2", True)):
        rec, bare = mapped_run(mode, arith, variant)[0], unmapped_run(mode, arith, filtered)
        for k in range(N_FRAMES):
            for name in ("poses", "status", "kf") + (("stats",) if k else ()) + (("depth", "weight") if filtered else ()):
                assert same_bits(rec[k][name], bare[k][name]), f"{variant} frame {k}: {name} depend on the map"


# ------------------------------------------------------------------------------------------------------------ 4
@MODES
@ARITHS
def test_clipping(mode, arith):
    rows, cols, _ = SHAPES[mode]
    cfg, frames, big = config(mode, arith), frames_of(mode), large_capacity(mode)
    rec, full = mapped_run(mode, arith, "plain")
    s3 = int(np.argmax(promotions(rec).sum(axis=0)))
    assert full["n_segments"][s3] >= 4   # init + three promotions
    seg = full["segments"][s3]
    assert seg[1]["count"] >= 2
    cap = int(seg[1]["first"]) + int(seg[1]["count"]) // 2   # strictly inside keyframe 1's segment, exhausted before the last keyframe
    assert seg[1]["first"] < cap < seg[1]["first"] + seg[1]["count"] <= seg[int(full["n_segments"][s3]) - 1]["first"]
    _, clipped = run(cfg, frames, rows, cols, (0, cap, MAX_KF, 0))
    assert same_bits(clipped["counts"], full["counts"]) and same_bits(clipped["n_segments"], full["n_segments"])
    assert clipped["counts"][s3] > cap
    for s in range(N_SEQ):
        k = int(full["n_segments"][s])
        assert same_bits(clipped["segments"][s, :k], full["segments"][s, :k]), f"sequence {s}: records differ under a capacity of {cap}"
        w = written(clipped, s, cap)
        for name, ref in written(full, s, big).items():
            assert w[name] == ref[:len(w[name])] and len(w[name]) == min(int(full["counts"][s]), cap) * {"xyz": 12, "pixel": 4, "gray": 1}[name], \
                f"sequence {s}: {name} prefix differs under a capacity of {cap}"
    _, few = run(cfg, frames, rows, cols, (0, big, 2, 0))
    assert same_bits(few["counts"], full["counts"]) and same_bits(few["n_segments"], full["n_segments"]) and few["n_segments"][s3] > 2
    for s in range(N_SEQ):
        k = min(int(full["n_segments"][s]), 2)
        assert same_bits(few["segments"][s, :k], full["segments"][s, :k]), f"sequence {s}: records differ under max_keyframes 2"
        assert written(few, s, big) == written(full, s, big), f"sequence {s}: lists differ under max_keyframes 2"


# ------------------------------------------------------------------------------------------------------------ 5
@MODES
def test_independent_of_the_other_sequences_and_of_the_stream(mode):
    import torch
    arith = V.ARITH_FUSED
    rows, cols, _ = SHAPES[mode]
    (_, m), frames, cfg, cap = mapped_run(mode, arith, "filter2"), frames_of(mode), config(mode, arith), large_capacity(mode)
    args = (0, cap, MAX_KF, 2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for s, stream in ((0, None), (N_SEQ - 1, side)):
        if stream is None:
            _, alone = run(cfg, frames, rows, cols, args, FILTER, seqs=[s])
        else:
            with torch.cuda.stream(stream):
                _, alone = run(cfg, frames, rows, cols, args, FILTER, seqs=[s])
            stream.synchronize()
        assert alone["counts"][0] == m["counts"][s] and alone["n_segments"][0] == m["n_segments"][s] and m["counts"][s] > 0
        k = int(m["n_segments"][s])
        assert same_bits(alone["segments"][0, :k], m["segments"][s, :k]), f"sequence {s}: records depend on the company"
        assert written(alone, 0, cap) == written(m, s, cap), f"sequence {s}: lists depend on the company"
    _, again = run(cfg, frames, rows, cols, args, FILTER)
    assert same_bits(again["counts"], m["counts"]) and same_bits(again["n_segments"], m["n_segments"])
    for s in range(N_SEQ):
        k = int(m["n_segments"][s])
        assert same_bits(again["segments"][s, :k], m["segments"][s, :k]) and written(again, s, cap) == written(m, s, cap), f"sequence {s}: two runs differ"


# ------------------------------------------------------------------------------------------------------------ 6
@MODES
@ARITHS
@pytest.mark.parametrize("variant", ["plain", "filter2"])
def test_single_tracker_equals_one_sequence_handle(mode, arith, variant):
    rows, cols, _ = SHAPES[mode]
    frames, cfg, s, cap = frames_of(mode), config(mode, arith), 4, large_capacity(mode)
    depth_filter, min_weight = VARIANTS[variant]
    many, m = run(cfg, frames, rows, cols, (0, cap, MAX_KF, min_weight), depth_filter, seqs=[s])
    host = [(g[s].cpu().numpy(), d[s].cpu().numpy().view(np.uint16)) for g, d in frames]
    one = V.Tracker(cfg, 0.0, host[0][1], 0.0, host[0][0], depth_filter=depth_filter, map=(0, cap, MAX_KF, min_weight))
    first = one.read_map()   # keyframe 0 was emitted by the switch itself
    assert first["n_segments"] == 1 and first["segments"][0]["frame"] == 0 and first["count"] == m["segments"][0, 0]["count"]
    for k in range(1, N_FRAMES):
        assert one.track(float(k), host[k][1], float(k), host[k][0]) == many[k]["status"][0]
    got = one.read_map()
    total, nseg = int(m["counts"][0]), int(m["n_segments"][0])
    assert nseg >= 4 and total > 0
    assert got["count"] == total and got["n_segments"] == nseg
    assert same_bits(got["segments"], m["segments"][0, :nseg])
    assert same_bits(got["xyz"], m["xyz"][0, :total]) and same_bits(got["pixel"], m["pixel"][0, :total]) and same_bits(got["gray"], m["gray"][0, :total])
    part = one.read_map(capacity=total // 2, max_segments=2)   # smaller than the handle's: a prefix, the totals unclipped
    assert part["count"] == total and part["n_segments"] == nseg and len(part["xyz"]) == total // 2 and len(part["segments"]) == 2
    assert same_bits(part["xyz"], got["xyz"][:total // 2]) and same_bits(part["pixel"], got["pixel"][:total // 2])
    assert same_bits(part["gray"], got["gray"][:total // 2]) and same_bits(part["segments"], got["segments"][:2])
    none = one.read_map(capacity=0, max_segments=0)
    assert none["count"] == total and none["n_segments"] == nseg and len(none["xyz"]) == 0 and len(none["segments"]) == 0
    with pytest.raises(V.VorsError, match="before the first"):   # the switch is legal until the first track only
        V._check(V.lib().vors_tracker_enable_map(one._h, 0, cap, MAX_KF, 0))


# ------------------------------------------------------------------------------------------------------------ 7
def test_contracts():
    import torch
    mode = V.CANDIDATES_DSO
    rows, cols, L = SHAPES[mode]
    cfg, frames = config(mode, V.ARITH_FUSED), frames_of(mode)
    plain, batch = V.Trackers(cfg, N_SEQ, rows, cols), V.Batch(cfg, N_SEQ, rows, cols)
    assert plain.workspace_bytes() == batch.workspace_bytes()   # a handle that never enables the map pays nothing
    with pytest.raises(V.VorsError, match="not enabled"):
        plain.map()
    t = V.Trackers(cfg, N_SEQ, rows, cols)
    before = t.workspace_bytes()
    for bad, word in (((-1, 100, 4, 0), "level"), ((L, 100, 4, 0), "level"), ((0, 0, 4, 0), "capacity"), ((0, -5, 4, 0), "capacity"),
                      ((0, 100, 0, 0), "max_keyframes"), ((0, 100, 4, -1), "min_weight"), ((0, 100, 4, 256), "min_weight"),
                      ((0, 100, 4, 2), "depth filter")):
        with pytest.raises(V.VorsError, match=word):
            t.enable_map(*bad)
    assert t.workspace_bytes() == before   # a refused call allocates nothing
    t.enable_depth_filter(0.02)
    filtered = t.workspace_bytes()
    with pytest.raises(V.VorsError, match="level 0"):
        t.enable_map(1, 100, 4, 2)
    assert t.workspace_bytes() == filtered
    cap, nkf = 5000, 3
    t.enable_map(0, cap, nkf, 2)
    enabled = t.workspace_bytes()
    # Count workspace: 4 bytes per sequence and chunk of the level (engine.h eval_pairs_chunks). A DSO list is sized for 8000 candidates
    # and cut into chunks of 4096 points (eval_pairs_chunk_points): 2 chunks.
    chunks = 2
    assert enabled == filtered + N_SEQ * cap * 17 + N_SEQ * nkf * 40 + 8 * N_SEQ + 4 * N_SEQ * chunks
    with pytest.raises(V.VorsError, match="already"):
        t.enable_map(0, cap, nkf, 0)
    assert t.workspace_bytes() == enabled
    t.init(*frames[0])
    for k in range(1, 4):
        t.track(*frames[k])
    first = read_map(t)
    assert t.workspace_bytes() == enabled   # no later call allocates
    assert (first["n_segments"] >= 1).all() and first["n_segments"].max() >= 2
    t.init(*frames[0])   # a second init empties the map
    again = read_map(t)
    assert (again["n_segments"] == 1).all() and (again["segments"][:, 0]["frame"] == 0).all() and (again["segments"][:, 0]["first"] == 0).all()
    assert (again["counts"] == again["segments"][:, 0]["count"]).all()
    assert t.workspace_bytes() == enabled
    plain.init(*frames[0])
    with pytest.raises(V.VorsError, match="before vors_trackers_init"):
        plain.enable_map(0, cap, nkf)
    plain.track(*frames[1])
    torch.cuda.synchronize()
    assert plain.workspace_bytes() == batch.workspace_bytes()
    lib = V.lib()
    assert lib.vors_trackers_enable_map(None, 0, 100, 4, 0) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_trackers_map(None, None, None, None, None, None, None) == -1
    assert lib.vors_trackers_map(t._h, None, None, None, None, None, None) == 0   # every output may be NULL
    assert lib.vors_tracker_enable_map(None, 0, 100, 4, 0) == -1 and lib.vors_tracker_read_map(None, 0, None, None, None, None, 0, None, None) == -1


# ------------------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("name", sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "adversarial", "*.npz"))))
def test_hostile_scenes(name):
    import torch
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "adversarial", name + ".npz"))
    L, mode, rows, cols, intr = int(g["L"]), int(g["mode"]), int(g["rows"]), int(g["cols"]), tuple(float(x) for x in g["intr"])
    kg, cg = (torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("kf_gray", "cur_gray"))
    kd = torch.from_numpy(np.ascontiguousarray(g["kf_depth"]).view(np.int16)).cuda()   # (stands in for the current depth as well)
    n = kg.shape[0]
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, huber_delta=float(g["huber"]),
                   arithmetic=V.ARITH_FUSED)
    cap = 2 * rows * cols
    out = []
    for mapped in (True, False):
        tr = V.Trackers(cfg, n, rows, cols)   # every pair of the scene is one two-frame sequence
        if mapped:
            tr.enable_map(0, cap, 4)
        tr.init(kg, kd)
        tr.track(cg, kd)
        out.append(tr.current_frames())
        if mapped:
            m, stats = read_map(tr), tr.stats()
            assert (m["segments"][:, 0]["count"] == stats["n_points"][:, 0]).all(), "segment 0 must hold the usable points of level 0"
            assert (m["counts"] <= cap).all()
            for s in range(n):
                assert np.isfinite(m["xyz"][s, :int(m["counts"][s])]).all(), f"sequence {s}: a kept point is not finite"
    assert (out[0][1] == out[1][1]).all(), "statuses of the first frame must not depend on the map"
    assert same_bits(out[0][0], out[1][0]) and (out[0][2] == out[1][2]).all()
