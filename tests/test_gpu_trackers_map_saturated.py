"""The keyframe map beyond its two limits — more keyframes than max_keyframes records, more entries than capacity — and every consumer
of that state: the voxel statistics, the resolve's segment search (vors_trackers_map_voxel_means, vors_voxel_means,
vors_tracker_map_voxel_means), the windows and verdicts of the map ICP correction (plain, joint, averaged model) and the single tracker.
GPU only; every comparison is on bits, no tolerance appears. Sequences, shapes, seeds, parameters and helpers are those of
tests/test_gpu_trackers_map.py, test_gpu_trackers_map_voxel_stats.py and test_gpu_trackers_map_icp*.py: six sequences, ten frames,
96x128 / 4 levels coarse-to-fine (120x160 dense where stated), NORMALS, ICP / JOINT with BOUNDS, MEANS = (2, 1) on 0.02 m voxels.

  a. the inputs reach the cases     b. the statistics do not depend on max_keyframes     c. the resolve's segment search, clipped and
  over empty segments               d. every correction at K = 2 is the composition of public entries on a snapshot, the frozen edge
  e. a full list: clipped and empty windows, TOO_FEW, nothing moves; the next sequence's rows     f. Tracker == an N = 1 handle at K = 2

K is the small max_keyframes under test (2 and 3); the FULL run is the same configuration at MAX_KF = 16 and large_capacity, where nothing
is clipped; true_segment(s, r) is the index of the full run's record that holds rank r. The first segment the resolve takes for a rank is
min(true_segment, n_rec - 1), n_rec = min(n_segments, K): product_kernels.hip's rule (the last record whose `first` is <= the rank)
restated without a search; d and e restate it a second time with numpy's searchsorted over the snapshot's own records, since a corrected
run at K has no full twin (its windows, hence its poses, depend on K).

EDGE = 0.75 m, dense: the empty-segment scene. Chosen on the device among 0.3 .. 2.0 m as the first edge at which a later keyframe of a
sequence adds no voxel while a still later one does: filtered counts per keyframe 0: 16 0 0 3, 1: 16, 2: 16 0 4 0, 3: 16 0, 4: 16 0 0 3 5,
5: 16 0 0 2 2 — inner empty records in sequences 0, 2, 4, 5, trailing empty ones in 2 and 3 (at 0.5 m no keyframe is empty, at 0.6 m only
trailing ones, at 1.0 m only trailing ones, at 2.0 m every later keyframe).

MEASURED (MI355X; the tests print these figures; none is a bound):
  unrecorded keyframes: n_segments 3 1 4 2 5 3 coarse-to-fine, 4 1 4 2 5 5 dense; beyond K = 2: 7 / 10 keyframes, beyond K = 3: 3 / 6. Ranks
    whose last segment is an unrecorded keyframe that saw them AGAIN: 1312 / 57232 at K = 2, 796 / 52394 at K = 3; of them first seen by a
    recorded keyframe: 1122 / 48026 and 756 / 48779.
  ranks whose resolve verdict at K differs from the full run's (coarse-to-fine / dense): K = 2: (1, 1) 858 / 10244, (2, 2) 376 / 7608,
    (1, 2) 426 / 15404; K = 3: (1, 1) 274 / 9056, (2, 2) 97 / 4099, (1, 3) 0 / 0; (1, 0) never. The span test mixes the clipped first segment
    with the true last one: a rank first and last seen by unrecorded keyframe j has span j - (K - 1) at K and 0 in the full run. That is
    the rule include/vors_hip.h and product_kernels.hip state, pinned here as stated.
  empty segments: EDGE above; ranks behind an inner empty record, seen by their own keyframe alone, are rejected at min_span 1.
  corrections at K = 2, large capacity: 12 per run; last_keyframes = 1: 3 frozen edges per stage (windows (1497, 2963), (1497, 4441),
    (1471, 2972) plain and joint; (1455, 1908), (1455, 2715), (1431, 2632) averaged model); no empty window.
  a full list: capacity 2237 (lists) / 1964 (0.02 m voxels), 7 of 12 promotions on a full list; last_keyframes = 1, K = 16: 3 empty windows
    (2237, 0) / (1964, 0), all of the busiest sequence 4, each TOO_FEW / ICP_STATUS; K = 2: none — the edge freezes at record 1, below
    the capacity, and the windows stay (1497, 740) / (1455, 509).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
import test_gpu_trackers_map_voxel_stats as VS
from test_gpu_trackers_map import MAX_KF, N_FRAMES, N_SEQ, SHAPES, config, frames_of, large_capacity, mapped_run, promotions, read_map, same_bits
from test_gpu_trackers_map_icp import C2F, DENSE, ICP, NORMALS, keyframe_pose_bits, read_icp
from test_gpu_trackers_map_icp_joint import JOINT, read_joint
from test_gpu_trackers_map_icp_means import MEANS, VOXEL, read_means
from test_map_icp_condition_host import BOUNDS
from test_map_icp_host import window

FUSED = V.ARITH_FUSED
SLOTS = VS.SLOTS
KS = pytest.mark.parametrize("K", [2, 3])
STAT_MODES = pytest.mark.parametrize("mode", [C2F, DENSE], ids=["coarse_to_fine", "dense"])
EDGE = 0.75   # (the docstring)
NAN_BITS = np.uint32(0x7FC00000)


def pairs(K):
    return ((1, 0), (1, 1), (2, 2), (1, K))


# ------------------------------------------------------------------------------------------------------------ runs with statistics
@functools.lru_cache(maxsize=None)
def stats_run(mode, K, voxel_m=None):
    """Voxels and statistics on, ARITH_FUSED, variant plain, max_keyframes K, large_capacity -> (per frame, the map on the host, the handle)."""
    rows, cols, _ = SHAPES[mode]
    vm = VS.VOXEL_M[mode] if voxel_m is None else voxel_m
    return VS.run(VS.config(mode, FUSED), VS.frames_of(mode), rows, cols, (0, VS.large_capacity(mode), K, 0), voxels=(vm, SLOTS), stats=True, keep=True)


def true_segment(full, s):
    """[counts] the index of the full run's record with first <= r < first + count."""
    return VS.segment_of(full, s)


def searched_first_segment(segments, n_segments, K, capacity):
    """[capacity] the last of the min(n_segments, K) records whose `first` is <= the rank: the kernel's rule through numpy's search."""
    n_rec = min(int(n_segments), K)
    firsts = segments["first"][:n_rec].astype(np.int64)
    assert n_rec >= 1 and firsts[0] == 0
    return (np.searchsorted(firsts, np.arange(capacity), side="right") - 1).astype(np.uint32)


def clipped_first_segment(full, m, s, K, capacity):
    """[capacity] min(true_segment, n_rec - 1) below the count, 0 beyond."""
    out = np.zeros(capacity, np.uint32)
    ts = true_segment(full, s)
    out[:len(ts)] = np.minimum(ts, min(int(m["n_segments"][s]), K) - 1)
    return out


# ------------------------------------------------------------------------------------------------------------ a
@STAT_MODES
@KS
def test_inputs_reach_the_cases(mode, K):
    (rec, full, _), (_, m, _) = stats_run(mode, MAX_KF), stats_run(mode, K)
    assert (m["n_segments"] > K).sum() >= 2, f"fewer than two sequences end with n_segments > {K}: {m['n_segments']}"
    assert (promotions(rec).sum(axis=0) == 0).any() and (m["n_segments"] == 1).any(), "every sequence promotes"
    again = straddle = 0
    for s in range(N_SEQ):
        k = int(m["counts"][s])
        ts, last = true_segment(full, s).astype(np.int64), m["obs"][s, :k, 1].astype(np.int64)
        again += int(((last >= K) & (ts < last)).sum())
        straddle += int(((ts < K) & (K <= last)).sum())
    print(f"\n{mode=} K={K}: n_segments {m['n_segments'].tolist()}, unrecorded keyframes {int(np.maximum(m['n_segments'].astype(np.int64) - K, 0).sum())}, "
          f"ranks seen again by an unrecorded keyframe {again}, of them first seen by a recorded one {straddle}")
    assert again >= 1, f"no rank below the clipped count has obs[r][1] >= {K} from a keyframe that saw it again"
    assert straddle >= 1, f"no rank has true_segment < {K} <= obs[r][1]"


# ------------------------------------------------------------------------------------------------------------ b
@STAT_MODES
@KS
def test_statistics_do_not_depend_on_max_keyframes(mode, K):
    (_, full, _), (_, m, _), want = stats_run(mode, MAX_KF), stats_run(mode, K), VS.host_stats(mode, FUSED, "plain")
    cap = VS.large_capacity(mode)
    assert m["segments"].shape == (N_SEQ, K)
    for name in ("counts", "n_segments", "occupied", "overflow"):
        assert same_bits(m[name], full[name]), f"{name} depends on max_keyframes: {m[name]} against {full[name]}"
    assert (m["overflow"] == 0).all() and (m["counts"] <= cap).all()
    for s in range(N_SEQ):
        k, j = int(full["counts"][s]), min(int(full["n_segments"][s]), K)
        for name in ("xyz", "pixel", "gray", "sums", "obs"):
            assert same_bits(m[name][s, :k], full[name][s, :k]), f"sequence {s}: {name} below the count depends on max_keyframes {K}"
        assert same_bits(m["segments"][s, :j], full["segments"][s, :j]), f"sequence {s}: the first {j} records differ from the full run's"
        assert want[s]["total"] == k
        assert same_bits(m["sums"][s, :k], want[s]["sums"]), f"sequence {s}: sums differ from the host twin with the true segment_of"
        assert same_bits(m["obs"][s, :k], want[s]["obs"]), f"sequence {s}: obs differ from the host twin with the true segment_of"
        if int(full["n_segments"][s]) > K:
            assert int(m["obs"][s, :k, 1].max()) == int(full["n_segments"][s]) - 1, f"sequence {s}: the last keyframe's index is not the true one"
    VS.check_rows_beyond_are_zero(m, cap, f"max_keyframes {K}")


# ------------------------------------------------------------------------------------------------------------ c
def check_resolve(mode, K, voxel_m=None):
    """The handle resolve at every threshold pair against vors_voxel_means_host with min(true_segment, n_rec - 1), the handle-free pass
    with that array, sentinels -> per pair [N_SEQ] lists of the finite masks."""
    import torch
    (_, full, _), (_, m, tr) = stats_run(mode, MAX_KF, voxel_m), stats_run(mode, K, voxel_m)
    cap, vm = VS.large_capacity(mode), VS.VOXEL_M[mode] if voxel_m is None else voxel_m
    fs = np.stack([clipped_first_segment(full, m, s, K, cap) for s in range(N_SEQ)])
    for s in range(N_SEQ):   # the two restatements of the rule agree
        k = int(m["counts"][s])
        assert (fs[s, :k] == searched_first_segment(m["segments"][s], m["n_segments"][s], K, cap)[:k]).all(), f"sequence {s}: the two restatements differ"
    fs_t = torch.from_numpy(fs.view(np.int32)).cuda()
    dev_map, dev_stats = tr.map(copy=False), tr.map_voxel_stats(copy=False)
    masks = {}
    for min_count, min_span in pairs(K):
        sentinel = torch.full((N_SEQ, cap, 3), -7.0, dtype=torch.float32, device="cuda")
        gsent = torch.full((N_SEQ, cap), 201, dtype=torch.uint8, device="cuda")
        own = tr.map_voxel_means(min_count, min_span, xyz_mean=sentinel, gray_mean=gsent)
        free = V.voxel_means(dev_map["xyz"], dev_map["counts"], dev_stats["sums"], dev_stats["obs"], vm, min_count, min_span, first_segment_of_rank=fs_t)
        torch.cuda.synchronize()
        xm, gm, kept = own["xyz_mean"].cpu().numpy(), own["gray_mean"].cpu().numpy(), own["kept"].cpu().numpy()
        fx, fg, fk = free["xyz_mean"].cpu().numpy(), free["gray_mean"].cpu().numpy(), free["kept"].cpu().numpy()
        masks[(min_count, min_span)] = []
        for s in range(N_SEQ):
            k = int(m["counts"][s])
            want = V.voxel_means_host(m["xyz"][s, :k], m["sums"][s, :k], m["obs"][s, :k], vm, min_count, min_span, fs[s, :k])
            where = f"max_keyframes {K} min_count {min_count} min_span {min_span} sequence {s}"
            assert same_bits(xm[s, :k].view(np.uint32), want["xyz_mean"].view(np.uint32)), f"{where}: centroids differ from the host twin on the documented first segment"
            assert same_bits(gm[s, :k], want["gray_mean"]), f"{where}: mean grey"
            assert same_bits(fx[s, :k].view(np.uint32), xm[s, :k].view(np.uint32)) and same_bits(fg[s, :k], gm[s, :k]), f"{where}: the handle-free pass on the explicit array"
            finite = np.isfinite(xm[s, :k]).all(axis=1)
            assert (xm[s, :k][~finite].view(np.uint32) == NAN_BITS).all() and (gm[s, :k][~finite] == 0).all()
            assert int(kept[s]) == want["kept"] == int(finite.sum()) == int(fk[s]), f"{where}: kept {kept[s]} / {fk[s]} against {want['kept']} / {int(finite.sum())} finite rows"
            assert (xm[s, k:] == -7.0).all() and (gm[s, k:] == 201).all(), f"{where}: the pass wrote at or beyond the clipped count"
            masks[(min_count, min_span)].append(finite)
    return masks


@STAT_MODES
@KS
def test_resolve_takes_the_documented_first_segment(mode, K):
    import torch
    masks = check_resolve(mode, K)
    (_, full, full_tr), (_, m, _) = stats_run(mode, MAX_KF), stats_run(mode, K)
    differ = {}
    for min_count, min_span in pairs(K):
        xf = full_tr.map_voxel_means(min_count, min_span)["xyz_mean"]
        torch.cuda.synchronize()
        xf = xf.cpu().numpy()
        differ[(min_count, min_span)] = sum(int((np.isfinite(xf[s, :int(m["counts"][s])]).all(axis=1) != masks[(min_count, min_span)][s]).sum()) for s in range(N_SEQ))
    print(f"\n{mode=} K={K}: ranks whose verdict differs from the full run's, per (min_count, min_span): {differ}")
    assert differ[(1, 0)] == 0, "min_span 0 reads no segment"
    assert max(differ.values()) >= 1, "no rank's verdict differs from the full run's: the clipped rule was never distinguishable"


def empty_segment_cases(m):
    inner = [s for s in range(N_SEQ) if any(m["segments"][s, j]["count"] == 0 and m["segments"][s, j + 1]["count"] > 0 for j in range(int(m["n_segments"][s]) - 1))]
    trailing = [s for s in range(N_SEQ) if m["n_segments"][s] > 1 and m["segments"][s, int(m["n_segments"][s]) - 1]["count"] == 0]
    return inner, trailing


def test_resolve_over_empty_segments():
    """EDGE (the docstring): the empty records sit inside the MAX_KF records, so the search meets equal `first` values."""
    _, m, _ = stats_run(DENSE, MAX_KF, EDGE)
    assert (m["n_segments"] <= MAX_KF).all() and (m["overflow"] == 0).all()
    inner, trailing = empty_segment_cases(m)
    print(f"\nedge {EDGE}: counts per keyframe {[m['segments'][s, :int(m['n_segments'][s])]['count'].tolist() for s in range(N_SEQ)]}, inner empty in {inner}, "
          f"trailing empty in {trailing}")
    assert inner, "no sequence has an empty recorded segment followed by a recorded segment with points"
    assert trailing, "no sequence has a trailing empty recorded segment"
    masks = check_resolve(DENSE, MAX_KF, EDGE)
    # the ranks behind an inner empty segment belong to the LATER record: seen by it alone they have span 0 and fail min_span 1
    behind = 0
    for s in inner:
        seg, n = m["segments"][s], int(m["n_segments"][s])
        for j in range(1, n):
            if seg[j]["count"] > 0 and seg[j - 1]["count"] == 0:
                r = slice(int(seg[j]["first"]), int(seg[j]["first"]) + int(seg[j]["count"]))
                only = m["obs"][s, r, 1] == j
                assert not masks[(1, 1)][s][r][only].any(), f"sequence {s}: a rank seen by keyframe {j} alone passed min_span 1"
                behind += int(only.sum())
    assert behind >= 1, "no rank behind an empty segment was seen by its own keyframe alone"


# ------------------------------------------------------------------------------------------------------------ d, e: the correction stages
STAGES = ("plain", "joint", "means")


def stage_params(stage, last_keyframes):
    return dict(dict(JOINT, **BOUNDS) if stage == "joint" else ICP, last_keyframes=last_keyframes)


def stage_handle(stage, K, capacity, last_keyframes, n=N_SEQ):
    """A coarse-to-fine FUSED handle with a level-0 map of `capacity` entries and K records, normals and one stage; "means": the plain
    stage with the averaged model on a voxel-filtered map with statistics."""
    rows, cols, _ = SHAPES[C2F]
    tr = V.Trackers(config(C2F, FUSED), n, rows, cols)
    tr.enable_map(0, capacity, K, 0)
    if stage == "means":
        tr.enable_map_voxels(VOXEL[C2F], SLOTS)
        tr.enable_map_voxel_stats()
    tr.enable_map_normals(*NORMALS)
    params = stage_params(stage, last_keyframes)
    tr.enable_map_icp_joint(**params) if stage == "joint" else tr.enable_map_icp(**params)
    if stage == "means":
        tr.enable_map_icp_means(*MEANS)
    return tr


@functools.lru_cache(maxsize=None)
def corrections(stage, K, capacity, last_keyframes, seqs=None):
    """Ten frames of a stage_handle; before every track call what the stage will read is snapshot on the device (clones), after it EVERY
    attempted correction is compared with the host twins and the handle-free public entries on the snapshot, every sequence that did
    not promote with its own state before the call. -> dict: "events", one per attempted correction, the final map on the host (with
    normals, with means sums / obs / staging)."""
    import torch
    rows, cols, _ = SHAPES[C2F]
    n = N_SEQ if seqs is None else len(seqs)
    frames = frames_of(C2F) if seqs is None else [(g[list(seqs)].contiguous(), d[list(seqs)].contiguous()) for g, d in frames_of(C2F)]
    cam5 = np.array(V.scaled_intrinsics(rows, cols), np.float32)
    params, joint, means = stage_params(stage, last_keyframes), stage == "joint", stage == "means"
    tr = stage_handle(stage, K, capacity, last_keyframes, n)
    tr.init(*frames[0])
    want_xyz, want_gray = np.zeros((n, capacity, 3), np.uint32), np.zeros((n, capacity), np.uint8)   # the staging, as init leaves it
    true_last_first = np.zeros(n, np.int64)   # `first` of every sequence's true last keyframe, recorded or not
    events = []
    for k in range(1, N_FRAMES):
        g, d = frames[k]
        snap, snap_normals, before = tr.map(), tr.map_normals(), read_map(tr)
        assert tuple(snap_normals.shape) == (n, capacity, 3) and tuple(snap["xyz"].shape) == (n, capacity, 3), "a rank at or beyond capacity has no row"
        kf_before, totals_before = keyframe_pose_bits(tr), read_icp(tr)[1]
        if means:
            st = tr.map_voxel_stats()
            fs = np.stack([searched_first_segment(before["segments"][s], before["n_segments"][s], K, capacity) for s in range(n)])
            pre = V.voxel_means(snap["xyz"], snap["counts"], st["sums"], st["obs"], VOXEL[C2F], *MEANS,
                                first_segment_of_rank=torch.from_numpy(fs.view(np.int32)).cuda())
            model_xyz, model_gray = pre["xyz_mean"], pre["gray_mean"]
        else:
            model_xyz, model_gray = snap["xyz"], snap["gray"]
        tr.track(g, d)
        o_poses, _, o_kf = tr.current_frames()
        rec, totals = read_icp(tr)
        jrec = read_joint(tr) if joint else None
        staged = read_means(tr) if means else None
        kf_pose, after = keyframe_pose_bits(tr), read_map(tr)
        new = np.nonzero(o_kf == k)[0]
        assert ((rec["verdict"] != V.MAP_ICP_NOT_ATTEMPTED) == (o_kf == k)).all(), f"frame {k}: attempts {rec['verdict']} against promotions {o_kf == k}"
        ranges = np.zeros((n, 2), np.uint32)
        for s in new:
            nseg, count = int(before["n_segments"][s]), int(before["counts"][s])
            host = V.map_icp_window_host(before["segments"][s, :min(nseg, K)], nseg, K, count, capacity, last_keyframes)
            assert host == window(before["segments"][s], nseg, K, count, capacity, last_keyframes), f"frame {k} sequence {s}: the host twin against its restatement"
            ranges[s] = host
        fn = V.depth_normals(d, cam5, V.DEPTH_SCALE, *NORMALS)["normals"]
        start = torch.from_numpy(np.ascontiguousarray(rec["pose_before"])).cuda()
        common = dict(damping=0.0, step_eps=1e-5, iters=params["iters"], min_points=6, frame_normals=fn, min_cos=params["min_cos"],
                      huber_m=params["huber_m"], ranges=torch.from_numpy(ranges.view(np.int32)).cuda(), gate_counts=True, sums29=True)
        if joint:
            ref = V.icp_points_joint(model_xyz, snap_normals, model_gray, snap["counts"], d, g, cam5, V.DEPTH_SCALE, start, params["dist_m"],
                                     photo_scale_m=params["photo_scale_m"], photo_huber_grey=params["photo_huber_grey"], photo_counts=True, **common)
            dil, flags = V.icp_condition(ref["sums29"])
        else:
            ref = V.icp_points_robust(model_xyz, snap_normals, snap["counts"], d, cam5, V.DEPTH_SCALE, start, params["dist_m"], **common)
        torch.cuda.synchronize()
        ref_pose, ref_stats = ref["poses"].cpu().numpy(), V.decode_icp_stats(ref["stats"])
        ref_gates = ref["gate_counts"].cpu().numpy().view(np.uint32)
        if means:
            pre_xyz, pre_gray = pre["xyz_mean"].cpu().numpy().view(np.uint32), pre["gray_mean"].cpu().numpy()
        for s in range(n):
            r, where = rec[s], f"{stage} K={K} capacity={capacity} last_keyframes={last_keyframes} frame {k} sequence {s}"
            if s not in new:
                assert r["verdict"] == V.MAP_ICP_NOT_ATTEMPTED and (r["range_first"], r["range_count"]) == (0, 0), f"{where}: not promoted, record {r}"
                assert same_bits(r["pose_before"], kf_before[s]) and same_bits(r["pose_after"], kf_before[s]) and same_bits(kf_pose[s], kf_before[s]), \
                    f"{where}: not promoted, but its keyframe pose moved"
                assert same_bits(totals[s], totals_before[s]), f"{where}: not promoted, but its totals moved"
                assert before["n_segments"][s] == after["n_segments"][s] and before["counts"][s] == after["counts"][s]
                assert not joint or jrec[s].tobytes() == bytes(20), f"{where}: joint record {jrec[s]}"
                assert not means or staged["records"][s].tobytes() == bytes(8), f"{where}: means record {staged['records'][s]}"
                continue
            first, count = int(ranges[s, 0]), int(ranges[s, 1])
            assert r["frame"] == k and (r["range_first"], r["range_count"]) == (first, count), f"{where}: window {r['range_first'], r['range_count']} against {first, count}"
            assert first + count == min(int(before["counts"][s]), capacity)
            assert r["stats"]["considered"] == count, f"{where}: considered is not the window's length"
            assert same_bits(r["pose_after"], ref_pose[s]), f"{where}: pose_after differs from the public entry on the snapshot"
            assert r["stats"].tobytes() == ref_stats[s].tobytes(), f"{where}: stats {r['stats']} against {ref_stats[s]}"
            assert same_bits(r["gate_counts"], ref_gates[s]), f"{where}: gate counts {r['gate_counts']} against {ref_gates[s]}"
            if joint:
                j, dd, ff = jrec[s], dil.cpu().numpy(), flags.cpu().numpy()
                assert same_bits(np.array([j["dilution_t"], j["dilution_r"]], np.float32), dd[s]) and j["condition_flags"] == ff[s], f"{where}: {j}"
                assert same_bits(j["photo_counts"], ref["photo_counts"].cpu().numpy().view(np.uint32)[s]), f"{where}: photo counts"
                want = V.map_icp_verdict_joint_host(params, ref_stats[s], r["pose_before"], ref_pose[s], dd[s, 0], dd[s, 1])
            else:
                want = V.map_icp_verdict_host(params, ref_stats[s], r["pose_before"], ref_pose[s])
            assert r["verdict"] == want, f"{where}: verdict {r['verdict']} against the host twin's {want}"
            accepted = want == V.MAP_ICP_ACCEPTED
            assert totals[s, 0] == totals_before[s, 0] + 1 and totals[s, 1] == totals_before[s, 1] + accepted, f"{where}: totals {totals[s]} after {totals_before[s]}"
            reported = r["pose_after"] if accepted else r["pose_before"]
            assert same_bits(o_poses[s], reported) and same_bits(kf_pose[s], reported), f"{where}: the pose reported is not the {'accepted' if accepted else 'unchanged'} one"
            nseg = int(after["n_segments"][s])
            assert nseg == int(before["n_segments"][s]) + 1
            if nseg <= K:   # the new keyframe has a record
                seg = after["segments"][s, nseg - 1]
                assert seg["frame"] == k and seg["first"] == before["counts"][s] and same_bits(seg["pose7"], reported), f"{where}: the new segment's record {seg}"
            if means:
                mr, w = staged["records"][s], slice(first, first + count)
                nan = pre_xyz[s, w, 0] == NAN_BITS
                assert (mr["resolved"], mr["kept"]) == (count, int((~nan).sum())), f"{where}: means record {mr} against {count, int((~nan).sum())}"
                assert r["stats"]["matched"] <= mr["kept"]
                want_xyz[s, w], want_gray[s, w] = pre_xyz[s, w], pre_gray[s, w]
            if count == 0:   # an empty window of a promoted sequence: attempted, TOO_FEW, nothing moves
                assert r["stats"]["status"] == V.ICP_TOO_FEW and r["verdict"] == V.MAP_ICP_ICP_STATUS, f"{where}: an empty window gave {r['stats']}, verdict {r['verdict']}"
                assert same_bits(r["pose_after"], r["pose_before"]) and same_bits(o_poses[s], r["pose_before"]) and same_bits(kf_pose[s], r["pose_before"])
                assert not means or staged["records"][s].tobytes() == bytes(8)
            events.append(dict(k=k, s=s, first=first, count=count, verdict=int(want), status=int(r["stats"]["status"]),
                               frozen=last_keyframes == 1 and first < true_last_first[s], full_before=int(before["counts"][s]) >= capacity))
        if means:   # the staging whole: this call's windows, earlier bytes everywhere else
            assert same_bits(staged["xyz"], want_xyz), f"{stage} K={K} frame {k}: the staged centroids are not the public resolve's inside the windows, untouched outside"
            assert same_bits(staged["gray"], want_gray), f"{stage} K={K} frame {k}: the staged grey"
        for s in new:
            true_last_first[s] = int(before["counts"][s])
    m = read_map(tr)
    m["normals"] = tr.map_normals().cpu().numpy()
    if means:
        st = tr.map_voxel_stats()
        m["sums"], m["obs"], m["staged_xyz"], m["staged_gray"] = st["sums"].cpu().numpy(), st["obs"].cpu().numpy(), want_xyz, want_gray
    torch.cuda.synchronize()
    return dict(events=events, map=m)


def describe(out):
    ev = out["events"]
    return (f"{len(ev)} corrections, verdicts {[e['verdict'] for e in ev]}, windows {[(e['first'], e['count']) for e in ev]}, frozen edges {sum(e['frozen'] for e in ev)}, "
            f"empty windows {sum(e['count'] == 0 for e in ev)}, promotions on a full list {sum(e['full_before'] for e in ev)}")


# ------------------------------------------------------------------------------------------------------------ d
@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("last_keyframes", [0, 1, 2])
def test_every_correction_at_two_records(stage, last_keyframes):
    K, cap = 2, large_capacity(C2F)
    out = corrections(stage, K, cap, last_keyframes)
    print(f"\n{stage} K={K} last_keyframes={last_keyframes}: {describe(out)}; n_segments {out['map']['n_segments'].tolist()}")
    ev, m = out["events"], out["map"]
    assert len(ev) >= 10, f"only {len(ev)} corrections were attempted"
    assert (m["n_segments"] > K).sum() >= 2 and (m["n_segments"] == 1).any()
    assert all(e["count"] > 0 for e in ev), "a list that is not full has no empty window"
    if last_keyframes == 0:
        assert all(e["first"] == 0 for e in ev)
    if last_keyframes == 1:
        assert any(e["frozen"] for e in ev), "no window's lower edge lies below the `first` of the true last keyframe: the frozen edge was never seen"
    if last_keyframes >= K:   # n_rec <= last_keyframes: the whole map, whatever the number of keyframes
        assert all(e["first"] == 0 for e in ev)


# ------------------------------------------------------------------------------------------------------------ e
@functools.lru_cache(maxsize=None)
def capacity_inside_keyframe_1(stage):
    """(the busiest sequence, a capacity strictly inside its keyframe 1's segment) from the stage-less full run of the stage's map."""
    rec, full = (VS.voxel_run(C2F, FUSED, "plain", True, VOXEL[C2F]) if stage == "means" else mapped_run(C2F, FUSED, "plain"))[:2]
    s3 = int(np.argmax(promotions(rec).sum(axis=0)))
    seg = full["segments"][s3]
    assert full["n_segments"][s3] >= 4 and seg[1]["count"] >= 2 and s3 + 1 < N_SEQ
    return s3, int(seg[1]["first"]) + int(seg[1]["count"]) // 2


@pytest.mark.parametrize("stage", ["plain", "means"])
@pytest.mark.parametrize("K", [MAX_KF, 2])
@pytest.mark.parametrize("last_keyframes", [0, 1])
def test_a_full_list(stage, K, last_keyframes):
    s3, cap = capacity_inside_keyframe_1(stage)
    out = corrections(stage, K, cap, last_keyframes)
    print(f"\n{stage} K={K} capacity={cap} last_keyframes={last_keyframes}: {describe(out)}; counts {out['map']['counts'].tolist()}")
    ev, m = out["events"], out["map"]
    seg = m["segments"][s3]
    assert seg[1]["first"] < cap < seg[1]["first"] + seg[1]["count"], f"the capacity {cap} is not strictly inside keyframe 1's segment {seg[1]} of sequence {s3}"
    assert m["counts"][s3] > cap and m["normals"].shape == (N_SEQ, cap, 3) and m["xyz"].shape == (N_SEQ, cap, 3)
    assert any(e["full_before"] for e in ev), "no promotion happened on a sequence whose counts >= capacity before the call"
    empty = [e for e in ev if e["count"] == 0]
    assert all(e["first"] == cap and e["full_before"] and e["status"] == V.ICP_TOO_FEW and e["verdict"] == V.MAP_ICP_ICP_STATUS for e in empty)
    if last_keyframes == 0:
        assert not empty and all(e["first"] == 0 for e in ev)
    elif K == MAX_KF:
        # sequence s3's keyframe 2 starts beyond the capacity and has a record: its later promotions see (capacity, 0)
        assert any(e["s"] == s3 for e in empty), f"no empty window occurred for sequence {s3}"
    if last_keyframes == 1:
        # the next sequence's rows: a store past sequence s3's `cap` rows, of any array of the map, would land there
        alone = corrections(stage, K, cap, last_keyframes, seqs=(s3 + 1,))["map"]
        assert alone["counts"][0] == m["counts"][s3 + 1] and alone["n_segments"][0] == m["n_segments"][s3 + 1]
        j = min(int(alone["n_segments"][0]), K)
        assert same_bits(alone["segments"][0, :j], m["segments"][s3 + 1, :j]), f"sequence {s3 + 1}: records differ from its run alone"
        k = min(int(alone["counts"][0]), cap)
        for name in ("xyz", "pixel", "gray", "normals") + (("sums", "obs") if stage == "means" else ()):
            assert same_bits(alone[name][0, :k], m[name][s3 + 1, :k]), f"sequence {s3 + 1}: {name} differs from its run alone"
        if stage == "means":
            assert same_bits(alone["staged_xyz"][0], m["staged_xyz"][s3 + 1]) and same_bits(alone["staged_gray"][0], m["staged_gray"][s3 + 1])
            assert not m["sums"][s3 + 1, k:].any() and not m["obs"][s3 + 1, k:].any()


# ------------------------------------------------------------------------------------------------------------ f
def test_single_tracker_equals_one_sequence_handle_at_two_records():
    """K = 2, the averaged model at last_keyframes = 1: the map records, the four resolves (the host's linear walk against the device's
    binary search) and the ICP records."""
    import torch
    K, s, cap, last = 2, 4, large_capacity(C2F), 1
    frames = frames_of(C2F)
    one_seq = [(g[[s]].contiguous(), d[[s]].contiguous()) for g, d in frames]
    host = [(g[s].cpu().numpy(), d[s].cpu().numpy().view(np.uint16)) for g, d in frames]
    tr = stage_handle("means", K, cap, last, n=1)
    one = V.Tracker(config(C2F, FUSED), 0.0, host[0][1], 0.0, host[0][0], map=(0, cap, K, 0), map_voxels=(VOXEL[C2F], SLOTS), map_voxel_stats=True,
                    map_normals=NORMALS, map_icp=stage_params("means", last), map_icp_means=MEANS)
    tr.init(*one_seq[0])
    attempted = 0
    for k in range(1, N_FRAMES):
        tr.track(*one_seq[k])
        _, status, _ = tr.current_frames()
        assert one.track(float(k), host[k][1], float(k), host[k][0]) == status[0]
        rec, totals = read_icp(tr)
        got = one.read_map_icp()
        assert got["record"].tobytes() == rec[0].tobytes(), f"frame {k}: record {got['record']} against {rec[0]}"
        assert same_bits(got["totals"], totals[0])
        assert one.read_map_icp_means().tobytes() == read_means(tr)["records"][0].tobytes(), f"frame {k}: means record"
        attempted += got["record"]["verdict"] != V.MAP_ICP_NOT_ATTEMPTED
    m, final = read_map(tr), one.read_map()
    nseg, total = int(m["n_segments"][0]), int(m["counts"][0])
    assert attempted >= 3 and nseg > K, f"sequence {s} was meant to outgrow {K} records: {nseg} keyframes"
    assert final["n_segments"] == nseg and final["count"] == total and len(final["segments"]) == K
    assert same_bits(final["segments"], m["segments"][0, :K]) and same_bits(final["xyz"], m["xyz"][0, :total])
    for min_count, min_span in pairs(K):
        want = tr.map_voxel_means(min_count, min_span)
        torch.cuda.synchronize()
        mine = one.map_voxel_means(min_count, min_span)
        assert same_bits(mine["xyz_mean"].view(np.uint32), want["xyz_mean"][0, :total].cpu().numpy().view(np.uint32)), f"{(min_count, min_span)}: the linear walk against the search"
        assert same_bits(mine["gray_mean"], want["gray_mean"][0, :total].cpu().numpy()) and mine["kept"] == int(want["kept"][0])


def test_single_tracker_over_empty_segments():
    """EDGE, dense, MAX_KF records: a sequence with an inner and a trailing empty record; the four resolves of the two forms."""
    import torch
    _, m6, _ = stats_run(DENSE, MAX_KF, EDGE)
    inner, trailing = empty_segment_cases(m6)
    both = [s for s in inner if s in trailing] or inner
    assert both, "no sequence has an inner empty record"
    s = both[0]
    rows, cols, _ = SHAPES[DENSE]
    cap, vox, frames = VS.large_capacity(DENSE), (EDGE, SLOTS), VS.frames_of(DENSE)
    many, m, tr = VS.run(VS.config(DENSE, FUSED), frames, rows, cols, (0, cap, MAX_KF, 0), seqs=[s], voxels=vox, stats=True, keep=True)
    host = [(g[s].cpu().numpy(), d[s].cpu().numpy().view(np.uint16)) for g, d in frames]
    one = V.Tracker(VS.config(DENSE, FUSED), 0.0, host[0][1], 0.0, host[0][0], map=(0, cap, MAX_KF, 0), map_voxels=vox, map_voxel_stats=True)
    for k in range(1, N_FRAMES):
        assert one.track(float(k), host[k][1], float(k), host[k][0]) == many[k]["status"][0]
    nseg, total = int(m["n_segments"][0]), int(m["counts"][0])
    assert same_bits(m["segments"][0, :nseg], m6["segments"][s, :nseg]), f"sequence {s}: records depend on the company"
    final, st = one.read_map(), one.read_map_voxel_stats()
    assert final["n_segments"] == nseg and final["count"] == total and same_bits(final["segments"], m["segments"][0, :nseg])
    assert same_bits(st["sums"], m["sums"][0, :total]) and same_bits(st["obs"], m["obs"][0, :total])
    for min_count, min_span in pairs(MAX_KF):
        want = tr.map_voxel_means(min_count, min_span)
        torch.cuda.synchronize()
        mine = one.map_voxel_means(min_count, min_span)
        assert same_bits(mine["xyz_mean"].view(np.uint32), want["xyz_mean"][0, :total].cpu().numpy().view(np.uint32)), f"{(min_count, min_span)}: the linear walk against the search"
        assert same_bits(mine["gray_mean"], want["gray_mean"][0, :total].cpu().numpy()) and mine["kept"] == int(want["kept"][0])
