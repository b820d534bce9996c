"""The map ICP correction at keyframe promotion (vors_trackers_enable_map_icp, vors_trackers_map_icp, vors_tracker_enable_map_icp,
vors_tracker_read_map_icp). GPU only. Sequences, shapes and helpers are those of tests/test_gpu_trackers_map.py: six
sequences, ten frames, 96x128 coarse-to-fine (120x160 dense), a level-0 map with normals at (2, 0.05).

  1. rejections change nothing            2. the first correction is the composition of public entries, bit for bit
  3. later frames: invariants             4. the other paths (dense REFERENCE, depth filter, last_keyframes = 1, normal_gate = 0)
  5. Tracker(map_icp=...) == sequence 0 of an N = 1 handle     6. refusals     7. trajectory against the truth, recorded, not bounded

MEASURED (MI355X, the run recorded in profiles/trackers_map_icp_summary.md): see that file; nothing here is a bound on accuracy.
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from test_gpu_trackers_map import (BASE, MAX_KF, N_FRAMES, N_SEQ, SHAPES, SPEED, FILTER, config, frames_of, large_capacity, read_map, same_bits)

C2F, DENSE = V.CANDIDATES_COARSE_TO_FINE, V.CANDIDATES_DENSE
NORMALS = (2, 0.05)
# the issue's start; the verdict is wide enough for corrections of the 5 mm class and no wider than a few centimetres
ICP = dict(dist_m=0.05, iters=6, min_cos=0.9, huber_m=0.002, min_match_ratio=0.1, max_rms=0.02, max_trans_m=0.05, max_rot_rad=0.05)
NOTHING = dict(ICP, max_trans_m=0.0, max_rot_rad=0.0)


def handle(mode, arith, icp=None, depth_filter=None, n=N_SEQ):
    rows, cols, _ = SHAPES[mode]
    tr = V.Trackers(config(mode, arith), n, rows, cols)
    if depth_filter is not None:
        tr.enable_depth_filter(*depth_filter)
    tr.enable_map(0, large_capacity(mode), MAX_KF, 0)
    tr.enable_map_normals(*NORMALS)
    if icp is not None:
        tr.enable_map_icp(**icp)
    return tr


def read_icp(tr):
    import torch
    o = tr.map_icp()
    torch.cuda.synchronize()
    return V.decode_map_icp_records(o["records"]).copy(), o["totals"].cpu().numpy().view(np.uint32).copy()


def run(mode, arith, icp=None, depth_filter=None, frames=None, n_frames=N_FRAMES):
    """-> (per frame: poses, status, kf, stats, and with the stage records / totals; the map and its normals after the last frame)"""
    import torch
    frames = frames_of(mode) if frames is None else frames
    tr = handle(mode, arith, icp, depth_filter, n=frames[0][0].shape[0])
    rec = []
    for k in range(n_frames):
        g, d = frames[k]
        tr.init(g, d) if k == 0 else tr.track(g, d)
        poses, status, kf = tr.current_frames()
        r = dict(poses=poses, status=status, kf=kf, stats=tr.stats().copy() if k else None)
        if icp is not None and k:
            r["records"], r["totals"] = read_icp(tr)
        rec.append(r)
    m = read_map(tr)
    m["normals"] = tr.map_normals().cpu().numpy()
    torch.cuda.synchronize()
    return rec, m


@functools.lru_cache(maxsize=None)
def plain_run():
    return run(C2F, V.ARITH_FUSED)


@functools.lru_cache(maxsize=None)
def accepting_run():
    return run(C2F, V.ARITH_FUSED, ICP)


def keyframe_pose_bits(tr):
    """The keyframe pose table of a handle on the host (vors_trackers_state)."""
    import torch
    p = V.C.c_void_p()
    V._check(V.lib().vors_trackers_state(tr._h, None, V.C.byref(p), None, None, None))
    torch.cuda.synchronize()
    return V._device_view(p.value, (tr.n, 7), "<f4", V._torch_device(None)).cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ 1
def test_rejections_change_nothing():
    (bare, bm), (rec, m) = plain_run(), run(C2F, V.ARITH_FUSED, NOTHING)
    promoted = np.zeros(N_SEQ, np.int64)
    accepted = np.zeros(N_SEQ, np.int64)
    for k in range(N_FRAMES):
        for name in ("poses", "status", "kf") + (("stats",) if k else ()):
            assert same_bits(rec[k][name], bare[k][name]), f"frame {k}: {name} moved although every correction was to be rejected"
        if k:
            new = rec[k]["kf"] != rec[k - 1]["kf"]
            promoted += new
            r = rec[k]["records"]
            assert ((r["verdict"] != V.MAP_ICP_NOT_ATTEMPTED) == new).all(), f"frame {k}: attempts {r['verdict']} against promotions {new}"
            ok = r["verdict"] == V.MAP_ICP_ACCEPTED
            assert all(same_bits(r["pose_before"][s], r["pose_after"][s]) for s in np.nonzero(ok)[0]), "accepted at a bound of zero with a step that is not zero"
            accepted += ok
            assert (rec[k]["totals"][:, 0] == promoted).all() and (rec[k]["totals"][:, 1] == accepted).all()
    assert promoted.sum() >= 10 and same_bits(promoted, (np.stack([r["kf"] for r in bare[1:]]) != np.stack([r["kf"] for r in bare[:-1]])).sum(axis=0))
    moved = [(k, s) for k in range(1, N_FRAMES) for s in range(N_SEQ)
             if rec[k]["records"][s]["verdict"] != V.MAP_ICP_NOT_ATTEMPTED and not same_bits(rec[k]["records"][s]["pose_before"], rec[k]["records"][s]["pose_after"])]
    assert moved, "no attempted correction moved the pose: the bound of zero was never tested"
    for k, s in moved:
        assert rec[k]["records"][s]["verdict"] == V.MAP_ICP_STEP or rec[k]["records"][s]["verdict"] in (V.MAP_ICP_FEW_MATCHES, V.MAP_ICP_RMS, V.MAP_ICP_ICP_STATUS)
    for name in ("counts", "n_segments"):
        assert same_bits(m[name], bm[name]), f"the map's {name} moved"
    for s in range(N_SEQ):
        # the WRITTEN entries of every list (what lies past the totals is not data: read_map)
        k = min(int(bm["counts"][s]), m["xyz"].shape[1])
        for name in ("xyz", "pixel", "gray", "normals"):
            assert same_bits(m[name][s, :k], bm[name][s, :k]), f"sequence {s}: the map's {name} moved"
        k = int(bm["n_segments"][s])
        assert same_bits(m["segments"][s, :k], bm["segments"][s, :k])


# ------------------------------------------------------------------------------------------------------------ 2
def first_correction(mode, arith, icp, depth_filter=None, need_accepted=True):
    """The first frame in which a sequence promotes, against a twin handle without the stage and the public entries."""
    import torch
    rows, cols, _ = SHAPES[mode]
    frames, cap = frames_of(mode), large_capacity(mode)
    cam5 = np.array(V.scaled_intrinsics(rows, cols), np.float32)
    twin, on = handle(mode, arith, None, depth_filter), handle(mode, arith, icp, depth_filter)
    for k in range(N_FRAMES):
        g, d = frames[k]
        if k == 0:
            twin.init(g, d), on.init(g, d)
            continue
        before = read_map(twin)
        before_t = (twin.map()["xyz"], twin.map_normals(), twin.map()["counts"])
        twin.track(g, d), on.track(g, d)
        t_poses, t_status, t_kf = twin.current_frames()
        o_poses, o_status, o_kf = on.current_frames()
        assert same_bits(t_kf, o_kf) and same_bits(t_status, o_status)
        rec, totals = read_icp(on)
        new = np.nonzero(t_kf == k)[0]
        if len(new) == 0:
            assert same_bits(t_poses, o_poses) and (rec["verdict"] == V.MAP_ICP_NOT_ATTEMPTED).all() and (totals == 0).all()
            continue
        break
    else:
        pytest.fail("no sequence promoted in ten frames")
    # (the promotion pattern of these sequences puts it in frame 2 for three sequences: tests/test_gpu_trackers_map.py)
    assert k >= 1 and 1 <= len(new) < N_SEQ, f"frame {k}: promoted {new}: the run must hold promoted and not promoted sequences"
    # the depth plane the stage ran on: the frame, or with the filter the fused plane (what keyframe_depth() shows after the call)
    depth = on.keyframe_depth()[0] if depth_filter is not None else frames[k][1]
    ranges = np.zeros((N_SEQ, 2), np.uint32)
    for s in new:
        ranges[s] = V.map_icp_window_host(before["segments"][s], int(before["n_segments"][s]), MAX_KF, int(before["counts"][s]), cap, icp.get("last_keyframes", 0))
        assert ranges[s, 1] > 0
    gate = icp.get("normal_gate", 1)
    fn = V.depth_normals(depth, cam5, V.DEPTH_SCALE, *NORMALS)["normals"] if gate else None
    start = torch.from_numpy(np.ascontiguousarray(t_poses)).cuda()
    ref = V.icp_points_robust(before_t[0], before_t[1], before_t[2], depth, cam5, V.DEPTH_SCALE, start, icp["dist_m"], damping=0.0, step_eps=1e-5,
                              iters=icp["iters"], min_points=6, frame_normals=fn, min_cos=icp["min_cos"], huber_m=icp["huber_m"],
                              ranges=torch.from_numpy(ranges.view(np.int32)).cuda(), gate_counts=True)
    torch.cuda.synchronize()
    ref_pose, ref_stats = ref["poses"].cpu().numpy(), V.decode_icp_stats(ref["stats"])
    ref_gates = ref["gate_counts"].cpu().numpy().view(np.uint32)
    on_kf_pose, on_map = keyframe_pose_bits(on), read_map(on)
    verdicts = []
    for s in range(N_SEQ):
        r = rec[s]
        where = f"frame {k} sequence {s}"
        if s not in new:
            assert r["verdict"] == V.MAP_ICP_NOT_ATTEMPTED and (totals[s] == 0).all(), where
            assert same_bits(o_poses[s], t_poses[s]), f"{where}: not promoted, but its pose moved"
            continue
        assert r["frame"] == k and same_bits(r["pose_before"], t_poses[s]), f"{where}: pose_before is not the twin's pose"
        assert (r["range_first"], r["range_count"]) == tuple(ranges[s]), f"{where}: window {r['range_first'], r['range_count']} against {ranges[s]}"
        assert same_bits(r["pose_after"], ref_pose[s]), f"{where}: pose_after differs from icp_points_robust"
        assert r["stats"].tobytes() == ref_stats[s].tobytes(), f"{where}: stats {r['stats']} against {ref_stats[s]}"
        assert same_bits(r["gate_counts"], ref_gates[s]), f"{where}: gate counts"
        want = V.map_icp_verdict_host(icp, ref_stats[s], t_poses[s], ref_pose[s])
        assert r["verdict"] == want, f"{where}: verdict {r['verdict']} against the host twin's {want}"
        verdicts.append(int(want))
        assert totals[s, 0] == 1 and totals[s, 1] == (want == V.MAP_ICP_ACCEPTED)
        reported = r["pose_after"] if want == V.MAP_ICP_ACCEPTED else t_poses[s]
        assert same_bits(o_poses[s], reported) and same_bits(on_kf_pose[s], reported), f"{where}: the pose reported is not the {'corrected' if want == 1 else 'twin'}'s"
        seg = on_map["segments"][s, int(on_map["n_segments"][s]) - 1]
        assert seg["frame"] == k and same_bits(seg["pose7"], reported), f"{where}: the new segment was not emitted at the pose reported"
    print(f"\nfirst correction ({mode=}, {arith=}, filter={depth_filter is not None}, {icp}): frame {k}, sequences {list(new)}, verdicts {verdicts}")
    for s in new:
        print(f"   seq {s}: window {tuple(ranges[s])} stats {rec[s]['stats']} gates {rec[s]['gate_counts']}"
              f" |dt| = {np.linalg.norm(rec[s]['pose_after'][:3] - rec[s]['pose_before'][:3]):.3g} m")
    # the segment appended in that call against a shadow batch at the pose reported (the check of tests/test_gpu_trackers_map.py)
    shadow = V.Batch(config(mode, arith), len(new), rows, cols)
    shadow.prepare_keyframes(frames[k][0][new].contiguous(), depth[new].contiguous())
    out = shadow.point_cloud(0, poses=torch.from_numpy(np.ascontiguousarray(o_poses[new])).cuda(), capacity=cap, gray=True)
    torch.cuda.synchronize()
    for i, s in enumerate(new):
        seg = on_map["segments"][s, int(on_map["n_segments"][s]) - 1]
        a, count = int(seg["first"]), int(out["counts"][i])
        assert seg["count"] == count and count > 0
        assert same_bits(on_map["xyz"][s, a:a + count], out["xyz"][i, :count].cpu().numpy()), f"sequence {s}: the new cloud is not the back-projection at the pose reported"
    assert len(verdicts) >= 1, "no correction was attempted"
    if need_accepted:
        assert V.MAP_ICP_ACCEPTED in verdicts, f"no correction was accepted in this run: {verdicts}"
    return verdicts


def test_first_correction_is_the_composition_of_public_entries():
    first_correction(C2F, V.ARITH_FUSED, ICP)


# ------------------------------------------------------------------------------------------------------------ 3
def test_later_frames_invariants():
    rec, m = accepting_run()
    attempted, accepted = np.zeros(N_SEQ, np.int64), np.zeros(N_SEQ, np.int64)
    for k in range(1, N_FRAMES):
        r, new = rec[k]["records"], rec[k]["kf"] != rec[k - 1]["kf"]
        assert np.isfinite(rec[k]["poses"]).all()
        assert ((r["verdict"] != V.MAP_ICP_NOT_ATTEMPTED) == new).all()
        for s in np.nonzero(new)[0]:
            assert r[s]["frame"] == k
            if r[s]["verdict"] == V.MAP_ICP_ACCEPTED:
                assert same_bits(rec[k]["poses"][s], r[s]["pose_after"]), f"frame {k} sequence {s}: accepted, but another pose is reported"
                seg = m["segments"][s]
                j = int(np.nonzero(seg["frame"][:int(m["n_segments"][s])] == k)[0][0])
                assert same_bits(seg[j]["pose7"], r[s]["pose_after"]), f"frame {k} sequence {s}: the segment's pose is not the accepted one"
            else:
                assert same_bits(rec[k]["poses"][s], r[s]["pose_before"])
        attempted += new
        accepted += r["verdict"] == V.MAP_ICP_ACCEPTED
        assert (rec[k]["totals"][:, 0] == attempted).all() and (rec[k]["totals"][:, 1] == accepted).all()
    assert attempted.sum() >= 10 and accepted.sum() >= 1
    assert np.isfinite(m["xyz"][0, :int(m["counts"][0])]).all()


# ------------------------------------------------------------------------------------------------------------ 4
def test_dense_reference():
    first_correction(DENSE, V.ARITH_REFERENCE, ICP, need_accepted=False)


def test_depth_filter_fused_plane():
    first_correction(C2F, V.ARITH_FUSED, ICP, depth_filter=FILTER, need_accepted=False)


def test_last_keyframes_1_and_no_normal_gate():
    first_correction(C2F, V.ARITH_FUSED, dict(ICP, normal_gate=0), need_accepted=False)
    # last_keyframes = 1 differs from the whole map from the second promotion of a sequence on: the window starts at its last segment
    rec, m = run(C2F, V.ARITH_FUSED, dict(ICP, last_keyframes=1))
    seen = 0
    for k in range(1, N_FRAMES):
        for s in np.nonzero(rec[k]["kf"] != rec[k - 1]["kf"])[0]:
            r, seg, nseg = rec[k]["records"][s], m["segments"][s], int(m["n_segments"][s])
            j = int(np.nonzero(seg["frame"][:nseg] == k)[0][0])   # the keyframe this call appended: the map before it held j keyframes
            assert j >= 1 and (r["range_first"], r["range_count"]) == (seg[j - 1]["first"], seg[j - 1]["count"]), f"frame {k} sequence {s}: window"
            assert r["stats"]["considered"] == seg[j - 1]["count"]
            seen += j >= 2
    assert seen >= 1, "no sequence promoted twice: last_keyframes = 1 never differed from the whole map"


# ------------------------------------------------------------------------------------------------------------ 5
def test_single_tracker_equals_one_sequence_handle():
    mode, arith, s = C2F, V.ARITH_FUSED, 4
    frames = frames_of(mode)
    one_seq = [(g[[s]].contiguous(), d[[s]].contiguous()) for g, d in frames]
    many, m = run(mode, arith, ICP, frames=one_seq)
    host = [(g[s].cpu().numpy(), d[s].cpu().numpy().view(np.uint16)) for g, d in frames]
    one = V.Tracker(config(mode, arith), 0.0, host[0][1], 0.0, host[0][0], map=(0, large_capacity(mode), MAX_KF, 0), map_normals=NORMALS, map_icp=ICP)
    attempted = 0
    for k in range(1, N_FRAMES):
        assert one.track(float(k), host[k][1], float(k), host[k][0]) == many[k]["status"][0]
        got = one.read_map_icp()
        assert got["record"].tobytes() == many[k]["records"][0].tobytes(), f"frame {k}: record {got['record']} against {many[k]['records'][0]}"
        assert same_bits(got["totals"], many[k]["totals"][0])
        assert same_bits(one.current_frame()[1], many[k]["poses"][0]), f"frame {k}: the pose returned is not the handle's (corrected) pose"
        if got["record"]["verdict"] == V.MAP_ICP_ACCEPTED:
            assert same_bits(one.current_frame()[1], got["record"]["pose_after"]) and same_bits(one.keyframe()[1], got["record"]["pose_after"])
        attempted += got["record"]["verdict"] != V.MAP_ICP_NOT_ATTEMPTED
    assert attempted >= 3
    final = one.read_map()
    assert final["count"] == m["counts"][0] and same_bits(final["xyz"], m["xyz"][0, :final["count"]])
    with pytest.raises(V.VorsError, match="enable_map_icp: the correction is already enabled"):
        V._check(V.lib().vors_tracker_enable_map_icp(one._h, V.C.byref(V.map_icp_params(**ICP))))


# ------------------------------------------------------------------------------------------------------------ 6
def test_refusals():
    mode = C2F
    rows, cols, _ = SHAPES[mode]
    cfg, frames = config(mode, V.ARITH_FUSED), frames_of(mode)

    def refused(tr, sentence, **kw):
        before = tr.workspace_bytes()
        with pytest.raises(V.VorsError) as e:
            tr.enable_map_icp(**dict(ICP, **kw))
        assert str(e.value).endswith(sentence), str(e.value)
        assert tr.workspace_bytes() == before   # a refused call allocates nothing

    t = V.Trackers(cfg, N_SEQ, rows, cols)
    refused(t, "enable_map_icp: needs an enabled keyframe map first (vors_trackers_enable_map)")
    with pytest.raises(V.VorsError, match="map_icp: the ICP correction is not enabled"):
        t.map_icp()
    t.enable_map(0, 5000, 4, 0)
    refused(t, "enable_map_icp: needs the normals of the map first (vors_trackers_enable_map_normals)")
    t.enable_map_normals(*NORMALS)
    nan = float("nan")
    for kw, sentence in ((dict(dist_m=-1.0), "enable_map_icp: dist_m must be >= 0 (and not NaN)"), (dict(dist_m=nan), "enable_map_icp: dist_m must be >= 0 (and not NaN)"),
                         (dict(damping=-1.0), "enable_map_icp: damping must be >= 0 (and not NaN)"),
                         (dict(step_eps=nan), "enable_map_icp: step_eps must be >= 0 (and not NaN)"),
                         (dict(iters=65), "enable_map_icp: iters must be in 0..64"), (dict(iters=-1), "enable_map_icp: iters must be in 0..64"),
                         (dict(min_points=5), "enable_map_icp: min_points must be >= 6 (a pose has six degrees of freedom)"),
                         (dict(min_cos=1.5), "enable_map_icp: min_cos must lie in [-1, 1] (and not be NaN)"),
                         (dict(huber_m=-0.1), "enable_map_icp: huber_m must be >= 0 (and not NaN; 0 = no Huber weight)"),
                         (dict(last_keyframes=-1), "enable_map_icp: last_keyframes must be >= 0 (0 = the whole map)"),
                         (dict(min_match_ratio=1.5), "enable_map_icp: min_match_ratio must lie in [0, 1] (and not be NaN)"),
                         (dict(min_match_ratio=nan), "enable_map_icp: min_match_ratio must lie in [0, 1] (and not be NaN)"),
                         (dict(max_rms=-1.0), "enable_map_icp: max_rms must be >= 0 (and not NaN)"),
                         (dict(max_trans_m=nan), "enable_map_icp: max_trans_m must be >= 0 (and not NaN)"),
                         (dict(max_rot_rad=-1.0), "enable_map_icp: max_rot_rad must be >= 0 (and not NaN)")):
        refused(t, sentence, **kw)
    assert V.lib().vors_trackers_enable_map_icp(t._h, None) == -1 and V.lib().vors_last_error() == b"enable_map_icp: params is NULL"
    before = t.workspace_bytes()
    t.enable_map_icp(**ICP)
    S, cap = rows * cols, 5000
    per_seq = 8 + 4 + 56 + 24 + 16 + 112 + 8
    assert t.workspace_bytes() == before + V.icp_workspace_bytes(N_SEQ, cap) + N_SEQ * per_seq + N_SEQ * S * 12
    refused(t, "enable_map_icp: the correction is already enabled")
    late = V.Trackers(cfg, N_SEQ, rows, cols)
    late.enable_map(0, cap, 4, 0)
    late.enable_map_normals(*NORMALS)
    late.init(*frames[0])
    refused(late, "enable_map_icp: legal only before vors_trackers_init")
    gateless = V.Trackers(cfg, N_SEQ, rows, cols)
    gateless.enable_map(0, cap, 4, 0)
    gateless.enable_map_normals(*NORMALS)
    before = gateless.workspace_bytes()
    gateless.enable_map_icp(**dict(ICP, normal_gate=0))
    assert gateless.workspace_bytes() == before + V.icp_workspace_bytes(N_SEQ, cap) + N_SEQ * per_seq   # no frame normals are kept
    # the stage's records start at zero and a second init zeroes them again
    t.init(*frames[0])
    rec, totals = read_icp(t)
    assert (rec["verdict"] == V.MAP_ICP_NOT_ATTEMPTED).all() and (totals == 0).all()
    for k in range(1, 4):
        t.track(*frames[k])
    assert read_icp(t)[1][:, 0].sum() >= 3
    t.init(*frames[0])
    assert (read_icp(t)[1] == 0).all()
    host = (frames[0][0][0].cpu().numpy(), frames[0][1][0].cpu().numpy().view(np.uint16))
    with pytest.raises(V.VorsError, match="map_icp: the correction needs the map's normals"):
        V.Tracker(cfg, 0.0, host[1], 0.0, host[0], map=(0, cap, 4, 0), map_icp=0.05)
    one = V.Tracker(cfg, 0.0, host[1], 0.0, host[0], map=(0, cap, 4, 0), map_normals=NORMALS)
    with pytest.raises(V.VorsError, match="read_map_icp: the correction is not enabled"):
        one.read_map_icp()
    one.track(1.0, host[1], 1.0, host[0])
    with pytest.raises(V.VorsError) as e:
        V._check(V.lib().vors_tracker_enable_map_icp(one._h, V.C.byref(V.map_icp_params(**ICP))))
    assert str(e.value).endswith("enable_map_icp: legal only before the first vors_tracker_track")


# ------------------------------------------------------------------------------------------------------------ 7
def pose_error(pose, truth):
    """(translation distance, rotation angle) between two camera -> world poses"""
    d = V.iso_mul(V.iso_inverse(truth.astype(np.float32)), pose.astype(np.float32))
    return float(np.linalg.norm(d[:3])), float(2.0 * np.arccos(min(1.0, abs(float(d[6])))))


def test_trajectory_against_the_truth_recorded():
    """Recorded, not bounded (nobody has measured these): the final pose of every sequence against the twists the scenes were rendered
    from, with the stage off and on, and every accepted record's pose before and after. The figures of the recorded run are in
    profiles/trackers_map_icp_summary.md; the run itself prints them and writes them where VORS_MAP_ICP_SUMMARY points."""
    (off, _), (on, _) = plain_run(), accepting_run()
    truth = [[V.iso_inverse(V.se3_exp((BASE * SPEED[s] * k).astype(np.float32))) for s in range(N_SEQ)] for k in range(N_FRAMES)]
    lines = ["| sequence | off: dt [mm] | off: angle [mrad] | on: dt [mm] | on: angle [mrad] | attempted | accepted |", "|---|---|---|---|---|---|---|"]
    for s in range(N_SEQ):
        a, b = pose_error(off[-1]["poses"][s], truth[-1][s]), pose_error(on[-1]["poses"][s], truth[-1][s])
        lines.append(f"| {s} | {1e3 * a[0]:.3f} | {1e3 * a[1]:.3f} | {1e3 * b[0]:.3f} | {1e3 * b[1]:.3f} | {on[-1]['totals'][s, 0]} | {on[-1]['totals'][s, 1]} |")
    lines += ["", "| frame | sequence | before: dt [mm] | before: angle [mrad] | after: dt [mm] | after: angle [mrad] | matched / considered | rms [mm] |",
              "|---|---|---|---|---|---|---|---|"]
    worse = 0
    for k in range(1, N_FRAMES):
        for s in range(N_SEQ):
            r = on[k]["records"][s]
            if r["verdict"] != V.MAP_ICP_ACCEPTED:
                continue
            a, b = pose_error(r["pose_before"], truth[k][s]), pose_error(r["pose_after"], truth[k][s])
            worse += b[0] > a[0]
            lines.append(f"| {k} | {s} | {1e3 * a[0]:.3f} | {1e3 * a[1]:.3f} | {1e3 * b[0]:.3f} | {1e3 * b[1]:.3f} | {r['stats']['matched']} / {r['stats']['considered']}"
                         f" | {1e3 * r['stats']['rms']:.3f} |")
    lines.append(f"\naccepted records whose translation error grew: {worse}")
    text = "\n".join(lines)
    print("\n" + text)
    path = os.environ.get("VORS_MAP_ICP_SUMMARY")
    if path:
        with open(path, "w") as f:
            f.write(text + "\n")
    assert all(np.isfinite(r["poses"]).all() for r in on)
