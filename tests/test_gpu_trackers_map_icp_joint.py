"""The map ICP correction through the joint pass with the condition test (vors_icp_condition, vors_trackers_enable_map_icp_joint,
vors_trackers_map_icp_joint, vors_tracker_enable_map_icp_joint, vors_tracker_read_map_icp_joint). GPU only. Sequences,
shapes, parameters and helpers are those of tests/test_gpu_trackers_map_icp.py: six sequences, ten frames, 96x128 coarse-to-fine
(120x160 dense), a level-0 map with normals at (2, 0.05), its ICP parameters.

  1. vors_icp_condition == the host, bit for bit     2. photo_scale_m = 0, both bounds 0 == vors_trackers_enable_map_icp, bit for bit
  3. the first correction is the composition of public entries, both records bit for bit (FUSED, depth filter, dense REFERENCE)
  4. CONDITION rejects and changes nothing           5. Tracker(map_icp_joint=...) == sequence 0 of an N = 1 handle
  6. refusals, exclusivity with the plain enable     7. the workspace figure     8. trajectory against the truth, recorded, not bounded

BOUNDS are tests/test_map_icp_condition_host.py's (80, 70 1/m): chosen there, on the host scenes, between a constrained system and one
that slides; nothing here tunes them. SMALL = 1.0 is below every dilution_t of a pass without photometric rows: its H_tt is a sum of n
matrices n n^T of unit normals under weights <= 1, so H_tt <= n I, C_tt >= H_tt^-1 >= I / n and dilution_t >= sqrt(3).

MEASURED (MI355X, the run recorded in profiles/trackers_map_icp_joint_summary.md): see that file; nothing here is a bound on accuracy.
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from test_gpu_trackers_map import (BASE, MAX_KF, N_FRAMES, N_SEQ, SHAPES, SPEED, FILTER, config, frames_of, large_capacity, read_map, same_bits)
from test_gpu_trackers_map_icp import C2F, DENSE, ICP, NORMALS, accepting_run, handle, keyframe_pose_bits, plain_run, pose_error, read_icp
from test_map_icp_condition_host import BOUNDS

PHOTO = dict(photo_scale_m=0.0005, photo_huber_grey=10.0)   # tests/test_icp_joint_host.py's PHOTO_SCALE_M and PHOTO_HUBER_GREY
NEUTRAL = dict(ICP)                                         # photo_scale_m = 0, both bounds 0
JOINT = dict(ICP, **PHOTO)
SMALL = 1.0                                                 # (the docstring)


def handle_j(mode, arith, joint, depth_filter=None, n=N_SEQ):
    tr = handle(mode, arith, None, depth_filter, n)
    tr.enable_map_icp_joint(**joint)
    return tr


def read_joint(tr):
    import torch
    o = tr.map_icp_joint()
    torch.cuda.synchronize()
    return V.decode_map_icp_joint_records(o).copy()


def run_j(mode, arith, joint, depth_filter=None, frames=None, n_frames=N_FRAMES):
    """test_gpu_trackers_map_icp.run() for a handle with the joint stage: per frame also the joint records."""
    import torch
    frames = frames_of(mode) if frames is None else frames
    tr = handle_j(mode, arith, joint, depth_filter, n=frames[0][0].shape[0])
    rec = []
    for k in range(n_frames):
        g, d = frames[k]
        tr.init(g, d) if k == 0 else tr.track(g, d)
        poses, status, kf = tr.current_frames()
        r = dict(poses=poses, status=status, kf=kf, stats=tr.stats().copy() if k else None)
        if k:
            r["records"], r["totals"] = read_icp(tr)
            r["joint"] = read_joint(tr)
        rec.append(r)
    m = read_map(tr)
    m["normals"] = tr.map_normals().cpu().numpy()
    torch.cuda.synchronize()
    return rec, m


@functools.lru_cache(maxsize=None)
def neutral_run():
    return run_j(C2F, V.ARITH_FUSED, NEUTRAL)


def same_map(m, bm):
    """The totals, and of every list and of the segment records the WRITTEN entries (what lies past the totals is not data: read_map)."""
    for name in ("counts", "n_segments"):
        assert same_bits(m[name], bm[name]), f"the map's {name} differs"
    for s in range(len(bm["n_segments"])):
        k = min(int(bm["counts"][s]), m["xyz"].shape[1])
        for name in ("xyz", "pixel", "gray", "normals"):
            assert same_bits(m[name][s, :k], bm[name][s, :k]), f"sequence {s}: the map's {name} differs"
        k = int(bm["n_segments"][s])
        assert same_bits(m["segments"][s, :k], bm["segments"][s, :k])


# ------------------------------------------------------------------------------------------------------------ 1
def condition_rows(n, seed):
    """[n, 29] sums mixing, row after row: a good system, too few points (count 6), a singular H (five rows, up to the rounding of its
    entries; every other time the zero matrix), NaN entries."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 29), np.float32)
    for i in range(n):
        rows = 5 if i % 4 == 2 else 40
        j = rng.normal(size=(rows, 6)) * np.array([1, 1, 1, 0.3, 0.3, 0.3])
        h = (j.T @ j).astype(np.float32)
        out[i, 0], out[i, 1] = rng.random(), 6.0 if i % 4 == 1 else float(rows * 50)
        out[i, 2:8] = rng.normal(size=6)
        out[i, 8:] = h[np.triu_indices(6)]
        if i % 8 == 6:
            out[i, 8:] = 0.0
        if i % 4 == 3:
            out[i, 8 + int(rng.integers(21))] = np.nan
    return out


@pytest.mark.parametrize("n", [1, 65])
def test_icp_condition_equals_the_host(n):
    import torch
    batches = [condition_rows(65, 7)] if n == 65 else [condition_rows(8, 11)[[i]] for i in range(8)]   # n = 1: each kind in a call of its own
    seen = set()
    for sums in batches:
        dil, flags = V.icp_condition(torch.from_numpy(sums).cuda())
        torch.cuda.synchronize()
        dil, flags = dil.cpu().numpy(), flags.cpu().numpy()
        for i in range(len(sums)):
            dt, dr, fl = V.icp_condition_from_sums(sums[i])
            assert flags[i] == fl, f"row {i}: flags {flags[i]} against the host's {fl}"
            assert same_bits(dil[i], np.array([dt, dr], np.float32)), f"row {i}: {dil[i]} against the host's {(dt, dr)}"
            assert np.isnan(dil[i]).all() if fl else np.isfinite(dil[i]).all()
            seen.add(int(fl))
    assert {0, 1, 2} <= seen, f"the batch held flags {seen} only"


# ------------------------------------------------------------------------------------------------------------ 2
def test_neutral_case_is_the_plain_stage():
    (plain, pm), (rec, m) = accepting_run(), neutral_run()
    attempted = 0
    for k in range(N_FRAMES):
        for name in ("poses", "status", "kf") + (("stats", "records", "totals") if k else ()):
            assert same_bits(rec[k][name], plain[k][name]), f"frame {k}: {name} differs from the handle with vors_trackers_enable_map_icp"
        if k:
            new = rec[k]["records"]["verdict"] != V.MAP_ICP_NOT_ATTEMPTED
            j = rec[k]["joint"]
            assert (j["photo_counts"] == 0).all()
            assert (j[~new].view(np.uint8).reshape(-1, 20) == 0).all(), f"frame {k}: a joint record of a sequence that was not promoted is not zeros"
            for s in np.nonzero(new)[0]:
                ok = rec[k]["records"][s]["stats"]["matched"] > 6
                assert (j[s]["condition_flags"] & 1) == (0 if ok else 1)
                assert np.isfinite(j[s]["dilution_t"]) == (j[s]["condition_flags"] == 0)
            attempted += int(new.sum())
    assert attempted >= 10
    same_map(m, pm)


def test_neutral_dilutions_in_every_frame_from_the_public_robust_entry():
    """Every promotion of the ten-frame neutral run, not only the first: the map as it stood before the track call, the record's own
    window and pose_before, vors_depth_normals of the frame and the device's vors_icp_points_robust give the record's pose_after and
    statistics again, bit for bit, and vors_icp_condition of THAT pass's sums29 gives the joint record's dilutions and flags."""
    import torch
    mode, arith = C2F, V.ARITH_FUSED
    rows, cols, _ = SHAPES[mode]
    frames = frames_of(mode)
    cam5 = np.array(V.scaled_intrinsics(rows, cols), np.float32)
    tr = handle_j(mode, arith, NEUTRAL)
    pinned = 0
    for k in range(N_FRAMES):
        g, d = frames[k]
        if k == 0:
            tr.init(g, d)
            continue
        before = tr.map()
        before_normals = tr.map_normals()
        tr.track(g, d)
        rec, _ = read_icp(tr)
        jrec = read_joint(tr)
        new = np.nonzero(rec["verdict"] != V.MAP_ICP_NOT_ATTEMPTED)[0]
        if len(new) == 0:
            continue
        ranges = np.stack([rec["range_first"], rec["range_count"]], -1).astype(np.uint32)
        fn = V.depth_normals(d, cam5, V.DEPTH_SCALE, *NORMALS)["normals"]
        ref = V.icp_points_robust(before["xyz"], before_normals, before["counts"], d, cam5, V.DEPTH_SCALE,
                                  torch.from_numpy(np.ascontiguousarray(rec["pose_before"])).cuda(), ICP["dist_m"], damping=0.0, step_eps=1e-5,
                                  iters=ICP["iters"], min_points=6, frame_normals=fn, min_cos=ICP["min_cos"], huber_m=ICP["huber_m"],
                                  ranges=torch.from_numpy(ranges.view(np.int32)).cuda(), sums29=True)
        dil, flags = V.icp_condition(ref["sums29"])
        torch.cuda.synchronize()
        ref_pose, ref_stats = ref["poses"].cpu().numpy(), V.decode_icp_stats(ref["stats"])
        dil, flags = dil.cpu().numpy(), flags.cpu().numpy()
        for s in new:
            where = f"frame {k} sequence {s}"
            assert same_bits(rec[s]["pose_after"], ref_pose[s]) and rec[s]["stats"].tobytes() == ref_stats[s].tobytes(), f"{where}: not the public pass"
            j = jrec[s]
            assert same_bits(np.array([j["dilution_t"], j["dilution_r"]], np.float32), dil[s]), f"{where}: dilutions {j} against vors_icp_condition's {dil[s]}"
            assert j["condition_flags"] == flags[s], where
            pinned += 1
    assert pinned >= 10, f"only {pinned} promotions were compared"


# ------------------------------------------------------------------------------------------------------------ 3
def first_correction_joint(mode, arith, joint, depth_filter=None):
    """The first frame in which a sequence promotes, against a twin handle without the stage and the public entries -> the dilutions seen."""
    import torch
    rows, cols, _ = SHAPES[mode]
    frames, cap = frames_of(mode), large_capacity(mode)
    cam5 = np.array(V.scaled_intrinsics(rows, cols), np.float32)
    twin, on = handle(mode, arith, None, depth_filter), handle_j(mode, arith, joint, depth_filter)
    for k in range(N_FRAMES):
        g, d = frames[k]
        if k == 0:
            twin.init(g, d), on.init(g, d)
            continue
        before = read_map(twin)
        tm = twin.map()
        before_t = (tm["xyz"], twin.map_normals(), tm["gray"], tm["counts"])
        twin.track(g, d), on.track(g, d)
        t_poses, t_status, t_kf = twin.current_frames()
        o_poses, o_status, o_kf = on.current_frames()
        assert same_bits(t_kf, o_kf) and same_bits(t_status, o_status)
        rec, totals = read_icp(on)
        jrec = read_joint(on)
        new = np.nonzero(t_kf == k)[0]
        if len(new) == 0:
            assert same_bits(t_poses, o_poses) and (rec["verdict"] == V.MAP_ICP_NOT_ATTEMPTED).all() and (totals == 0).all()
            assert (jrec.view(np.uint8) == 0).all()
            continue
        break
    else:
        pytest.fail("no sequence promoted in ten frames")
    assert k >= 1 and 1 <= len(new) < N_SEQ, f"frame {k}: promoted {new}: the run must hold promoted and not promoted sequences"
    depth = on.keyframe_depth()[0] if depth_filter is not None else frames[k][1]
    ranges = np.zeros((N_SEQ, 2), np.uint32)
    for s in new:
        ranges[s] = V.map_icp_window_host(before["segments"][s], int(before["n_segments"][s]), MAX_KF, int(before["counts"][s]), cap, joint.get("last_keyframes", 0))
        assert ranges[s, 1] > 0
    fn = V.depth_normals(depth, cam5, V.DEPTH_SCALE, *NORMALS)["normals"]
    start = torch.from_numpy(np.ascontiguousarray(t_poses)).cuda()
    common = dict(damping=0.0, step_eps=1e-5, iters=joint["iters"], min_points=6, frame_normals=fn, min_cos=joint["min_cos"], huber_m=joint["huber_m"],
                  ranges=torch.from_numpy(ranges.view(np.int32)).cuda(), gate_counts=True, sums29=True)
    scale = joint.get("photo_scale_m", 0.0)
    if scale == 0.0:   # the neutral case: the sums of the public ROBUST entry
        ref = V.icp_points_robust(before_t[0], before_t[1], before_t[3], depth, cam5, V.DEPTH_SCALE, start, joint["dist_m"], **common)
        ref_photo = np.zeros((N_SEQ, 2), np.uint32)
    else:
        ref = V.icp_points_joint(before_t[0], before_t[1], before_t[2], before_t[3], depth, frames[k][0], cam5, V.DEPTH_SCALE, start, joint["dist_m"],
                                 photo_scale_m=scale, photo_huber_grey=joint.get("photo_huber_grey", 0.0), photo_counts=True, **common)
        ref_photo = ref["photo_counts"].cpu().numpy().view(np.uint32)
    dil, flags = V.icp_condition(ref["sums29"])
    torch.cuda.synchronize()
    ref_pose, ref_stats = ref["poses"].cpu().numpy(), V.decode_icp_stats(ref["stats"])
    ref_gates = ref["gate_counts"].cpu().numpy().view(np.uint32)
    dil, flags = dil.cpu().numpy(), flags.cpu().numpy()
    on_kf_pose, on_map = keyframe_pose_bits(on), read_map(on)
    verdicts, seen = [], []
    for s in range(N_SEQ):
        r, j = rec[s], jrec[s]
        where = f"frame {k} sequence {s}"
        if s not in new:
            assert r["verdict"] == V.MAP_ICP_NOT_ATTEMPTED and (totals[s] == 0).all() and j.tobytes() == bytes(20), where
            assert same_bits(o_poses[s], t_poses[s]), f"{where}: not promoted, but its pose moved"
            continue
        assert r["frame"] == k and same_bits(r["pose_before"], t_poses[s]), f"{where}: pose_before is not the twin's pose"
        assert (r["range_first"], r["range_count"]) == tuple(ranges[s]), f"{where}: window"
        assert same_bits(r["pose_after"], ref_pose[s]), f"{where}: pose_after differs from the public pass"
        assert r["stats"].tobytes() == ref_stats[s].tobytes(), f"{where}: stats {r['stats']} against {ref_stats[s]}"
        assert same_bits(r["gate_counts"], ref_gates[s]), f"{where}: gate counts"
        assert same_bits(np.array([j["dilution_t"], j["dilution_r"]], np.float32), dil[s]), f"{where}: dilutions {j} against vors_icp_condition's {dil[s]}"
        assert j["condition_flags"] == flags[s] and same_bits(j["photo_counts"], ref_photo[s]), f"{where}: {j} against flags {flags[s]}, photo counts {ref_photo[s]}"
        if scale > 0.0:
            assert j["photo_counts"][0] > 0, f"{where}: the photometric row was never used"
        want = V.map_icp_verdict_joint_host(joint, ref_stats[s], t_poses[s], ref_pose[s], dil[s, 0], dil[s, 1])
        assert r["verdict"] == want, f"{where}: verdict {r['verdict']} against the host twin's {want}"
        verdicts.append(int(want))
        seen.append((float(dil[s, 0]), float(dil[s, 1])))
        assert totals[s, 0] == 1 and totals[s, 1] == (want == V.MAP_ICP_ACCEPTED)
        reported = r["pose_after"] if want == V.MAP_ICP_ACCEPTED else t_poses[s]
        assert same_bits(o_poses[s], reported) and same_bits(on_kf_pose[s], reported), f"{where}: the pose reported"
        seg = on_map["segments"][s, int(on_map["n_segments"][s]) - 1]
        assert seg["frame"] == k and same_bits(seg["pose7"], reported), f"{where}: the new segment was not emitted at the pose reported"
    print(f"\nfirst joint correction ({mode=}, {arith=}, filter={depth_filter is not None}, photo_scale_m={scale}): frame {k}, sequences {list(new)}, "
          f"verdicts {verdicts}, (dilution_t, dilution_r) {seen}, photo counts {[tuple(jrec[s]['photo_counts']) for s in new]}")
    assert len(verdicts) >= 1
    return seen


def test_first_correction_neutral_dilutions_from_the_public_robust_entry():
    first_correction_joint(C2F, V.ARITH_FUSED, NEUTRAL)


def test_first_correction_is_the_composition_of_public_entries():
    seen = first_correction_joint(C2F, V.ARITH_FUSED, dict(JOINT, **BOUNDS))
    assert all(np.isfinite(t) and np.isfinite(r) for t, r in seen)


def test_first_correction_depth_filter_fused_plane():
    first_correction_joint(C2F, V.ARITH_FUSED, dict(JOINT, **BOUNDS), depth_filter=FILTER)


def test_first_correction_dense_reference_own_gray():
    first_correction_joint(DENSE, V.ARITH_REFERENCE, dict(JOINT, **BOUNDS))


# ------------------------------------------------------------------------------------------------------------ 4
def test_condition_rejects_and_changes_nothing():
    """photo_scale_m = 0 and max_dilution_t = SMALL, below every dilution_t such a pass can have (the docstring), test 3's included; the
    plain gates as wide as they go, so that nothing else rejects. EVERY attempted verdict is CONDITION, nothing is accepted, and every
    pose and the map keep the bits of a run with the stage off."""
    wide = dict(ICP, min_match_ratio=0.0, max_rms=1e3, max_trans_m=1e3, max_rot_rad=3.2)
    joint = dict(wide, max_dilution_t=SMALL)
    (bare, bm), (rec, m) = plain_run(), run_j(C2F, V.ARITH_FUSED, joint)
    promoted = np.zeros(N_SEQ, np.int64)
    for k in range(N_FRAMES):
        for name in ("poses", "status", "kf") + (("stats",) if k else ()):
            assert same_bits(rec[k][name], bare[k][name]), f"frame {k}: {name} moved although every correction was to be rejected"
        if k:
            new = rec[k]["kf"] != rec[k - 1]["kf"]
            promoted += new
            r, j = rec[k]["records"], rec[k]["joint"]
            assert ((r["verdict"] != V.MAP_ICP_NOT_ATTEMPTED) == new).all()
            for s in np.nonzero(new)[0]:
                assert r[s]["verdict"] == V.MAP_ICP_CONDITION, f"frame {k} sequence {s}: verdict {r[s]['verdict']}, stats {r[s]['stats']}, joint record {j[s]}"
                assert V.map_icp_verdict_host(wide, r[s]["stats"], r[s]["pose_before"], r[s]["pose_after"]) == V.MAP_ICP_ACCEPTED
                assert not (j[s]["dilution_t"] <= SMALL), f"frame {k} sequence {s}: dilution_t {j[s]['dilution_t']} under a bound it cannot meet"
            assert (rec[k]["totals"][:, 0] == promoted).all() and (rec[k]["totals"][:, 1] == 0).all()
    assert promoted.sum() >= 10
    same_map(m, bm)


# ------------------------------------------------------------------------------------------------------------ 5
def test_single_tracker_equals_one_sequence_handle():
    mode, arith, s = C2F, V.ARITH_FUSED, 4
    joint = dict(JOINT, **BOUNDS)
    frames = frames_of(mode)
    one_seq = [(g[[s]].contiguous(), d[[s]].contiguous()) for g, d in frames]
    many, m = run_j(mode, arith, joint, frames=one_seq)
    host = [(g[s].cpu().numpy(), d[s].cpu().numpy().view(np.uint16)) for g, d in frames]
    one = V.Tracker(config(mode, arith), 0.0, host[0][1], 0.0, host[0][0], map=(0, large_capacity(mode), MAX_KF, 0), map_normals=NORMALS, map_icp_joint=joint)
    attempted = 0
    for k in range(1, N_FRAMES):
        assert one.track(float(k), host[k][1], float(k), host[k][0]) == many[k]["status"][0]
        got, gj = one.read_map_icp(), one.read_map_icp_joint()
        assert got["record"].tobytes() == many[k]["records"][0].tobytes(), f"frame {k}: record {got['record']} against {many[k]['records'][0]}"
        assert gj.tobytes() == many[k]["joint"][0].tobytes(), f"frame {k}: joint record {gj} against {many[k]['joint'][0]}"
        assert same_bits(got["totals"], many[k]["totals"][0])
        assert same_bits(one.current_frame()[1], many[k]["poses"][0]), f"frame {k}: the pose returned is not the handle's (corrected) pose"
        if got["record"]["verdict"] == V.MAP_ICP_ACCEPTED:
            assert same_bits(one.current_frame()[1], got["record"]["pose_after"]) and same_bits(one.keyframe()[1], got["record"]["pose_after"])
        attempted += got["record"]["verdict"] != V.MAP_ICP_NOT_ATTEMPTED
    assert attempted >= 3
    final = one.read_map()
    assert final["count"] == m["counts"][0] and same_bits(final["xyz"], m["xyz"][0, :final["count"]])
    for call, p in ((V.lib().vors_tracker_enable_map_icp_joint, V.map_icp_joint_params(**joint)), (V.lib().vors_tracker_enable_map_icp, V.map_icp_params(**ICP))):
        with pytest.raises(V.VorsError, match="the correction is already enabled"):
            V._check(call(one._h, V.C.byref(p)))


# ------------------------------------------------------------------------------------------------------------ 6 and 7
def test_refusals_and_the_workspace_figure():
    mode = C2F
    rows, cols, _ = SHAPES[mode]
    cfg, frames = config(mode, V.ARITH_FUSED), frames_of(mode)

    def refused(tr, sentence, **kw):
        before = tr.workspace_bytes()
        with pytest.raises(V.VorsError) as e:
            tr.enable_map_icp_joint(**dict(JOINT, **kw))
        assert str(e.value).endswith(sentence), str(e.value)
        assert tr.workspace_bytes() == before   # a refused call allocates nothing

    t = V.Trackers(cfg, N_SEQ, rows, cols)
    refused(t, "enable_map_icp_joint: needs an enabled keyframe map first (vors_trackers_enable_map)")
    cap = 5000
    t.enable_map(0, cap, 4, 0)
    refused(t, "enable_map_icp_joint: needs the normals of the map first (vors_trackers_enable_map_normals)")
    t.enable_map_normals(*NORMALS)
    with pytest.raises(V.VorsError, match="map_icp_joint: the joint ICP correction is not enabled"):
        t.map_icp_joint()
    nan = float("nan")
    for kw, sentence in ((dict(dist_m=-1.0), "enable_map_icp_joint: dist_m must be >= 0 (and not NaN)"),
                         (dict(iters=65), "enable_map_icp_joint: iters must be in 0..64"),
                         (dict(min_points=5), "enable_map_icp_joint: min_points must be >= 6 (a pose has six degrees of freedom)"),
                         (dict(min_cos=1.5), "enable_map_icp_joint: min_cos must lie in [-1, 1] (and not be NaN)"),
                         (dict(last_keyframes=-1), "enable_map_icp_joint: last_keyframes must be >= 0 (0 = the whole map)"),
                         (dict(max_rms=-1.0), "enable_map_icp_joint: max_rms must be >= 0 (and not NaN)"),
                         (dict(photo_scale_m=-1.0), "enable_map_icp_joint: photo_scale_m must be >= 0 (and not NaN; 0 = no photometric term)"),
                         (dict(photo_scale_m=nan), "enable_map_icp_joint: photo_scale_m must be >= 0 (and not NaN; 0 = no photometric term)"),
                         (dict(photo_huber_grey=-2.0), "enable_map_icp_joint: photo_huber_grey must be >= 0 (and not NaN; 0 = no Huber weight)"),
                         (dict(photo_huber_grey=nan), "enable_map_icp_joint: photo_huber_grey must be >= 0 (and not NaN; 0 = no Huber weight)"),
                         (dict(max_dilution_t=-1.0), "enable_map_icp_joint: max_dilution_t must be >= 0 (and not NaN; 0 = that bound is off)"),
                         (dict(max_dilution_t=nan), "enable_map_icp_joint: max_dilution_t must be >= 0 (and not NaN; 0 = that bound is off)"),
                         (dict(max_dilution_r=-1.0), "enable_map_icp_joint: max_dilution_r must be >= 0 (and not NaN; 0 = that bound is off)"),
                         (dict(max_dilution_r=nan), "enable_map_icp_joint: max_dilution_r must be >= 0 (and not NaN; 0 = that bound is off)")):
        refused(t, sentence, **kw)
    assert V.lib().vors_trackers_enable_map_icp_joint(t._h, None) == -1 and V.lib().vors_last_error() == b"enable_map_icp_joint: params is NULL"
    # 7: the plain stage's figure (tests/test_gpu_trackers_map_icp.py) and per sequence 116 bytes of sums, 8 of photo counts, 20 of joint record
    before = t.workspace_bytes()
    t.enable_map_icp_joint(**dict(JOINT, **BOUNDS))
    S = rows * cols
    per_seq = 8 + 4 + 56 + 24 + 16 + 112 + 8
    assert t.workspace_bytes() == before + V.icp_workspace_bytes(N_SEQ, cap) + N_SEQ * (per_seq + 116 + 8 + 20) + N_SEQ * S * 12
    # exclusivity: either enable after the other is refused
    refused(t, "enable_map_icp_joint: the correction is already enabled")
    with pytest.raises(V.VorsError) as e:
        t.enable_map_icp(**ICP)
    assert str(e.value).endswith("enable_map_icp: the correction is already enabled")
    t.map_icp(), t.map_icp_joint()   # both readers work on the joint handle
    plain = V.Trackers(cfg, N_SEQ, rows, cols)
    plain.enable_map(0, cap, 4, 0)
    plain.enable_map_normals(*NORMALS)
    plain.enable_map_icp(**ICP)
    refused(plain, "enable_map_icp_joint: the correction is already enabled")
    with pytest.raises(V.VorsError, match="map_icp_joint: the joint ICP correction is not enabled"):
        plain.map_icp_joint()
    late = V.Trackers(cfg, N_SEQ, rows, cols)
    late.enable_map(0, cap, 4, 0)
    late.enable_map_normals(*NORMALS)
    late.init(*frames[0])
    refused(late, "enable_map_icp_joint: legal only before vors_trackers_init")
    gateless = V.Trackers(cfg, N_SEQ, rows, cols)
    gateless.enable_map(0, cap, 4, 0)
    gateless.enable_map_normals(*NORMALS)
    before = gateless.workspace_bytes()
    gateless.enable_map_icp_joint(**dict(JOINT, normal_gate=0))
    assert gateless.workspace_bytes() == before + V.icp_workspace_bytes(N_SEQ, cap) + N_SEQ * (per_seq + 116 + 8 + 20)
    # records start at zero, and a second init zeroes them again; no later call allocates
    t.init(*frames[0])
    assert (read_joint(t).view(np.uint8) == 0).all() and (read_icp(t)[1] == 0).all()
    ws, written = t.workspace_bytes(), False
    for k in range(1, 4):
        t.track(*frames[k])
        written |= bool((read_joint(t).view(np.uint8) != 0).any())
    assert read_icp(t)[1][:, 0].sum() >= 3 and written and t.workspace_bytes() == ws
    t.init(*frames[0])
    assert (read_joint(t).view(np.uint8) == 0).all() and (read_icp(t)[1] == 0).all()
    host = (frames[0][0][0].cpu().numpy(), frames[0][1][0].cpu().numpy().view(np.uint16))
    with pytest.raises(V.VorsError, match="map_icp_joint: the correction needs the map's normals"):
        V.Tracker(cfg, 0.0, host[1], 0.0, host[0], map=(0, cap, 4, 0), map_icp_joint=JOINT)
    with pytest.raises(V.VorsError, match="map_icp_joint: the joint stage stands INSTEAD of map_icp"):
        V.Tracker(cfg, 0.0, host[1], 0.0, host[0], map=(0, cap, 4, 0), map_normals=NORMALS, map_icp=ICP, map_icp_joint=JOINT)
    one = V.Tracker(cfg, 0.0, host[1], 0.0, host[0], map=(0, cap, 4, 0), map_normals=NORMALS, map_icp=ICP)
    with pytest.raises(V.VorsError, match="read_map_icp_joint: the joint correction is not enabled"):
        one.read_map_icp_joint()
    assert V.lib().vors_tracker_read_map_icp_joint(one._h, None) == -1
    assert V.lib().vors_last_error() == b"read_map_icp_joint: the joint ICP correction is not enabled (vors_tracker_enable_map_icp_joint)"
    bare = V.Tracker(cfg, 0.0, host[1], 0.0, host[0], map=(0, cap, 4, 0), map_normals=NORMALS)
    bare.track(1.0, host[1], 1.0, host[0])
    with pytest.raises(V.VorsError) as e:
        V._check(V.lib().vors_tracker_enable_map_icp_joint(bare._h, V.C.byref(V.map_icp_joint_params(**JOINT))))
    assert str(e.value).endswith("enable_map_icp_joint: legal only before the first vors_tracker_track")


# ------------------------------------------------------------------------------------------------------------ 8
def test_trajectory_against_the_truth_recorded():
    """Recorded, not bounded (nobody has measured these): four runs — the stage off, vors_trackers_enable_map_icp, the robust pass with
    the CONDITION test, the joint pass with the CONDITION test, BOUNDS from the host scenes — against the twists the scenes were rendered
    from. The figures of the recorded run are in profiles/trackers_map_icp_joint_summary.md; the run prints them and writes them where
    VORS_MAP_ICP_JOINT_SUMMARY points."""
    names = ["off", "plain stage", "robust + CONDITION", "joint + CONDITION"]
    runs = [plain_run()[0], accepting_run()[0], run_j(C2F, V.ARITH_FUSED, dict(NEUTRAL, **BOUNDS))[0], run_j(C2F, V.ARITH_FUSED, dict(JOINT, **BOUNDS))[0]]
    truth = [[V.iso_inverse(V.se3_exp((BASE * SPEED[s] * k).astype(np.float32))) for s in range(N_SEQ)] for k in range(N_FRAMES)]
    lines = ["| sequence | " + " | ".join(f"{n}: dt [mm], angle [mrad]" for n in names) + " |", "|---|" + "---|" * len(names)]
    for s in range(N_SEQ):
        errs = [pose_error(r[-1]["poses"][s], truth[-1][s]) for r in runs]
        lines.append(f"| {s} | " + " | ".join(f"{1e3 * a:.3f}, {1e3 * b:.3f}" for a, b in errs) + " |")
    label = {0: "NOT_ATTEMPTED", 1: "ACCEPTED", 2: "ICP_STATUS", 3: "FEW_MATCHES", 4: "RMS", 5: "STEP", 6: "NONFINITE", 7: "CONDITION"}
    for name, run in zip(names[1:], runs[1:]):
        hist, worse, rows = {}, 0, []
        for k in range(1, N_FRAMES):
            for s in range(N_SEQ):
                r = run[k]["records"][s]
                if r["verdict"] == V.MAP_ICP_NOT_ATTEMPTED:
                    continue
                hist[label[int(r["verdict"])]] = hist.get(label[int(r["verdict"])], 0) + 1
                j = run[k]["joint"][s] if "joint" in run[k] else None
                dil = f"{j['dilution_t']:.4g} | {j['dilution_r']:.4g} | {j['photo_counts'][0]}" if j is not None else "- | - | -"
                a, b = pose_error(r["pose_before"], truth[k][s]), pose_error(r["pose_after"], truth[k][s])
                if r["verdict"] == V.MAP_ICP_ACCEPTED:
                    worse += b[0] > a[0]
                rows.append(f"| {k} | {s} | {label[int(r['verdict'])]} | {1e3 * a[0]:.3f} | {1e3 * a[1]:.3f} | {1e3 * b[0]:.3f} | {1e3 * b[1]:.3f} | "
                            f"{r['stats']['matched']} / {r['stats']['considered']} | {1e3 * r['stats']['rms']:.3f} | {dil} |")
        lines += ["", f"### {name}", "", f"verdicts: {hist}; accepted records whose translation error grew: {worse} of {hist.get('ACCEPTED', 0)}", "",
                  "| frame | sequence | verdict | before: dt [mm] | before: angle [mrad] | proposed: dt [mm] | proposed: angle [mrad] | matched / considered | rms [mm] | "
                  "dilution_t | dilution_r [1/m] | photo used |", "|---|---|---|---|---|---|---|---|---|---|---|---|"] + rows
    text = "\n".join(lines)
    print("\n" + text)
    path = os.environ.get("VORS_MAP_ICP_JOINT_SUMMARY")
    if path:
        with open(path, "w") as f:
            f.write(text + "\n")
    assert all(np.isfinite(r["poses"]).all() for run in runs for r in run)
