"""The averaged map as the model of the map ICP correction (vors_trackers_enable_map_icp_means, vors_trackers_map_icp_means,
vors_tracker_enable_map_icp_means, vors_tracker_read_map_icp_means). GPU only; every comparison is on bits. Sequences,
shapes, parameters and helpers are those of tests/test_gpu_trackers_map.py, tests/test_gpu_trackers_map_icp.py and
tests/test_gpu_trackers_map_icp_joint.py — six sequences, ten frames, 96x128 coarse-to-fine (120x160 dense), MAX_KF, NORMALS, ICP / JOINT —
with the voxel filter and its statistics at tests/test_gpu_trackers_map_voxel_stats.py's SLOTS and the 0.02 m of its VOXEL_M (below).

  1. the inputs reach the cases     2. the staging equals the public resolve, bit for bit, and only inside the window
  3. every correction is the composition of public entries, records bit for bit (robust and joint FUSED, dense REFERENCE, depth filter)
  4. a rejected correction changes nothing but the records and the staging     5. min_count beyond every count
  6. independence; Tracker(map_icp_means=...) == sequence 0 of an N = 1 handle     7. off means off; the workspace figure
  8. refusals     9. trajectory against the truth, recorded, not bounded

MEANS = (2, 1): at the first promotion of a sequence its map holds keyframe 0 alone, every voxel has span 0 and every rank is rejected; from
the second promotion on the voxels both keyframes saw pass. Test 1 asserts that the run reaches 0 < kept < resolved, an accepted
correction at ICP's min_match_ratio = 0.1 of the WHOLE window, and a sequence that promotes twice.
VOXEL: 0.02 m in both modes — VOXEL_M's dense value, used for the coarse-to-fine sequences too. At VOXEL_M's sparse 0.10 m a window holds
400 to 800 ranks and at (2, 1) no correction of the ten frames is accepted: the first promotions match nothing (ICP_STATUS), and every
later one proposes a step beyond ICP's 0.05 m / 0.05 rad (STEP; min_match_ratio rejects none of them: 162 / 616 is the lowest share). At
0.02 m windows hold 1400 to 5100 ranks and four corrections are accepted at (2, 1). min_count stays 2, ICP stays as it is.

Test 3 goes beyond the FIRST correction of tests/test_gpu_trackers_map_icp.py's recipe, on purpose: at a sequence's first promotion every
voxel was seen once, its centroid is its first point and the averaged model IS the list, so a stage that ignored the staging would pass.
Every promotion of the ten frames is compared instead, from the handle's own map, statistics and record before and after the call.

Test 7: neutral_run() and accepting_run() have no voxel filter, which the statistics need, and a filtered map is another model: their bits
cannot be those of a handle with statistics. What is compared is their recipe with the voxel filter on — with the statistics and without,
joint (neutral) and plain: the existing paths among themselves, which the new switch, left off, must not touch.

MEASURED (MI355X, the run recorded in profiles/trackers_map_icp_means_summary.md): see that file; nothing here is a bound on accuracy.
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from test_gpu_trackers_map import (BASE, MAX_KF, N_FRAMES, N_SEQ, SHAPES, SPEED, FILTER, config, frames_of, large_capacity, read_map, same_bits)
from test_gpu_trackers_map_icp import C2F, DENSE, ICP, NORMALS, keyframe_pose_bits, pose_error, read_icp
from test_gpu_trackers_map_icp_joint import JOINT, NEUTRAL, read_joint
from test_gpu_trackers_map_voxel_stats import SLOTS, VOXEL_M
from test_map_icp_condition_host import BOUNDS

MEANS = (2, 1)
VOXEL = {DENSE: VOXEL_M[DENSE], C2F: VOXEL_M[DENSE]}   # (the docstring)
NOTHING = dict(ICP, max_trans_m=0.0, max_rot_rad=0.0)


def handle_m(mode, arith, icp=None, joint=None, means=None, depth_filter=None, n=N_SEQ, stats=True):
    """A handle with the voxel filter, (stats) its statistics, normals, one of the two corrections or none, and (means) the averaged model."""
    rows, cols, _ = SHAPES[mode]
    tr = V.Trackers(config(mode, arith), n, rows, cols)
    if depth_filter is not None:
        tr.enable_depth_filter(*depth_filter)
    tr.enable_map(0, large_capacity(mode), MAX_KF, 0)
    tr.enable_map_voxels(VOXEL[mode], SLOTS)
    if stats:
        tr.enable_map_voxel_stats()
    tr.enable_map_normals(*NORMALS)
    if icp is not None:
        tr.enable_map_icp(**icp)
    if joint is not None:
        tr.enable_map_icp_joint(**joint)
    if means is not None:
        tr.enable_map_icp_means(*means)
    return tr


def read_means(tr):
    """Trackers.map_icp_means() on the host: the staging whole and the records."""
    import torch
    o = tr.map_icp_means()
    torch.cuda.synchronize()
    return dict(xyz=o["xyz_mean"].cpu().numpy().view(np.uint32), gray=o["gray_mean"].cpu().numpy(), records=o["records"].copy())


def run_m(mode, arith, icp=None, joint=None, means=None, depth_filter=None, frames=None, stats=True, resolve=None):
    """-> (per frame: poses, status, kf, stats, with a correction records / totals (/ joint), with means the staging and the means records,
    with `resolve` = (min_count, min_span) the public resolve and the map's totals and segments taken BEFORE the call; the map, its normals
    and (stats) its statistics after the last frame)"""
    import torch
    frames = frames_of(mode) if frames is None else frames
    tr = handle_m(mode, arith, icp, joint, means, depth_filter, n=frames[0][0].shape[0], stats=stats)
    rec = []
    for k in range(N_FRAMES):
        g, d = frames[k]
        pre = None
        if k and resolve is not None:
            o, m = tr.map_voxel_means(*resolve), read_map(tr)
            torch.cuda.synchronize()
            pre = dict(xyz=o["xyz_mean"].cpu().numpy().view(np.uint32), gray=o["gray_mean"].cpu().numpy(), counts=m["counts"], n_segments=m["n_segments"],
                       segments=m["segments"])
        tr.init(g, d) if k == 0 else tr.track(g, d)
        poses, status, kf = tr.current_frames()
        r = dict(poses=poses, status=status, kf=kf, stats=tr.stats().copy() if k else None, pre=pre)
        if (icp is not None or joint is not None) and k:
            r["records"], r["totals"] = read_icp(tr)
            if joint is not None:
                r["joint"] = read_joint(tr)
        if means is not None:
            r["means"] = read_means(tr)
        rec.append(r)
    m = read_map(tr)
    m["normals"] = tr.map_normals().cpu().numpy()
    if stats:
        st = tr.map_voxel_stats()
        m["sums"], m["obs"] = st["sums"].cpu().numpy(), st["obs"].cpu().numpy()
    torch.cuda.synchronize()
    return rec, m


@functools.lru_cache(maxsize=None)
def bare_run():
    """The voxel filter, its statistics and the normals; no correction."""
    return run_m(C2F, V.ARITH_FUSED)


@functools.lru_cache(maxsize=None)
def means_run(last_keyframes=0):
    return run_m(C2F, V.ARITH_FUSED, icp=dict(ICP, last_keyframes=last_keyframes), means=MEANS, resolve=MEANS)


def window_of(pre, s, mode, last_keyframes):
    return V.map_icp_window_host(pre["segments"][s], int(pre["n_segments"][s]), MAX_KF, int(pre["counts"][s]), large_capacity(mode), last_keyframes)


def same_map_and_statistics(m, bm):
    for name in ("counts", "n_segments"):
        assert same_bits(m[name], bm[name]), f"the map's {name} differs"
    for s in range(len(bm["n_segments"])):
        k = min(int(bm["counts"][s]), m["xyz"].shape[1])
        for name in ("xyz", "pixel", "gray", "normals") + (("sums", "obs") if "sums" in bm and "sums" in m else ()):
            assert same_bits(m[name][s, :k], bm[name][s, :k]), f"sequence {s}: the map's {name} differs"
        k = int(bm["n_segments"][s])
        assert same_bits(m["segments"][s, :k], bm["segments"][s, :k])


# ------------------------------------------------------------------------------------------------------------ 1
def test_inputs_reach_the_cases():
    rec, _ = means_run()
    promoted, partly, accepted = np.zeros(N_SEQ, np.int64), 0, 0
    for k in range(1, N_FRAMES):
        new = rec[k]["kf"] != rec[k - 1]["kf"]
        promoted += new
        mr, r = rec[k]["means"]["records"], rec[k]["records"]
        for s in np.nonzero(new)[0]:
            print(f"frame {k} sequence {s}: kept {mr[s]['kept']} / resolved {mr[s]['resolved']}, verdict {r[s]['verdict']}, "
                  f"matched {r[s]['stats']['matched']} / considered {r[s]['stats']['considered']}")
            partly += 0 < mr[s]["kept"] < mr[s]["resolved"]
            accepted += r[s]["verdict"] == V.MAP_ICP_ACCEPTED
    assert partly >= 1, "no promoted sequence had 0 < kept < resolved at (2, 1)"
    assert accepted >= 1, "no correction was accepted with the averaged model"
    assert (promoted >= 2).any(), "no sequence promoted twice"


# ------------------------------------------------------------------------------------------------------------ 2
def test_staging_is_the_public_resolve_inside_the_window_only():
    rec, _ = means_run(last_keyframes=1)
    cap = large_capacity(C2F)
    assert (rec[0]["means"]["xyz"] == 0).all() and (rec[0]["means"]["gray"] == 0).all() and (rec[0]["means"]["records"].view(np.uint8) == 0).all()
    want_xyz, want_gray = np.zeros((N_SEQ, cap, 3), np.uint32), np.zeros((N_SEQ, cap), np.uint8)
    promoted, kept_older, windows = np.zeros(N_SEQ, np.int64), 0, 0
    for k in range(1, N_FRAMES):
        new = rec[k]["kf"] != rec[k - 1]["kf"]
        pre, got = rec[k]["pre"], rec[k]["means"]
        for s in range(N_SEQ):
            mr = got["records"][s]
            if not new[s]:
                assert mr["resolved"] == 0 and mr["kept"] == 0, f"frame {k} sequence {s}: not promoted, record {mr}"
                continue
            first, count = window_of(pre, s, C2F, 1)
            r = rec[k]["records"][s]
            assert (r["range_first"], r["range_count"]) == (first, count) and count > 0
            assert mr["resolved"] == count, f"frame {k} sequence {s}: resolved {mr['resolved']} against the window's {count}"
            w = slice(first, first + count)
            nan = np.isnan(pre["xyz"][s, w].view(np.float32)[:, 0])
            assert mr["kept"] == int((~nan).sum()), f"frame {k} sequence {s}: kept {mr['kept']} against {int((~nan).sum())} ranks of the public resolve"
            if promoted[s] >= 1 and first > 0:   # the ranks below this window keep an EARLIER window's bits: do the statistics of now differ there?
                kept_older += int((pre["xyz"][s, :first] != want_xyz[s, :first]).any())
            want_xyz[s, w], want_gray[s, w] = pre["xyz"][s, w], pre["gray"][s, w]
            promoted[s] += 1
            windows += 1
        # every sequence whole: windows of this call, earlier windows' bits below them, zero bytes beyond, a sequence not promoted unchanged
        assert same_bits(got["xyz"], want_xyz), f"frame {k}: the staged centroids are not the public resolve's inside the windows, untouched outside"
        assert same_bits(got["gray"], want_gray), f"frame {k}: the staged grey"
    assert windows >= 10 and (promoted >= 2).any()
    assert kept_older >= 1, "no second window left ranks below it whose statistics had moved on: the window's lower edge was never tested"
    assert (promoted == 0).any(), "every sequence promoted: an untouched sequence was never seen"


# ------------------------------------------------------------------------------------------------------------ 3
def every_correction(mode, arith, params, joint, means, depth_filter=None):
    """Every promotion of the ten frames: the handle's own map, normals and public resolve BEFORE the call, the record's pose_before, the
    window of map_icp_window_host and the public ICP entry give pose_after, statistics, gate counts (and the joint record) again; the host
    twins give the verdict; the means record is the window's length and the resolve's passing ranks in it."""
    import torch
    rows, cols, _ = SHAPES[mode]
    frames, cap = frames_of(mode), large_capacity(mode)
    cam5 = np.array(V.scaled_intrinsics(rows, cols), np.float32)
    on = handle_m(mode, arith, None if joint else params, params if joint else None, means, depth_filter)
    compared, verdicts, moved = 0, [], 0
    for k in range(N_FRAMES):
        g, d = frames[k]
        if k == 0:
            on.init(g, d)
            continue
        before, counts_t, normals_t = read_map(on), on.map()["counts"], on.map_normals()
        pre = on.map_voxel_means(*means)
        lists_differ = (on.map()["xyz"].view(torch.int32) != pre["xyz_mean"].view(torch.int32)).any(dim=2).cpu().numpy()
        on.track(g, d)
        o_poses, _, o_kf = on.current_frames()
        rec, _ = read_icp(on)
        jrec = read_joint(on) if joint else None
        mrec = read_means(on)["records"]
        new = np.nonzero(o_kf == k)[0]
        assert ((rec["verdict"] != V.MAP_ICP_NOT_ATTEMPTED) == (o_kf == k)).all()
        if len(new) == 0:
            assert (mrec.view(np.uint8) == 0).all()
            continue
        depth = on.keyframe_depth()[0] if depth_filter is not None else frames[k][1]
        ranges = np.zeros((N_SEQ, 2), np.uint32)
        for s in new:
            ranges[s] = V.map_icp_window_host(before["segments"][s], int(before["n_segments"][s]), MAX_KF, int(before["counts"][s]), cap,
                                              params.get("last_keyframes", 0))
        fn = V.depth_normals(depth, cam5, V.DEPTH_SCALE, *NORMALS)["normals"]
        start = torch.from_numpy(np.ascontiguousarray(rec["pose_before"])).cuda()
        common = dict(damping=0.0, step_eps=1e-5, iters=params["iters"], min_points=6, frame_normals=fn, min_cos=params["min_cos"],
                      huber_m=params["huber_m"], ranges=torch.from_numpy(ranges.view(np.int32)).cuda(), gate_counts=True, sums29=True)
        if joint:
            ref = V.icp_points_joint(pre["xyz_mean"], normals_t, pre["gray_mean"], counts_t, depth, frames[k][0], cam5, V.DEPTH_SCALE, start,
                                     params["dist_m"], photo_scale_m=params["photo_scale_m"], photo_huber_grey=params["photo_huber_grey"],
                                     photo_counts=True, **common)
            dil, flags = V.icp_condition(ref["sums29"])
        else:
            ref = V.icp_points_robust(pre["xyz_mean"], normals_t, counts_t, depth, cam5, V.DEPTH_SCALE, start, params["dist_m"], **common)
        torch.cuda.synchronize()
        ref_pose, ref_stats = ref["poses"].cpu().numpy(), V.decode_icp_stats(ref["stats"])
        ref_gates = ref["gate_counts"].cpu().numpy().view(np.uint32)
        pre_nan = torch.isnan(pre["xyz_mean"][:, :, 0]).cpu().numpy()
        kf_pose, after = keyframe_pose_bits(on), read_map(on)
        for s in new:
            r, where = rec[s], f"frame {k} sequence {s}"
            first, count = int(ranges[s, 0]), int(ranges[s, 1])
            assert r["frame"] == k and (r["range_first"], r["range_count"]) == (first, count) and count > 0, f"{where}: window"
            assert r["stats"]["considered"] == count, f"{where}: considered is not the window's length"
            assert mrec[s]["resolved"] == count and mrec[s]["kept"] == int((~pre_nan[s, first:first + count]).sum()), f"{where}: means record {mrec[s]}"
            assert same_bits(r["pose_after"], ref_pose[s]), f"{where}: pose_after differs from the public pass on the public resolve"
            assert r["stats"].tobytes() == ref_stats[s].tobytes(), f"{where}: stats {r['stats']} against {ref_stats[s]}"
            assert same_bits(r["gate_counts"], ref_gates[s]), f"{where}: gate counts"
            assert r["stats"]["matched"] <= mrec[s]["kept"], f"{where}: more matches than finite ranks"
            if joint:
                j = jrec[s]
                dd, ff = dil.cpu().numpy(), flags.cpu().numpy()
                assert same_bits(np.array([j["dilution_t"], j["dilution_r"]], np.float32), dd[s]) and j["condition_flags"] == ff[s], f"{where}: {j}"
                assert same_bits(j["photo_counts"], ref["photo_counts"].cpu().numpy().view(np.uint32)[s]), f"{where}: photo counts"
                want = V.map_icp_verdict_joint_host(params, ref_stats[s], r["pose_before"], ref_pose[s], dd[s, 0], dd[s, 1])
            else:
                want = V.map_icp_verdict_host(params, ref_stats[s], r["pose_before"], ref_pose[s])
            assert r["verdict"] == want, f"{where}: verdict {r['verdict']} against the host twin's {want}"
            reported = r["pose_after"] if want == V.MAP_ICP_ACCEPTED else r["pose_before"]
            assert same_bits(o_poses[s], reported) and same_bits(kf_pose[s], reported), f"{where}: the pose reported"
            seg = after["segments"][s, int(after["n_segments"][s]) - 1]
            assert seg["frame"] == k and same_bits(seg["pose7"], reported), f"{where}: the new segment was not emitted at the pose reported"
            verdicts.append(int(want))
            moved += bool(lists_differ[s, first:first + count].any())
            compared += 1
    print(f"\nevery correction ({mode=}, {arith=}, joint={joint}, means={means}, filter={depth_filter is not None}): {compared} compared, "
          f"verdicts {verdicts}, windows whose model differed from the lists: {moved}")
    assert compared >= 10, f"only {compared} promotions were compared"
    assert moved >= 1, "the averaged model never differed from the map's own lists inside a window: the staging was never told from them"
    return verdicts


def test_every_correction_robust_fused():
    assert V.MAP_ICP_ACCEPTED in every_correction(C2F, V.ARITH_FUSED, ICP, False, MEANS)


def test_every_correction_joint_fused():
    every_correction(C2F, V.ARITH_FUSED, dict(JOINT, **BOUNDS), True, MEANS)


def test_every_correction_dense_reference():
    every_correction(DENSE, V.ARITH_REFERENCE, dict(JOINT, **BOUNDS), True, (1, 0))


def test_every_correction_depth_filter():
    every_correction(C2F, V.ARITH_FUSED, ICP, False, (1, 0), depth_filter=FILTER)


# ------------------------------------------------------------------------------------------------------------ 4
def test_rejections_change_nothing_but_records_and_staging():
    (bare, bm), (rec, m) = bare_run(), run_m(C2F, V.ARITH_FUSED, icp=NOTHING, means=(1, 0))
    promoted, moved, staged = 0, 0, False
    for k in range(N_FRAMES):
        for name in ("poses", "status", "kf") + (("stats",) if k else ()):
            assert same_bits(rec[k][name], bare[k][name]), f"frame {k}: {name} moved although every correction was to be rejected"
        if k:
            new = rec[k]["kf"] != rec[k - 1]["kf"]
            r = rec[k]["records"]
            assert ((r["verdict"] != V.MAP_ICP_NOT_ATTEMPTED) == new).all()
            for s in np.nonzero(new)[0]:
                promoted += 1
                if not same_bits(r[s]["pose_before"], r[s]["pose_after"]):
                    moved += 1
                    assert r[s]["verdict"] != V.MAP_ICP_ACCEPTED, f"frame {k} sequence {s}: accepted at a bound of zero with a step that is not zero"
            assert (rec[k]["means"]["records"]["resolved"] > 0).tolist() == new.tolist()
            staged |= bool((rec[k]["means"]["xyz"] != 0).any())
    assert promoted >= 10 and moved >= 1 and staged
    same_map_and_statistics(m, bm)


# ------------------------------------------------------------------------------------------------------------ 5
def test_min_count_beyond_every_count():
    (bare, bm), (rec, m) = bare_run(), run_m(C2F, V.ARITH_FUSED, icp=ICP, means=(0xFFFFFFFF, 0))
    attempted = 0
    for k in range(N_FRAMES):
        for name in ("poses", "status", "kf") + (("stats",) if k else ()):
            assert same_bits(rec[k][name], bare[k][name]), f"frame {k}: {name} moved although no rank passed"
        if k:
            r, mr, st = rec[k]["records"], rec[k]["means"]["records"], rec[k]["means"]
            for s in np.nonzero(rec[k]["kf"] != rec[k - 1]["kf"])[0]:
                w = slice(int(r[s]["range_first"]), int(r[s]["range_first"]) + int(r[s]["range_count"]))
                assert mr[s]["resolved"] == r[s]["range_count"] > 0 and mr[s]["kept"] == 0
                assert (st["xyz"][s, w] == 0x7FC00000).all() and (st["gray"][s, w] == 0).all(), f"frame {k} sequence {s}: a rank of the window is not the NaN row"
                assert r[s]["stats"]["matched"] == 0 and r[s]["stats"]["considered"] == r[s]["range_count"]
                assert r[s]["verdict"] not in (V.MAP_ICP_ACCEPTED, V.MAP_ICP_NOT_ATTEMPTED)
                attempted += 1
            assert (rec[k]["totals"][:, 1] == 0).all()
    assert attempted >= 10
    same_map_and_statistics(m, bm)


# ------------------------------------------------------------------------------------------------------------ 6
def test_independence_and_the_single_tracker():
    mode, arith, s = C2F, V.ARITH_FUSED, 4
    joint = dict(JOINT, **BOUNDS)
    frames = frames_of(mode)
    six, _ = run_m(mode, arith, joint=joint, means=MEANS)
    one_seq = [(g[[s]].contiguous(), d[[s]].contiguous()) for g, d in frames]
    alone, m = run_m(mode, arith, joint=joint, means=MEANS, frames=one_seq)
    host = [(g[s].cpu().numpy(), d[s].cpu().numpy().view(np.uint16)) for g, d in frames]
    one = V.Tracker(config(mode, arith), 0.0, host[0][1], 0.0, host[0][0], map=(0, large_capacity(mode), MAX_KF, 0), map_voxels=(VOXEL[mode], SLOTS),
                    map_voxel_stats=True, map_normals=NORMALS, map_icp_joint=joint, map_icp_means=MEANS)
    attempted, partly = 0, 0
    for k in range(1, N_FRAMES):
        for name in ("poses", "status", "kf", "stats", "records", "totals", "joint"):
            assert same_bits(six[k][name][[s]], alone[k][name]), f"frame {k}: {name} of sequence {s} depends on its company"
        for name in ("xyz", "gray", "records"):
            assert same_bits(six[k]["means"][name][[s]], alone[k]["means"][name]), f"frame {k}: the staged {name} of sequence {s} depends on its company"
        assert one.track(float(k), host[k][1], float(k), host[k][0]) == alone[k]["status"][0]
        got, gj, gm = one.read_map_icp(), one.read_map_icp_joint(), one.read_map_icp_means()
        assert got["record"].tobytes() == alone[k]["records"][0].tobytes(), f"frame {k}: record {got['record']} against {alone[k]['records'][0]}"
        assert gj.tobytes() == alone[k]["joint"][0].tobytes() and same_bits(got["totals"], alone[k]["totals"][0])
        assert gm.tobytes() == alone[k]["means"]["records"][0].tobytes(), f"frame {k}: means record {gm} against {alone[k]['means']['records'][0]}"
        assert same_bits(one.current_frame()[1], alone[k]["poses"][0]), f"frame {k}: the pose returned is not the handle's"
        attempted += got["record"]["verdict"] != V.MAP_ICP_NOT_ATTEMPTED
        partly += 0 < gm["kept"] < gm["resolved"]
    assert attempted >= 3 and partly >= 1
    final = one.read_map()
    assert final["count"] == m["counts"][0] and same_bits(final["xyz"], m["xyz"][0, :final["count"]])


# ------------------------------------------------------------------------------------------------------------ 7
def test_off_means_off_and_the_workspace_figure():
    """(the docstring of the module: the recipes of neutral_run / accepting_run with the voxel filter on)"""
    with_stats, ms = run_m(C2F, V.ARITH_FUSED, joint=NEUTRAL)
    without, mw = run_m(C2F, V.ARITH_FUSED, joint=NEUTRAL, stats=False)
    plain, mp = run_m(C2F, V.ARITH_FUSED, icp=ICP, stats=False)
    accepted = 0
    for k in range(N_FRAMES):
        for name in ("poses", "status", "kf") + (("stats", "records", "totals") if k else ()):
            assert same_bits(with_stats[k][name], without[k][name]), f"frame {k}: {name}: the statistics moved a handle without the averaged model"
            assert same_bits(with_stats[k][name], plain[k][name]), f"frame {k}: {name} differs from the handle with vors_trackers_enable_map_icp"
        if k:
            assert same_bits(with_stats[k]["joint"], without[k]["joint"])
            accepted += int((with_stats[k]["records"]["verdict"] == V.MAP_ICP_ACCEPTED).sum())
    assert accepted >= 1
    same_map_and_statistics(ms, mw), same_map_and_statistics(ms, mp)
    for make in (lambda: handle_m(C2F, V.ARITH_FUSED, icp=ICP), lambda: handle_m(C2F, V.ARITH_FUSED, joint=dict(JOINT, **BOUNDS))):
        tr = make()
        before = tr.workspace_bytes()
        tr.enable_map_icp_means(*MEANS)
        assert tr.workspace_bytes() == before + N_SEQ * large_capacity(C2F) * 13 + 8 * N_SEQ
        ws = tr.workspace_bytes()
        frames = frames_of(C2F)
        tr.init(*frames[0])
        for k in range(1, 4):
            tr.track(*frames[k])
        assert read_means(tr)["records"]["resolved"].sum() > 0 and tr.workspace_bytes() == ws   # no later call allocates
        tr.init(*frames[0])   # a second init zeroes staging and records again
        o = read_means(tr)
        assert (o["xyz"] == 0).all() and (o["gray"] == 0).all() and (o["records"].view(np.uint8) == 0).all()


# ------------------------------------------------------------------------------------------------------------ 8
def test_refusals():
    mode = C2F
    rows, cols, _ = SHAPES[mode]
    cfg, frames, cap = config(mode, V.ARITH_FUSED), frames_of(mode), 5000
    lib = V.lib()

    def refused(tr, sentence):
        before = tr.workspace_bytes()
        with pytest.raises(V.VorsError) as e:
            tr.enable_map_icp_means(*MEANS)
        assert str(e.value).endswith(sentence), str(e.value)
        assert tr.workspace_bytes() == before   # a refused call allocates nothing

    def started(stats=True, icp=True):
        t = V.Trackers(cfg, N_SEQ, rows, cols)
        t.enable_map(0, cap, 4, 0)
        t.enable_map_voxels(VOXEL[mode], SLOTS)
        if stats:
            t.enable_map_voxel_stats()
        t.enable_map_normals(*NORMALS)
        if icp:
            t.enable_map_icp(**ICP)
        return t

    assert lib.vors_trackers_enable_map_icp_means(None, 2, 1) == -1 and lib.vors_last_error() == b"enable_map_icp_means: the handle t is NULL"
    refused(started(stats=False), "enable_map_icp_means: needs the voxel statistics first (vors_trackers_enable_map_voxel_stats)")
    no_icp = started(icp=False)
    refused(no_icp, "enable_map_icp_means: needs the correction first (vors_trackers_enable_map_icp or vors_trackers_enable_map_icp_joint)")
    with pytest.raises(V.VorsError, match="map_icp_means: the averaged model is not enabled"):
        no_icp.map_icp_means()
    t = started()
    with pytest.raises(V.VorsError, match="map_icp_means: the averaged model is not enabled"):
        t.map_icp_means()
    with pytest.raises(V.VorsError, match="min_count must be in"):
        t.enable_map_icp_means(-1, 0)
    t.enable_map_icp_means(*MEANS)
    refused(t, "enable_map_icp_means: the averaged model is already enabled")
    p = [V.C.c_void_p() for _ in range(3)]
    assert lib.vors_trackers_map_icp_means(t._h, None, None, None) == 0   # each output is nullable
    assert lib.vors_trackers_map_icp_means(t._h, V.C.byref(p[0]), V.C.byref(p[1]), V.C.byref(p[2])) == 0 and all(q.value for q in p)
    late = started()
    late.init(*frames[0])
    refused(late, "enable_map_icp_means: legal only before vors_trackers_init")
    # the single tracker: the same refusals, "before init" reads "before the first vors_tracker_track"
    host = (frames[0][0][0].cpu().numpy(), frames[0][1][0].cpu().numpy().view(np.uint16))
    kw = dict(map=(0, cap, 4, 0), map_voxels=(VOXEL[mode], SLOTS), map_normals=NORMALS)
    with pytest.raises(V.VorsError, match="map_icp_means: the averaged model needs the voxel statistics"):
        V.Tracker(cfg, 0.0, host[1], 0.0, host[0], map_icp=ICP, map_icp_means=MEANS, **kw)
    with pytest.raises(V.VorsError, match="map_icp_means: the averaged model needs the correction"):
        V.Tracker(cfg, 0.0, host[1], 0.0, host[0], map_voxel_stats=True, map_icp_means=MEANS, **kw)

    def refused_one(one, sentence):
        assert lib.vors_tracker_enable_map_icp_means(one._h, 2, 1) == -1
        assert lib.vors_last_error().decode().endswith(sentence), lib.vors_last_error()

    assert lib.vors_tracker_enable_map_icp_means(None, 2, 1) == -1 and lib.vors_last_error() == b"enable_map_icp_means: the handle t is NULL"
    assert lib.vors_tracker_read_map_icp_means(None, None) == -1 and lib.vors_last_error() == b"read_map_icp_means: the handle t is NULL"
    refused_one(V.Tracker(cfg, 0.0, host[1], 0.0, host[0], map_icp=ICP, **kw),
                "enable_map_icp_means: needs the voxel statistics first (vors_trackers_enable_map_voxel_stats)")
    no_icp = V.Tracker(cfg, 0.0, host[1], 0.0, host[0], map_voxel_stats=True, **kw)
    refused_one(no_icp, "enable_map_icp_means: needs the correction first (vors_trackers_enable_map_icp or vors_trackers_enable_map_icp_joint)")
    with pytest.raises(V.VorsError, match="read_map_icp_means: the averaged model is not enabled"):
        no_icp.read_map_icp_means()
    assert lib.vors_tracker_read_map_icp_means(no_icp._h, None) == -1
    assert lib.vors_last_error() == b"read_map_icp_means: the averaged model is not enabled (vors_tracker_enable_map_icp_means)"
    one = V.Tracker(cfg, 0.0, host[1], 0.0, host[0], map_voxel_stats=True, map_icp=ICP, map_icp_means=MEANS, **kw)
    refused_one(one, "enable_map_icp_means: the averaged model is already enabled")
    assert one.read_map_icp_means().tobytes() == bytes(8)
    late = V.Tracker(cfg, 0.0, host[1], 0.0, host[0], map_voxel_stats=True, map_icp=ICP, **kw)
    late.track(1.0, host[1], 1.0, host[0])
    refused_one(late, "enable_map_icp_means: legal only before the first vors_tracker_track")


# ------------------------------------------------------------------------------------------------------------ 9
def test_trajectory_against_the_truth_recorded():
    """Recorded, not bounded: tests/test_gpu_trackers_map_icp_joint.py's experiment (robust + CONDITION, joint + CONDITION, BOUNDS from the
    host scenes) on a voxel-filtered map, the model being the map's lists and the averaged map at (1, 0) and (2, 1), against the twists
    the scenes were rendered from; every attempted correction with its pose error before and after. The figures of the recorded run are
    in profiles/trackers_map_icp_means_summary.md; the run prints them and writes them where VORS_MAP_ICP_MEANS_SUMMARY points."""
    stages = {"robust + CONDITION": dict(NEUTRAL, **BOUNDS), "joint + CONDITION": dict(JOINT, **BOUNDS)}
    models = {"lists": None, "means (1, 0)": (1, 0), "means (2, 1)": (2, 1)}
    runs = {"off": bare_run()[0]}
    for sn, joint in stages.items():
        for mn, means in models.items():
            runs[f"{sn}, {mn}"] = run_m(C2F, V.ARITH_FUSED, joint=joint, means=means)[0]
    truth = [[V.iso_inverse(V.se3_exp((BASE * SPEED[s] * k).astype(np.float32))) for s in range(N_SEQ)] for k in range(N_FRAMES)]
    lines = ["final pose error per sequence, dt [mm], angle [mrad]:", "", "| run | " + " | ".join(str(s) for s in range(N_SEQ)) + " |", "|---|" + "---|" * N_SEQ]
    for name, run in runs.items():
        errs = [pose_error(run[-1]["poses"][s], truth[-1][s]) for s in range(N_SEQ)]
        lines.append(f"| {name} | " + " | ".join(f"{1e3 * a:.3f}, {1e3 * b:.3f}" for a, b in errs) + " |")
    label = {0: "NOT_ATTEMPTED", 1: "ACCEPTED", 2: "ICP_STATUS", 3: "FEW_MATCHES", 4: "RMS", 5: "STEP", 6: "NONFINITE", 7: "CONDITION"}
    for name, run in list(runs.items())[1:]:
        hist, worse, rows = {}, 0, []
        for k in range(1, N_FRAMES):
            for s in range(N_SEQ):
                r = run[k]["records"][s]
                if r["verdict"] == V.MAP_ICP_NOT_ATTEMPTED:
                    continue
                hist[label[int(r["verdict"])]] = hist.get(label[int(r["verdict"])], 0) + 1
                mr = run[k]["means"]["records"][s] if "means" in run[k] else None
                a, b = pose_error(r["pose_before"], truth[k][s]), pose_error(r["pose_after"], truth[k][s])
                if r["verdict"] == V.MAP_ICP_ACCEPTED:
                    worse += b[0] > a[0]
                rows.append(f"| {k} | {s} | {label[int(r['verdict'])]} | {1e3 * a[0]:.3f} | {1e3 * a[1]:.3f} | {1e3 * b[0]:.3f} | {1e3 * b[1]:.3f} | "
                            f"{r['stats']['matched']} / {r['stats']['considered']} | {'-' if mr is None else str(mr['kept']) + ' / ' + str(mr['resolved'])} | "
                            f"{1e3 * r['stats']['rms']:.3f} |")
        lines += ["", f"### {name}", "", f"verdicts: {hist}; accepted records whose translation error grew: {worse} of {hist.get('ACCEPTED', 0)}", "",
                  "| frame | sequence | verdict | before: dt [mm] | before: angle [mrad] | proposed: dt [mm] | proposed: angle [mrad] | matched / considered | "
                  "kept / resolved | rms [mm] |", "|---|---|---|---|---|---|---|---|---|---|"] + rows
    text = "\n".join(lines)
    print("\n" + text)
    path = os.environ.get("VORS_MAP_ICP_MEANS_SUMMARY")
    if path:
        with open(path, "w") as f:
            f.write(text + "\n")
    assert all(np.isfinite(r["poses"]).all() for run in runs.values() for r in run)
