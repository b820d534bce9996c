"""The masked passes of the lock-step trackers (depth filter, keyframe map, its voxel filter) on planes that force every narrow path.
GPU only; every comparison is on bits.

Every other file runs these passes on planes of 60x80, 96x128 or 120x160 pixels: multiples of 4, so every sequence's planes start
aligned and the passes take their wide forms throughout. Here S0 is ODD — dense 61x81 / 3 levels (S0 = 4941), coarse-to-fine 97x129 /
4 levels (S0 = 12513) — so with three sequences every sequence but the first starts its weight plane off a 4-byte boundary, sequence 1
starts its key plane off a 16-byte boundary, and no plane is a multiple of 4 pixels: the fill of the key planes, the splat's weight
gather, the merge and the map's keep gather all run one element per access.

  1. the inputs reach the cases (odd planes, a frame that promotes some but not all sequences, the last sequence promotes, a keyframe
     that keeps some of its points at min_weight 2, the voxel filter drops something)
  2. shadow fusion: every promoted plane equals a separate Batch's fuse_depth (tests/test_gpu_trackers_depth_filter.py, case 1); a
     sequence that does not promote keeps its planes
  3. shadow map: every segment equals a separate Batch's point_cloud under the weight mask (tests/test_gpu_trackers_map.py, case 2); a
     sequence that does not promote keeps its list
  4. voxel filter: the filtered map is the first-occurrence filter of the unfiltered run's list (tests/test_gpu_trackers_map_voxels.py,
     case 2), and tracking and the filter's planes do not depend on it

Seeds and BASE are those of tests/test_gpu_trackers_depth_filter.py. SPEED was chosen with the oracle's tracker on the CPU (an unfiltered
run, oracle.track_sequences on oracle.synth_frame's renderings of these seeds and twists): promotions per sequence 2, 0, 2 and per frame
0, 2, 0, 2, 0 (dense 61x81 / 3), 2, 0, 1 and 0, 1, 1, 1, 0 (coarse-to-fine 97x129 / 4) — in both modes sequence 1 never promotes, so every
promotion is a partial one, and the last sequence promotes. Case 1 asserts what the tests need of it on the run itself.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V

N_SEQ, N_FRAMES = 3, 6
BASE = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001])
SPEED = np.array([6.0, 0.05, 9.0])
TOL_M, MAX_W, FILL = 0.02, 255, 1
MIN_WEIGHT, MAX_KF, SLOTS = 2, 8, 65536
SHAPES = {V.CANDIDATES_DENSE: (61, 81, 3), V.CANDIDATES_COARSE_TO_FINE: (97, 129, 4)}
# voxel edges of tests/test_gpu_trackers_map_voxels.py's crowded table (dense) and of its sparse modes
VOXEL_M = {V.CANDIDATES_DENSE: 0.05, V.CANDIDATES_COARSE_TO_FINE: 0.10}
MODES = pytest.mark.parametrize("mode", [V.CANDIDATES_DENSE, V.CANDIDATES_COARSE_TO_FINE], ids=["dense", "coarse_to_fine"])
ARITH = V.ARITH_FUSED   # (the passes are the EXACT sources' whatever the handle's arithmetic)
NONE = np.uint64(V.VOXEL_NONE)


def config(mode):
    rows, cols, L = SHAPES[mode]
    intr = V.scaled_intrinsics(rows, cols)
    return V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, arithmetic=ARITH)


def capacity(mode):
    rows, cols, _ = SHAPES[mode]
    return rows * cols * N_FRAMES   # every pixel of every frame: nothing is clipped


@functools.lru_cache(maxsize=None)
def frames_of(mode):
    """[N_FRAMES] of (gray [N_SEQ, rows, cols] u8, depth int16 holding u16) on the device: 2 % of the depth pixels are 0."""
    import torch
    rows, cols, _ = SHAPES[mode]
    intr = V.scaled_intrinsics(rows, cols)
    out = [V.synth_render_frames([1000 + s for s in range(N_SEQ)], [k] * N_SEQ, [BASE * SPEED[s] * k for s in range(N_SEQ)], rows, cols, intr,
                                 invalid_percent=2) for k in range(N_FRAMES)]
    torch.cuda.synchronize()
    return out


def read_map(tr, voxels):
    import torch
    m = tr.map()
    v = tr.map_voxels() if voxels else {}
    torch.cuda.synchronize()
    out = dict(xyz=m["xyz"].cpu().numpy(), pixel=m["pixel"].cpu().numpy().view(np.uint32), gray=m["gray"].cpu().numpy(),
               counts=m["counts"].cpu().numpy().view(np.uint32), n_segments=m["n_segments"].cpu().numpy().view(np.uint32),
               segments=V.decode_map_segments(m["segments"]))
    out.update({k: t.cpu().numpy().view(np.uint32) for k, t in v.items()})
    return out


@functools.lru_cache(maxsize=None)
def mapped_run(mode, voxels):
    """Depth filter on, keyframe map at level 0 from min_weight 2 on, with or without the voxel filter -> per frame a dict of host
    arrays: poses, status, kf, stats (k >= 1), depth, weight and map, all read back after the frame."""
    rows, cols, _ = SHAPES[mode]
    tr = V.Trackers(config(mode), N_SEQ, rows, cols)
    tr.enable_depth_filter(TOL_M, MAX_W, FILL)
    tr.enable_map(0, capacity(mode), MAX_KF, MIN_WEIGHT)
    if voxels:
        tr.enable_map_voxels(VOXEL_M[mode], SLOTS)
    rec = []
    for k, (g, d) in enumerate(frames_of(mode)):
        if k == 0:
            tr.init(g, d)
        else:
            tr.track(g, d)
        poses, status, kf = tr.current_frames()
        dd, ww = tr.keyframe_depth()
        rec.append(dict(poses=poses, status=status, kf=kf, stats=tr.stats().copy() if k else None, depth=dd.cpu().numpy().view(np.uint16),
                        weight=ww.cpu().numpy(), map=read_map(tr, voxels)))
    return rec


def promotions(rec):
    """[F-1, n] bool: sequence s promoted at frame k (the keyframe index moved)."""
    return np.stack([rec[k]["kf"] != rec[k - 1]["kf"] for k in range(1, len(rec))])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def written(m, s):
    """Sequence s's list and records as bytes."""
    k, j = int(m["counts"][s]), int(m["n_segments"][s])
    return (k, j, m["segments"][s, :j].tobytes()) + tuple(m[name][s, :k].tobytes() for name in ("xyz", "pixel", "gray"))


# ------------------------------------------------------------------------------------------------------------ 1
@MODES
def test_inputs_reach_the_cases(mode):
    rows, cols, _ = SHAPES[mode]
    S0 = rows * cols
    assert S0 % 2 == 1 and N_SEQ >= 3, "an odd plane: sequence 1 starts every plane off its wide alignment, sequence 2 its weight plane"
    for voxels in (False, True):
        rec = mapped_run(mode, voxels)
        p = promotions(rec)
        per_frame = p.sum(axis=1)
        print(f"promotions per sequence {p.sum(axis=0)}, per frame {per_frame}")
        assert ((per_frame > 0) & (per_frame < N_SEQ)).any(), "no frame on which some but not all sequences promote"
        assert p[:, N_SEQ - 1].any(), "the last sequence must promote"
        assert all((r["status"] == 0).all() for r in rec)
    m, f = mapped_run(mode, False)[-1]["map"], mapped_run(mode, True)[-1]["map"]
    usable = mapped_run(mode, False)[-1]["stats"]["n_points"][:, 0]
    print(f"kept at min_weight {MIN_WEIGHT}: {m['counts']}, after the voxel filter {f['counts']}, usable points of the last frame {usable}")
    assert (m["segments"][:, 0]["count"] == 0).all(), "at init every weight is 1: nothing reaches min_weight 2"
    assert m["counts"][N_SEQ - 1] > 0, "the last sequence's promotions must keep something"
    assert (f["counts"] > 0).any() and (f["counts"] < m["counts"]).any(), "the voxel filter must keep something and drop something"
    w = mapped_run(mode, False)[-1]["weight"]
    assert ((w >= MIN_WEIGHT).any(axis=1) & (w < MIN_WEIGHT).any(axis=1)).any(), "no plane with weights on both sides of min_weight"


# ------------------------------------------------------------------------------------------------------------ 2
@MODES
def test_shadow_fusion_bit_for_bit(mode):
    import torch
    rows, cols, _ = SHAPES[mode]
    rec, frames = mapped_run(mode, False), frames_of(mode)
    shadow = V.Batch(config(mode), N_SEQ, rows, cols)
    counts = np.zeros(6, np.int64)
    d0 = frames[0][1].cpu().numpy().view(np.uint16)
    assert same_bits(rec[0]["depth"], d0) and same_bits(rec[0]["weight"], (d0 != 0).astype(np.uint8))
    for k in range(1, N_FRAMES):
        before, after = rec[k - 1], rec[k]
        promoted = np.nonzero(after["kf"] != before["kf"])[0]
        kept = np.nonzero(after["kf"] == before["kf"])[0]
        assert (after["stats"]["change_keyframe"][promoted] == 1).all() and (after["stats"]["change_keyframe"][kept] == 0).all()
        for s in kept:
            assert same_bits(after["depth"][s], before["depth"][s]) and same_bits(after["weight"][s], before["weight"][s]), f"frame {k} sequence {s} moved"
        if len(promoted) == 0:
            continue
        kf_gray = torch.stack([frames[before["kf"][s]][0][s] for s in promoted]).contiguous()
        kf_depth = torch.from_numpy(before["depth"][promoted].view(np.int16)).cuda()
        kf_weight = torch.from_numpy(before["weight"][promoted]).cuda()
        models = torch.from_numpy(np.ascontiguousarray(after["stats"]["lm_model"][promoted])).cuda()
        shadow.prepare_keyframes(kf_gray, kf_depth)
        m = shadow.fuse_depth(models, frames[k][1][promoted].contiguous(), TOL_M, kf_weight=kf_weight, max_weight=MAX_W, fill_min_weight=FILL, counts=True)
        torch.cuda.synchronize()
        assert same_bits(m["depth"].cpu().numpy().view(np.uint16), after["depth"][promoted]), f"frame {k}: fused depth differs from the shadow batch"
        assert same_bits(m["weight"].cpu().numpy(), after["weight"][promoted]), f"frame {k}: fused weight differs from the shadow batch"
        counts += m["counts"].cpu().numpy().sum(axis=0)
    assert counts[0] > 0 and counts[3] > 0 and counts[4] > 0 and counts[5] > 0, f"agree / measured only / filled / empty must all occur: {counts}"


# ------------------------------------------------------------------------------------------------------------ 3
@MODES
def test_shadow_map_bit_for_bit(mode):
    import torch
    rows, cols, _ = SHAPES[mode]
    rec, frames, cap = mapped_run(mode, False), frames_of(mode), capacity(mode)
    m = rec[-1]["map"]
    shadow = V.Batch(config(mode), N_SEQ, rows, cols)
    seen = np.zeros(N_SEQ, np.int64)     # segments checked per sequence
    total = np.zeros(N_SEQ, np.int64)    # points of the segments checked
    for k in range(N_FRAMES):
        new = np.arange(N_SEQ) if k == 0 else np.nonzero(rec[k]["kf"] != rec[k - 1]["kf"])[0]
        for s in (() if k == 0 else np.nonzero(rec[k]["kf"] == rec[k - 1]["kf"])[0]):
            assert written(rec[k]["map"], s) == written(rec[k - 1]["map"], s), f"frame {k} sequence {s}: the list of a sequence that did not promote moved"
        if len(new) == 0:
            continue
        assert (rec[k]["kf"][new] == k).all()
        gray = frames[k][0][new].contiguous()
        depth = torch.from_numpy(rec[k]["depth"][new].view(np.int16)).cuda()
        keep = torch.from_numpy((rec[k]["weight"][new] >= MIN_WEIGHT).astype(np.uint8)).cuda()
        shadow.prepare_keyframes(gray, depth)
        out = shadow.point_cloud(0, poses=torch.from_numpy(np.ascontiguousarray(rec[k]["poses"][new])).cuda(), keep=keep, capacity=cap, gray=True)
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
            assert rec[k]["map"]["counts"][s] == total[s] and rec[k]["map"]["n_segments"][s] == seen[s], f"{where}: running totals"
    assert (m["n_segments"] == seen).all() and (m["counts"] == total).all(), f"totals {m['counts']} / {m['n_segments']} against {total} / {seen}"
    assert total.max() <= cap, "the capacity of this run was meant to clip nothing"


# ------------------------------------------------------------------------------------------------------------ 4
@MODES
def test_voxel_filter_first_occurrence_bit_for_bit(mode):
    bare, rec = mapped_run(mode, False), mapped_run(mode, True)
    for k in range(N_FRAMES):
        for name in ("poses", "status", "kf", "depth", "weight") + (("stats",) if k else ()):
            assert same_bits(rec[k][name], bare[k][name]), f"frame {k}: {name} depend on the voxel filter"
        for s in (() if k == 0 else np.nonzero(rec[k]["kf"] == rec[k - 1]["kf"])[0]):
            assert written(rec[k]["map"], s) == written(rec[k - 1]["map"], s), f"frame {k} sequence {s}: the list of a sequence that did not promote moved"
    m, got = bare[-1]["map"], rec[-1]["map"]
    print(f"occupied {got['occupied']} of {SLOTS} slots, unfiltered {m['counts']}, overflow {got['overflow']}")
    assert (got["overflow"] == 0).all() and same_bits(got["occupied"], got["counts"])
    for s in range(N_SEQ):
        keys = V.voxel_keys(VOXEL_M[mode], m["xyz"][s, :int(m["counts"][s])])
        uniq, first = np.unique(keys, return_index=True)
        idx = np.sort(first[uniq != NONE])
        seg = m["segments"][s, :int(m["n_segments"][s])].copy()
        total = 0
        for j in range(len(seg)):
            a, b = int(seg[j]["first"]), int(seg[j]["first"]) + int(seg[j]["count"])
            kept = int(((idx >= a) & (idx < b)).sum())
            seg[j]["first"], seg[j]["count"] = total, kept
            total += kept
        assert got["counts"][s] == len(idx) and got["n_segments"][s] == len(seg), \
            f"sequence {s}: totals {got['counts'][s]} / {got['n_segments'][s]} against {len(idx)} / {len(seg)}"
        assert same_bits(got["segments"][s, :len(seg)], seg), f"sequence {s}: segment records\n{got['segments'][s, :len(seg)]}\n{seg}"
        for name in ("xyz", "pixel", "gray"):
            assert same_bits(got[name][s, :len(idx)], m[name][s][idx]), f"sequence {s}: {name} is not the first-occurrence filter of the unfiltered list"
