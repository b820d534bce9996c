"""Normals of the trackers' keyframe map (vors_trackers_enable_map_normals, vors_trackers_map_normals, vors_tracker_enable_map_normals,
vors_tracker_read_map_normals): every map entry carries the surface normal of its pixel in its keyframe's depth plane. GPU only.

  1. every segment's normals equal the host entry (vors_depth_normals_host, list form) on that keyframe's depth plane — the input frame,
     with the depth filter the plane vors_trackers_keyframe_depth showed after that track call — with the segment's pose, bit for bit
  2. clipping at a small capacity     3. normals on / off: tracking and the map keep their bits
  4. Tracker(map_normals=...) == a one-sequence handle     5. workspace bytes and the enable-order refusals

Frames, modes, shapes and helpers are those of tests/test_gpu_trackers_map.py; the first N_USED of its frames, which is enough for
promotions (asserted).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from test_gpu_trackers_map import ARITHS, FILTER, MAX_KF, MODES, N_SEQ, SHAPES, config, frames_of, promotions, read_map, same_bits

N_USED = 5
STEP, JUMP_M = 2, 0.05
SLOTS = 1 << 16
VOXEL_M = {V.CANDIDATES_DENSE: 0.02, V.CANDIDATES_COARSE_TO_FINE: 0.10, V.CANDIDATES_DSO: 0.10}
# (depth filter, voxel filter) of a run
VARIANTS = {"plain": (None, False), "filter": (FILTER, False), "voxels": (None, True)}
VARIANT = pytest.mark.parametrize("variant", list(VARIANTS))


def capacity_of(mode):
    rows, cols, _ = SHAPES[mode]
    return rows * cols * N_USED


def run(mode, arith, variant, with_normals, capacity=None, seqs=None):
    """-> (per frame a dict of host arrays, the map, the normals [n, capacity, 3] or None, workspace bytes before / after the switch)."""
    import torch
    rows, cols, _ = SHAPES[mode]
    depth_filter, voxels = VARIANTS[variant]
    cap = capacity_of(mode) if capacity is None else capacity
    sel = (lambda t: t) if seqs is None else (lambda t: t[seqs].contiguous())
    n = N_SEQ if seqs is None else len(seqs)
    tr = V.Trackers(config(mode, arith), n, rows, cols)
    if depth_filter is not None:
        tr.enable_depth_filter(*depth_filter)
    tr.enable_map(0, cap, MAX_KF, 0)
    if voxels:
        tr.enable_map_voxels(VOXEL_M[mode], SLOTS)
    before = tr.workspace_bytes()
    if with_normals:
        tr.enable_map_normals(STEP, JUMP_M)
    after = tr.workspace_bytes()
    rec = []
    for k, (g, d) in enumerate(frames_of(mode)[:N_USED]):
        g, d = sel(g), sel(d)
        if k == 0:
            tr.init(g, d)
        else:
            tr.track(g, d)
        poses, status, kf = tr.current_frames()
        r = dict(poses=poses, status=status, kf=kf, stats=tr.stats().copy() if k else None)
        if depth_filter is not None:
            r["depth"] = tr.keyframe_depth()[0].cpu().numpy().view(np.uint16)
        rec.append(r)
    normals = tr.map_normals().cpu().numpy() if with_normals else None
    torch.cuda.synchronize()
    assert tr.workspace_bytes() == after, "no call after the switch allocates"
    return rec, read_map(tr), normals, (before, after)


cached_run = functools.lru_cache(maxsize=None)(run)


def expected_normals(mode, rec, m, cap):
    """[n, cap, 3] from the host entry, segment by segment; -> (normals, written [n, cap] bool)."""
    rows, cols, _ = SHAPES[mode]
    frames = frames_of(mode)
    intr = np.array(V.scaled_intrinsics(rows, cols), np.float32)
    n = len(m["counts"])
    want, written = np.zeros((n, cap, 3), np.float32), np.zeros((n, cap), bool)
    for s in range(n):
        for j in range(min(int(m["n_segments"][s]), MAX_KF)):
            seg = m["segments"][s, j]
            k = int(seg["frame"])
            plane = rec[k]["depth"][s] if "depth" in rec[k] else frames[k][1][s].cpu().numpy().view(np.uint16)
            a, b = min(int(seg["first"]), cap), min(int(seg["first"]) + int(seg["count"]), cap)
            if b > a:
                o = V.depth_normals_host(plane, intr, V.DEPTH_SCALE, STEP, JUMP_M, pose7=seg["pose7"], pixel=m["pixel"][s, a:b])
                want[s, a:b] = o["normals"]
                written[s, a:b] = True
    return want, written


# ------------------------------------------------------------------------------------------------------------ 1
@MODES
@ARITHS
@VARIANT
def test_segments_equal_the_host_entry(mode, arith, variant):
    rec, m, normals, _ = cached_run(mode, arith, variant, True)
    cap = capacity_of(mode)
    p = promotions(rec)
    assert p.any(), "no sequence promotes: the masked launch was never exercised"
    assert (p.sum(axis=1) < N_SEQ).all(), "every launch after init is a partial promotion here"
    assert (m["counts"] <= cap).all() and (m["counts"] > 0).all() and (m["n_segments"] <= MAX_KF).all()
    want, written = expected_normals(mode, rec, m, cap)
    for s in range(N_SEQ):
        assert written[s, :int(m["counts"][s])].all() and not written[s, int(m["counts"][s]):].any()
        k = int(m["counts"][s])
        assert np.array_equal(normals[s, :k].view(np.uint32), want[s, :k].view(np.uint32)), f"sequence {s}: normals differ from the host entry"
    have = want[written].any(axis=-1)
    assert 2 * int(have.sum()) >= int(written.sum()), "fewer than half of the map's points get a normal"
    unit = np.linalg.norm(want[written][have].astype(np.float64), axis=-1)
    assert np.abs(unit - 1.0).max() <= 1e-6


# ------------------------------------------------------------------------------------------------------------ 2
@MODES
def test_clipping_at_a_small_capacity(mode):
    arith = V.ARITH_FUSED
    _, big, big_normals, _ = cached_run(mode, arith, "plain", True)
    s = int(np.argmax(big["n_segments"]))
    assert big["n_segments"][s] >= 2
    # inside the sequence's second keyframe: keyframe 0 whole, keyframe 1 cut, the later ones entirely beyond
    cap = int(big["segments"][s, 1]["first"]) + int(big["segments"][s, 1]["count"]) // 2
    rec, m, normals, _ = run(mode, arith, "plain", True, capacity=cap)
    assert same_bits(m["counts"], big["counts"]) and (m["counts"] > cap).any()
    for q in range(N_SEQ):
        k = min(int(m["counts"][q]), cap)
        assert same_bits(m["pixel"][q, :k], big["pixel"][q, :k])
        assert np.array_equal(normals[q, :k].view(np.uint32), big_normals[q, :k].view(np.uint32)), f"sequence {q}: the written prefix differs"
    want, written = expected_normals(mode, rec, m, cap)
    assert np.array_equal(normals[written].view(np.uint32), want[written].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ 3
@MODES
@ARITHS
@VARIANT
def test_normals_only_read(mode, arith, variant):
    on, m_on, _, _ = cached_run(mode, arith, variant, True)
    off, m_off, _, _ = cached_run(mode, arith, variant, False)
    for a, b in zip(on, off):
        for name in a:
            assert (a[name] is None and b[name] is None) or same_bits(a[name], b[name]), f"{name} depends on the normals"
    for name in ("counts", "n_segments"):
        assert same_bits(m_on[name], m_off[name])
    for s in range(N_SEQ):
        k, j = int(m_on["counts"][s]), int(m_on["n_segments"][s])
        assert same_bits(m_on["segments"][s, :j], m_off["segments"][s, :j])
        for name in ("xyz", "pixel", "gray"):
            assert same_bits(m_on[name][s, :k], m_off[name][s, :k]), f"sequence {s}: {name} depends on the normals"


# ------------------------------------------------------------------------------------------------------------ 4
@MODES
@pytest.mark.parametrize("variant", ["plain", "filter"])
def test_single_tracker_equals_one_sequence_handle(mode, variant):
    arith, s = V.ARITH_FUSED, 4
    depth_filter, _ = VARIANTS[variant]
    cap = capacity_of(mode)
    many, m, normals, _ = run(mode, arith, variant, True, seqs=[s])
    host = [(g[s].cpu().numpy(), d[s].cpu().numpy().view(np.uint16)) for g, d in frames_of(mode)[:N_USED]]
    one = V.Tracker(config(mode, arith), 0.0, host[0][1], 0.0, host[0][0], depth_filter=depth_filter, map=(0, cap, MAX_KF, 0),
                    map_normals=(STEP, JUMP_M))
    first = one.read_map_normals()   # keyframe 0's normals come from the switch itself
    k0 = int(m["segments"][0, 0]["count"])
    assert len(first) == k0 and np.array_equal(first.view(np.uint32), normals[0, :k0].view(np.uint32))
    for k in range(1, N_USED):
        assert one.track(float(k), host[k][1], float(k), host[k][0]) == many[k]["status"][0]
    total = int(m["counts"][0])
    assert m["n_segments"][0] >= 2 and one.read_map()["count"] == total
    got = one.read_map_normals()
    assert len(got) == total and np.array_equal(got.view(np.uint32), normals[0, :total].view(np.uint32))
    part = one.read_map_normals(capacity=total // 2)
    assert len(part) == total // 2 and np.array_equal(part.view(np.uint32), got[:total // 2].view(np.uint32))
    with pytest.raises(V.VorsError, match="already"):
        V._check(V.lib().vors_tracker_enable_map_normals(one._h, STEP, JUMP_M))
    late = V.Tracker(config(mode, arith), 0.0, host[0][1], 0.0, host[0][0], map=(0, cap, MAX_KF, 0))
    late.track(1.0, host[1][1], 1.0, host[1][0])
    with pytest.raises(V.VorsError, match="before the first"):   # the switch is legal until the first track only
        V._check(V.lib().vors_tracker_enable_map_normals(late._h, STEP, JUMP_M))


# ------------------------------------------------------------------------------------------------------------ 5
def test_workspace_bytes_and_refusals():
    mode = V.CANDIDATES_COARSE_TO_FINE
    rows, cols, _ = SHAPES[mode]
    cfg, frames = config(mode, V.ARITH_FUSED), frames_of(mode)
    _, _, _, (before, after) = cached_run(mode, V.ARITH_FUSED, "plain", True)
    assert after == before + N_SEQ * capacity_of(mode) * 12 + 4 * N_SEQ
    t = V.Trackers(cfg, N_SEQ, rows, cols)
    with pytest.raises(V.VorsError, match="keyframe map first"):
        t.enable_map_normals(STEP, JUMP_M)
    with pytest.raises(V.VorsError, match="not enabled"):
        V._check(V.lib().vors_trackers_map_normals(t._h, None))
    t.enable_map(1, 1000, 4)
    with pytest.raises(V.VorsError, match="level 0"):
        t.enable_map_normals(STEP, JUMP_M)
    t = V.Trackers(cfg, N_SEQ, rows, cols)
    t.enable_map(0, 1000, 4)
    base = t.workspace_bytes()
    for bad, word in (((0, 0.1), "step"), ((9, 0.1), "step"), ((1, -0.5), "jump_m"), ((1, float("nan")), "jump_m")):
        with pytest.raises(V.VorsError, match=word):
            t.enable_map_normals(*bad)
    assert t.workspace_bytes() == base   # a refused call allocates nothing
    t.enable_map_normals(STEP, JUMP_M)
    assert t.workspace_bytes() == base + N_SEQ * 1000 * 12 + 4 * N_SEQ
    with pytest.raises(V.VorsError, match="already"):
        t.enable_map_normals(STEP, JUMP_M)
    late = V.Trackers(cfg, N_SEQ, rows, cols)
    late.enable_map(0, 1000, 4)
    late.init(*frames[0])
    with pytest.raises(V.VorsError, match="before vors_trackers_init"):
        late.enable_map_normals(STEP, JUMP_M)
    lib = V.lib()
    assert lib.vors_trackers_enable_map_normals(None, 1, 0.1) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_trackers_map_normals(None, None) == -1 and lib.vors_tracker_enable_map_normals(None, 1, 0.1) == -1
    assert lib.vors_tracker_read_map_normals(None, 0, None) == -1
    # the single tracker: the voxel filter re-emits keyframe 0, so it must come before the normals
    host = (frames[0][0][0].cpu().numpy(), frames[0][1][0].cpu().numpy().view(np.uint16))
    one = V.Tracker(cfg, 0.0, host[1], 0.0, host[0], map=(0, 50000, 4), map_normals=(STEP, JUMP_M))
    with pytest.raises(V.VorsError, match="before vors_tracker_enable_map_normals"):
        V._check(lib.vors_tracker_enable_map_voxels(one._h, 0.1, SLOTS))
    both = V.Tracker(cfg, 0.0, host[1], 0.0, host[0], map=(0, 50000, 4), map_voxels=(0.1, SLOTS), map_normals=(STEP, JUMP_M))
    assert len(both.read_map_normals()) == both.read_map()["count"] > 0
