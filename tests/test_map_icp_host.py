"""The two rules of the map ICP correction at keyframe promotion on the host (vors_map_icp_window_host, vors_map_icp_verdict_host:
lie.h map_icp_window / map_icp_verdict, the texts the kernels run), the two new records as the ctypes mirror sees them, the pinned
refusals, and the stand-alone sanitizer check of both twins. No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vors_amd as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-odometry-rs_amd", "csrc")
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1], np.float32)


def segments(counts):
    seg = np.zeros(len(counts), V.MAP_SEGMENT_DTYPE)
    seg["frame"] = np.arange(len(counts))
    seg["count"] = counts
    seg["first"] = np.concatenate([[0], np.cumsum(counts)[:-1]]) if len(counts) else []
    return seg


def window(seg, n_segments, max_keyframes, count, capacity, last_keyframes):
    """The definition, restated."""
    n_rec, total = min(n_segments, max_keyframes), min(count, capacity)
    first = 0 if last_keyframes == 0 or n_rec <= last_keyframes else min(int(seg[n_rec - last_keyframes]["first"]), total)
    return first, total - first


# ------------------------------------------------------------------------------------------------------------ the window
@pytest.mark.parametrize("counts, max_keyframes, capacity", [
    ([100, 50, 70, 30], 16, 1000),          # everything recorded and stored
    ([100, 50, 70, 30], 16, 180),           # count > capacity: the last keyframes are dropped, a late first is clipped
    ([100, 50, 70, 30, 20, 10], 3, 1000),   # n_segments > max_keyframes: the later keyframes stay inside the window
    ([100, 50, 70, 30, 20, 10], 3, 120),
    ([0, 0, 40], 16, 1000),                 # empty keyframes
    ([], 16, 1000),                         # an empty map
    ([7], 1, 1),
    ([100, 0, 0, 40, 0], 5, 1000),          # empty recorded segments share their `first` with their successor; a trailing one sits at the total
    ([100, 0, 0, 40, 0], 3, 1000),          # ... and the last recorded segment is an empty one whose successor has no record
    ([100, 0, 0, 40, 0], 5, 50),            # a capacity inside segment 0: every later `first` lies above the total
    ([100, 0, 0, 40, 0], 3, 50),
    ([100, 0, 0, 40, 0], 5, 120),           # a capacity inside segment 3: the trailing empty segment's `first` lies above the total
    ([100, 0, 0, 40, 0], 3, 120),
    ([100, 50, 70, 30, 20, 10], 2, 90),     # n_segments > max_keyframes and a capacity below the last recorded `first`
])
def test_window_rule(counts, max_keyframes, capacity):
    seg, n_segments, count = segments(counts), len(counts), int(sum(counts))
    n_rec = min(n_segments, max_keyframes)
    for last in sorted({0, 1, 2, n_rec, n_rec + 1, 2 ** 31 - 1}):
        got = V.map_icp_window_host(seg[:n_rec], n_segments, max_keyframes, count, capacity, last)
        assert got == window(seg, n_segments, max_keyframes, count, capacity, last), (counts, max_keyframes, capacity, last)
        assert got[0] + got[1] == min(count, capacity)   # always to the end of the list
    if n_rec >= 2:
        assert V.map_icp_window_host(seg[:n_rec], n_segments, max_keyframes, count, capacity, 1)[0] == min(int(seg[n_rec - 1]["first"]), min(count, capacity))
    assert V.map_icp_window_host(None, n_segments, max_keyframes, count, capacity, 0) == (0, min(count, capacity))


@pytest.mark.parametrize("counts, max_keyframes, capacity, last_keyframes, want", [
    # the edges the cases above are meant to reach, written out by hand from the definition (no helper of this file enters)
    ([100, 0, 0, 40, 0], 5, 1000, 1, (140, 0)),    # the trailing empty segment: an empty window at the total
    ([100, 0, 0, 40, 0], 5, 1000, 2, (100, 40)),
    ([100, 0, 0, 40, 0], 5, 1000, 3, (100, 40)),   # an empty segment's `first` is its successor's
    ([100, 0, 0, 40, 0], 5, 1000, 4, (100, 40)),
    ([100, 0, 0, 40, 0], 5, 1000, 5, (0, 140)),
    ([100, 0, 0, 40, 0], 3, 1000, 1, (100, 40)),   # frozen at recorded segment 2, an empty one: the unrecorded keyframe 3 stays inside
    ([100, 0, 0, 40, 0], 3, 1000, 2, (100, 40)),
    ([100, 0, 0, 40, 0], 3, 1000, 3, (0, 140)),
    ([100, 0, 0, 40, 0], 5, 50, 1, (50, 0)),       # `first` 140 above a total of 50
    ([100, 0, 0, 40, 0], 5, 50, 4, (50, 0)),       # `first` 100 above a total of 50
    ([100, 0, 0, 40, 0], 3, 50, 1, (50, 0)),
    ([100, 0, 0, 40, 0], 3, 50, 0, (0, 50)),
    ([100, 0, 0, 40, 0], 5, 120, 1, (120, 0)),     # `first` 140 above a total of 120
    ([100, 0, 0, 40, 0], 5, 120, 2, (100, 20)),
    ([100, 0, 0, 40, 0], 3, 120, 1, (100, 20)),
    ([100, 50, 70, 30, 20, 10], 2, 90, 1, (90, 0)),     # the last recorded `first` is 100
    ([100, 50, 70, 30, 20, 10], 2, 90, 2, (0, 90)),
    ([100, 50, 70, 30, 20, 10], 3, 120, 1, (120, 0)),   # recorded segment 2 starts at 150
    ([100, 50, 70, 30, 20, 10], 3, 120, 2, (100, 20)),
])
def test_window_edges_written_out(counts, max_keyframes, capacity, last_keyframes, want):
    seg, n_segments, count = segments(counts), len(counts), int(sum(counts))
    n_rec = min(n_segments, max_keyframes)
    assert V.map_icp_window_host(seg[:n_rec], n_segments, max_keyframes, count, capacity, last_keyframes) == want
    assert window(seg, n_segments, max_keyframes, count, capacity, last_keyframes) == want


def test_window_saturated_count():
    seg = segments([10, 20])
    assert V.map_icp_window_host(seg, 2, 4, 0xFFFFFFFF, 25, 1) == (10, 15)
    assert V.map_icp_window_host(seg, 0xFFFFFFFF, 2, 30, 25, 1) == (10, 15)


# ------------------------------------------------------------------------------------------------------------ the verdict
PARAMS = dict(dist_m=0.05, min_match_ratio=0.5, max_rms=0.25, max_trans_m=0.5, max_rot_rad=0.5)


def stats(status=1, matched=500, considered=1000, rms=0.25):
    s = np.zeros(1, V.ICP_STATS_DTYPE)
    s[0] = (status, 3, considered, matched, rms, 0.0)
    return s[0]


def rot_z(angle):
    return np.array([0, 0, 0, 0, 0, np.sin(0.5 * angle), np.cos(0.5 * angle)], np.float32)


def test_every_verdict_in_its_priority():
    nan = np.float32("nan")
    far = np.array([1, 0, 0, 0, 0, 0, 1], np.float32)
    bad = np.array([nan, 0, 0, 0, 0, 0, 1], np.float32)
    v = lambda s, after, **kw: V.map_icp_verdict_host(dict(PARAMS, **kw), s, IDENTITY, after)
    assert v(stats(), IDENTITY) == V.MAP_ICP_ACCEPTED                                           # equality on the ratio and on the rms
    assert v(stats(status=0), IDENTITY) == V.MAP_ICP_ACCEPTED                                   # ITERATIONS
    # an input that fails every test gets the first; then one test fewer at a time
    assert v(stats(status=2, matched=0, rms=nan), bad) == V.MAP_ICP_NONFINITE
    assert v(stats(status=2, matched=0, rms=nan), far) == V.MAP_ICP_ICP_STATUS
    assert v(stats(status=3, matched=0, rms=nan), far) == V.MAP_ICP_ICP_STATUS
    assert v(stats(matched=499, rms=1.0), far) == V.MAP_ICP_FEW_MATCHES
    assert v(stats(rms=0.2500001), far) == V.MAP_ICP_RMS
    assert v(stats(), far) == V.MAP_ICP_STEP
    assert v(stats(), rot_z(1.0)) == V.MAP_ICP_STEP


def test_nan_in_each_field():
    nan, inf = np.float32("nan"), np.float32("inf")
    for i in range(7):
        for value in (nan, inf, -inf):
            after = IDENTITY.copy()
            after[i] = value
            assert V.map_icp_verdict_host(PARAMS, stats(), IDENTITY, after) == V.MAP_ICP_NONFINITE
    assert V.map_icp_verdict_host(PARAMS, stats(rms=nan), IDENTITY, IDENTITY) == V.MAP_ICP_RMS
    before = IDENTITY.copy()
    before[0] = nan   # a NaN start pose makes D non-finite: NaN fails the comparison
    assert V.map_icp_verdict_host(PARAMS, stats(), before, IDENTITY) == V.MAP_ICP_STEP


def test_equality_on_each_threshold_is_accepted():
    # exactly representable values: 0.5 m along x from the identity, dot3 = 0.25 = 0.5 * 0.5
    at = np.array([0.5, 0, 0, 0, 0, 0, 1], np.float32)
    beyond = np.array([np.nextafter(np.float32(0.5), np.float32(1)), 0, 0, 0, 0, 0, 1], np.float32)
    assert V.map_icp_verdict_host(PARAMS, stats(), IDENTITY, at) == V.MAP_ICP_ACCEPTED
    assert V.map_icp_verdict_host(PARAMS, stats(), IDENTITY, beyond) == V.MAP_ICP_STEP
    assert V.map_icp_verdict_host(dict(PARAMS, min_match_ratio=1.0), stats(matched=1000), IDENTITY, IDENTITY) == V.MAP_ICP_ACCEPTED
    assert V.map_icp_verdict_host(dict(PARAMS, min_match_ratio=0.0), stats(matched=0, considered=0, rms=0.0), IDENTITY, IDENTITY) == V.MAP_ICP_ACCEPTED
    assert V.map_icp_verdict_host(dict(PARAMS, max_rms=0.0), stats(rms=0.0), IDENTITY, IDENTITY) == V.MAP_ICP_ACCEPTED
    # the rotation bound: |D.q.w| against the host's cosf(0.5f * max_rot_rad), the float the library itself computes
    c = np.cos(np.float32(0.25), dtype=np.float32)
    for w, want in ((c, V.MAP_ICP_ACCEPTED), (np.nextafter(c, np.float32(0)), V.MAP_ICP_STEP), (-c, V.MAP_ICP_ACCEPTED)):
        after = np.array([0, 0, 0, 0, 0, 0, w], np.float32)   # (the rule reads w alone: no renormalisation enters)
        got = V.map_icp_verdict_host(PARAMS, stats(), IDENTITY, after)
        # numpy's float32 cosine and the C library's may differ in the last bit: then the neighbouring value decides identically
        if np.float32(c) == np.float32(np.cos(0.25)):
            assert got == want, (w, got)


def test_rotation_at_zero_and_pi():
    quarter = rot_z(np.pi / 2)
    zero, pi = dict(PARAMS, max_rot_rad=0.0), dict(PARAMS, max_rot_rad=float(np.float32(np.pi)))
    assert V.map_icp_verdict_host(zero, stats(), IDENTITY, IDENTITY) == V.MAP_ICP_ACCEPTED   # |w| = 1 >= cosf(0) = 1
    assert V.map_icp_verdict_host(zero, stats(), IDENTITY, rot_z(1e-3)) == V.MAP_ICP_STEP
    assert V.map_icp_verdict_host(zero, stats(), IDENTITY, quarter) == V.MAP_ICP_STEP
    half = np.array([0, 0, 0, 0, 0, 1, 0], np.float32)   # a half turn: w = 0 >= cosf(pi / 2) = -4.4e-8
    for after in (IDENTITY, quarter, -quarter, half):
        assert V.map_icp_verdict_host(pi, stats(), IDENTITY, after) == V.MAP_ICP_ACCEPTED
    assert V.map_icp_verdict_host(dict(PARAMS, max_rot_rad=1.5), stats(), IDENTITY, -quarter) == V.MAP_ICP_STEP
    assert V.map_icp_verdict_host(dict(PARAMS, max_rot_rad=1.6), stats(), IDENTITY, -quarter) == V.MAP_ICP_ACCEPTED


# ------------------------------------------------------------------------------------------------------------ structs, refusals
def test_struct_layouts():
    p, r = V.vors_map_icp_params, V.vors_map_icp_record
    assert C.sizeof(p) == 52
    assert [getattr(p, n).offset for n, _ in p._fields_] == list(range(0, 52, 4))
    assert [n for n, _ in p._fields_] == ["dist_m", "damping", "step_eps", "iters", "min_points", "normal_gate", "min_cos", "huber_m", "last_keyframes",
                                          "min_match_ratio", "max_rms", "max_trans_m", "max_rot_rad"]
    assert C.sizeof(r) == 112 == V.MAP_ICP_RECORD_DTYPE.itemsize
    offsets = dict(frame=0, verdict=4, range_first=8, range_count=12, stats=16, gate_counts=40, pose_before=56, pose_after=84)
    assert {n: getattr(r, n).offset for n, _ in r._fields_} == offsets
    assert {n: V.MAP_ICP_RECORD_DTYPE.fields[n][1] for n in V.MAP_ICP_RECORD_DTYPE.names} == offsets
    assert (V.MAP_ICP_NOT_ATTEMPTED, V.MAP_ICP_ACCEPTED, V.MAP_ICP_ICP_STATUS, V.MAP_ICP_FEW_MATCHES, V.MAP_ICP_RMS, V.MAP_ICP_STEP,
            V.MAP_ICP_NONFINITE) == (0, 1, 2, 3, 4, 5, 6)
    hdr = open(os.path.join(ROOT, "include", "vors_hip.h")).read()
    for name, value in (("NOT_ATTEMPTED", 0), ("ACCEPTED", 1), ("ICP_STATUS", 2), ("FEW_MATCHES", 3), ("RMS", 4), ("STEP", 5), ("NONFINITE", 6)):
        assert f"#define VORS_MAP_ICP_{name}" in hdr and int(hdr.split(f"#define VORS_MAP_ICP_{name}")[1].split()[0]) == value


def test_refusals_of_the_host_twins():
    seg = segments([10, 20, 30])
    for args, sentence in (((seg, 3, 4, 60, 0, 0), "map_icp_window_host: capacity must be >= 1"),
                           ((seg, 3, 0, 60, 100, 0), "map_icp_window_host: max_keyframes must be >= 1"),
                           ((seg, 3, 4, 60, 100, -1), "map_icp_window_host: last_keyframes must be >= 0 (0 = the whole map)"),
                           ((None, 3, 4, 60, 100, 1), "map_icp_window_host: segments is NULL where a record is read")):
        with pytest.raises(V.VorsError) as e:
            V.map_icp_window_host(*args)
        assert str(e.value).endswith(sentence)
    assert V.lib().vors_map_icp_window_host(None, 0, 4, 0, 10, 0, None) == -1 and V.lib().vors_last_error() == b"map_icp_window_host: range2 is NULL"
    nan = float("nan")
    for kw, sentence in ((dict(min_match_ratio=-0.1), "min_match_ratio must lie in [0, 1] (and not be NaN)"),
                         (dict(min_match_ratio=1.1), "min_match_ratio must lie in [0, 1] (and not be NaN)"),
                         (dict(min_match_ratio=nan), "min_match_ratio must lie in [0, 1] (and not be NaN)"),
                         (dict(max_rms=-1.0), "max_rms must be >= 0 (and not NaN)"), (dict(max_rms=nan), "max_rms must be >= 0 (and not NaN)"),
                         (dict(max_trans_m=-1.0), "max_trans_m must be >= 0 (and not NaN)"), (dict(max_trans_m=nan), "max_trans_m must be >= 0 (and not NaN)"),
                         (dict(max_rot_rad=-1.0), "max_rot_rad must be >= 0 (and not NaN)"), (dict(max_rot_rad=nan), "max_rot_rad must be >= 0 (and not NaN)")):
        with pytest.raises(V.VorsError) as e:
            V.map_icp_verdict_host(dict(PARAMS, **kw), stats(), IDENTITY, IDENTITY)
        assert str(e.value).endswith("map_icp_verdict_host: " + sentence)
    p = V.map_icp_params(**PARAMS)
    assert V.lib().vors_map_icp_verdict_host(C.byref(p), None, None, None, None) == -1
    assert V.lib().vors_last_error() == b"map_icp_verdict_host: a NULL argument (params, stats, pose_before, pose_after, verdict)"
    with pytest.raises(V.VorsError, match="dist_m is required"):
        V.map_icp_params()
    with pytest.raises(V.VorsError, match="unknown parameter 'max_rot'"):
        V.map_icp_params(dist_m=0.05, max_rot=1.0)
    with pytest.raises(V.VorsError, match="iters must be an integer"):
        V.map_icp_params(dist_m=0.05, iters=2.5)


def test_new_symbols_are_exported():
    lib = V.lib()
    for name in ("vors_trackers_enable_map_icp", "vors_trackers_map_icp", "vors_tracker_enable_map_icp", "vors_tracker_read_map_icp",
                 "vors_map_icp_window_host", "vors_map_icp_verdict_host"):
        assert hasattr(lib, name) and name in V.EXPORTED_SYMBOLS
    assert lib.vors_trackers_enable_map_icp(None, None) == -1 and lib.vors_last_error() == b"enable_map_icp: the handle t is NULL"
    assert lib.vors_tracker_enable_map_icp(None, None) == -1 and lib.vors_last_error() == b"enable_map_icp: the handle t is NULL"
    assert lib.vors_trackers_map_icp(None, None, None) == -1 and lib.vors_tracker_read_map_icp(None, None, None) == -1


# ------------------------------------------------------------------------------------------------------------ sanitizer
def test_host_twins_under_the_sanitizers():
    """A stand-alone program (its own main) built with -fsanitize=address,undefined drives both twins; nothing is loaded into Python."""
    subprocess.check_call(["make", "-C", CSRC, "-s", "map_icp_host_check"])
    out = subprocess.run([os.path.join(CSRC, "map_icp_host_check")], capture_output=True, text=True)
    assert out.returncode == 0 and "map_icp_host_check: ok" in out.stdout, out.stdout + out.stderr
