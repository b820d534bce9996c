"""The refusals of vors_icp_points_robust, vors_icp_points_robust_host and vors_trackers_icp_map_robust's NULL handle: everything the plain
entries refuse (the sentences of tests/test_icp_args.py, restated) and what the robust arguments add. One fault per case, whole messages
compared with ==, every output buffer seen to be untouched. Needs no GPU: the device entry refuses before it asks for the device, and a
refused call touches none of its pointers."""
import numpy as np
import pytest

import vors_amd as V

INVALID = -1
ROWS, COLS, CAP, N = 6, 8, 16, 2
NAN = float("nan")
# (64-bit items: every base address is 8-byte aligned, so `+ 1` and `+ 2` below are misaligned for certain)
XYZ = np.zeros(N * CAP * 3, np.float64)
NORMALS = np.zeros(N * CAP * 3, np.float64)
COUNTS = np.zeros(N, np.uint64)
RANGES = np.zeros(N * 2, np.uint64)
POSES = np.zeros(N * 7, np.float64)
DEPTH = np.zeros(N * ROWS * COLS, np.uint64)
FRAME_NORMALS = np.zeros(N * ROWS * COLS * 3, np.float64)
CAM5 = np.array([3.5, 2.5, 9.0, 9.5, 0.0], np.float32)
WS = np.zeros(1024, np.uint64)
OUT = np.zeros(N * 7, np.float64)
STATS = np.zeros(N * 6, np.uint64)
SUMS = np.zeros(N * 29, np.float64)
RES = np.zeros(N * CAP, np.float64)
GATES = np.zeros(N * 4, np.uint64)
OUTPUTS = (OUT, STATS, SUMS, RES, GATES, WS)


def at(a, offset=0):
    return a.ctypes.data + offset


def last_error():
    return V.lib().vors_last_error().decode()


GOOD = dict(n=N, xyz=at(XYZ), normals=at(NORMALS), counts=at(COUNTS), capacity=CAP, ranges=at(RANGES), range_stride=0, poses=at(POSES),
            pose_stride=0, depth=at(DEPTH), cam5=at(CAM5), rows=ROWS, cols=COLS, depth_scale=5000.0, dist_m=0.1, damping=0.0, step_eps=1e-5,
            iters=4, min_points=6, frame_normals=at(FRAME_NORMALS), min_cos=0.5, huber_m=0.01, ws=at(WS), out=at(OUT), stats=at(STATS),
            sums=at(SUMS), res=at(RES), gates=at(GATES))


def device_call(**kw):
    a = dict(GOOD, **kw)
    return V.lib().vors_icp_points_robust(a["n"], a["xyz"], a["normals"], a["counts"], a["capacity"], a["ranges"], a["range_stride"], a["poses"],
                                          a["pose_stride"], a["depth"], a["cam5"], a["rows"], a["cols"], a["depth_scale"], a["dist_m"],
                                          a["damping"], a["step_eps"], a["iters"], a["min_points"], a["frame_normals"], a["min_cos"], a["huber_m"],
                                          a["ws"], a["out"], a["stats"], a["sums"], a["res"], a["gates"], None)


def host_call(**kw):
    a = dict(GOOD, **kw)
    return V.lib().vors_icp_points_robust_host(a["xyz"], a["normals"], 3, a["capacity"], a["ranges"], a["poses"], a["depth"], a["cam5"], a["rows"],
                                               a["cols"], a["depth_scale"], a["dist_m"], a["damping"], a["step_eps"], a["iters"], a["min_points"],
                                               a["frame_normals"], a["min_cos"], a["huber_m"], a["out"], a["stats"], a["sums"], a["res"], a["gates"])


# what both entries refuse, with the sentence after "<who>: ": the plain entries' list, then the robust arguments
SHARED = [
    (dict(xyz=None), "a list (xyz, normals) is NULL"),
    (dict(normals=None), "a list (xyz, normals) is NULL"),
    (dict(poses=None), "the start poses are NULL (an alignment needs a pose to refine)"),
    (dict(depth=None), "depth is NULL"),
    (dict(cam5=None), "cam5 is NULL"),
    (dict(out=None), "the output poses are NULL"),
    (dict(rows=0), "rows and cols must be >= 1"),
    (dict(cols=-3), "rows and cols must be >= 1"),
    (dict(capacity=0), "capacity must be >= 1"),
    (dict(rows=65536), "rows / cols must not exceed 65535 and rows * cols must not exceed 2^28 pixels"),
    (dict(rows=32768, cols=16384), "rows / cols must not exceed 65535 and rows * cols must not exceed 2^28 pixels"),
    (dict(depth_scale=0.0), "depth_scale must be > 0"),
    (dict(depth_scale=NAN), "depth_scale must be > 0"),
    (dict(dist_m=-1.0), "dist_m must be >= 0 (and not NaN)"),
    (dict(dist_m=NAN), "dist_m must be >= 0 (and not NaN)"),
    (dict(damping=-0.5), "damping must be >= 0 (and not NaN)"),
    (dict(damping=NAN), "damping must be >= 0 (and not NaN)"),
    (dict(step_eps=-1e-9), "step_eps must be >= 0 (and not NaN)"),
    (dict(step_eps=NAN), "step_eps must be >= 0 (and not NaN)"),
    (dict(iters=-1), "iters must be in 0..64"),
    (dict(iters=65), "iters must be in 0..64"),
    (dict(min_points=5), "min_points must be >= 6 (a pose has six degrees of freedom)"),
    (dict(depth=at(DEPTH, 1)), "depth must be 2-byte aligned"),
] + [(dict([(k, at(a, 2))]), "xyz, normals, the poses, stats, sums29 and residuals must be 4-byte aligned")
     for k, a in (("xyz", XYZ), ("normals", NORMALS), ("poses", POSES), ("out", OUT), ("stats", STATS), ("sums", SUMS), ("res", RES))] + [
    (dict(min_cos=NAN), "min_cos must lie in [-1, 1] (and not be NaN)"),
    (dict(min_cos=1.0001), "min_cos must lie in [-1, 1] (and not be NaN)"),
    (dict(min_cos=-1.5), "min_cos must lie in [-1, 1] (and not be NaN)"),
    (dict(huber_m=-1e-6), "huber_m must be >= 0 (and not NaN; 0 = no Huber weight)"),
    (dict(huber_m=NAN), "huber_m must be >= 0 (and not NaN; 0 = no Huber weight)"),
    (dict(frame_normals=at(FRAME_NORMALS, 2)), "the frame normals and the gate counts must be 4-byte aligned"),
    (dict(gates=at(GATES, 2)), "the frame normals and the gate counts must be 4-byte aligned"),
]


def refused(call, fault, message):
    for o in OUTPUTS:
        o[:] = 7
    assert call(**fault) == INVALID
    assert last_error() == message
    assert all((o == 7).all() for o in OUTPUTS)  # nothing written


@pytest.mark.parametrize("who, call", [("icp_points_robust", device_call), ("icp_points_robust_host", host_call)])
@pytest.mark.parametrize("k", range(len(SHARED)))
def test_shared_refusals(who, call, k):
    fault, sentence = SHARED[k]
    refused(call, fault, f"{who}: {sentence}")


DEVICE_ONLY = [
    (dict(n=0), "n must be >= 1"),
    (dict(counts=None), "a list (d_list_counts) is NULL"),
    (dict(ws=None), "d_workspace is NULL (the pass allocates nothing: vors_icp_workspace_bytes)"),
    (dict(pose_stride=24), "pose_stride_bytes must be 0 or a multiple of 4 of at least 28"),
    (dict(pose_stride=30), "pose_stride_bytes must be 0 or a multiple of 4 of at least 28"),
    (dict(range_stride=4), "range_stride_bytes must be 0 or a multiple of 4 of at least 8"),
    (dict(range_stride=10), "range_stride_bytes must be 0 or a multiple of 4 of at least 8"),
    (dict(ranges=at(RANGES, 2)), "d_ranges, d_list_counts and d_workspace must be 4-byte aligned"),
    (dict(counts=at(COUNTS, 2)), "d_ranges, d_list_counts and d_workspace must be 4-byte aligned"),
    (dict(ws=at(WS, 1)), "d_ranges, d_list_counts and d_workspace must be 4-byte aligned"),
]


@pytest.mark.parametrize("k", range(len(DEVICE_ONLY)))
def test_device_entry_refusals(k):
    fault, sentence = DEVICE_ONLY[k]
    refused(device_call, fault, f"icp_points_robust: {sentence}")


def test_the_bounds_themselves_and_the_nullable_arguments_are_accepted_on_the_host():
    for ok in (dict(min_cos=-1.0), dict(min_cos=1.0), dict(huber_m=0.0), dict(frame_normals=None), dict(gates=None),
               dict(stats=None, sums=None, res=None, ranges=None, gates=None, frame_normals=None)):
        assert host_call(**ok) == 0, ok


def test_icp_map_robust_refuses_a_null_handle():
    assert V.lib().vors_trackers_icp_map_robust(None, at(DEPTH), 0.1, 0.0, 1e-5, 4, 6, None, 0, None, 0, at(FRAME_NORMALS), 0.5, 0.01, at(WS), at(OUT),
                                                None, None, None, at(GATES), None) == INVALID
    assert last_error() == "icp_map: the handle t is NULL"


def test_python_layer():
    assert V.ICP_GATE_COUNTS == 4
    with pytest.raises(V.VorsError):  # a plane of frame normals of another shape
        V.icp_points_robust_host(np.zeros((4, 3)), np.zeros((4, 3)), np.zeros((3, 3), np.uint16), CAM5, 5000.0, np.zeros(7), 0.1,
                                 frame_normals=np.zeros((3, 4, 3), np.float32))
