"""The refusals of vors_icp_points_joint, vors_icp_points_joint_host and vors_trackers_icp_map_joint's NULL handle: everything the robust
entries refuse (the sentences of tests/test_icp_robust_args.py, whose table is reused) and what the joint arguments add. One fault per
case, whole messages compared with ==, every output buffer seen to be untouched. Needs no GPU: the device entry refuses before it asks for
the device, and a refused call touches none of its pointers."""
import numpy as np
import pytest

import vors_amd as V
from test_icp_robust_args import (CAM5, CAP, COLS, COUNTS, DEPTH, DEVICE_ONLY, FRAME_NORMALS, GATES, INVALID, N, NAN, NORMALS, OUT, POSES, RANGES, RES,
                                  ROWS, SHARED, STATS, SUMS, WS, XYZ, at, last_error)

LIST_GRAY = np.zeros(N * CAP, np.uint64)
FRAME_GRAY = np.zeros(N * ROWS * COLS, np.uint64)
PHOTO_RES = np.zeros(N * CAP, np.float64)
PHOTO_COUNTS = np.zeros(N * 2, np.uint64)
OUTPUTS = (OUT, STATS, SUMS, RES, GATES, WS, PHOTO_RES, PHOTO_COUNTS)

GOOD = dict(n=N, xyz=at(XYZ), normals=at(NORMALS), list_gray=at(LIST_GRAY), counts=at(COUNTS), capacity=CAP, ranges=at(RANGES), range_stride=0,
            poses=at(POSES), pose_stride=0, depth=at(DEPTH), frame_gray=at(FRAME_GRAY), cam5=at(CAM5), rows=ROWS, cols=COLS, depth_scale=5000.0,
            dist_m=0.1, damping=0.0, step_eps=1e-5, iters=4, min_points=6, frame_normals=at(FRAME_NORMALS), min_cos=0.5, huber_m=0.01,
            photo_scale_m=0.0005, photo_huber_grey=10.0, ws=at(WS), out=at(OUT), stats=at(STATS), sums=at(SUMS), res=at(RES), gates=at(GATES),
            photo_res=at(PHOTO_RES), photo_counts=at(PHOTO_COUNTS))


def device_call(**kw):
    a = dict(GOOD, **kw)
    return V.lib().vors_icp_points_joint(a["n"], a["xyz"], a["normals"], a["list_gray"], a["counts"], a["capacity"], a["ranges"], a["range_stride"],
                                         a["poses"], a["pose_stride"], a["depth"], a["frame_gray"], a["cam5"], a["rows"], a["cols"],
                                         a["depth_scale"], a["dist_m"], a["damping"], a["step_eps"], a["iters"], a["min_points"], a["frame_normals"],
                                         a["min_cos"], a["huber_m"], a["photo_scale_m"], a["photo_huber_grey"], a["ws"], a["out"], a["stats"],
                                         a["sums"], a["res"], a["gates"], a["photo_res"], a["photo_counts"], None)


def host_call(**kw):
    a = dict(GOOD, **kw)
    return V.lib().vors_icp_points_joint_host(a["xyz"], a["normals"], a["list_gray"], 3, a["capacity"], a["ranges"], a["poses"], a["depth"],
                                              a["frame_gray"], a["cam5"], a["rows"], a["cols"], a["depth_scale"], a["dist_m"], a["damping"],
                                              a["step_eps"], a["iters"], a["min_points"], a["frame_normals"], a["min_cos"], a["huber_m"],
                                              a["photo_scale_m"], a["photo_huber_grey"], a["out"], a["stats"], a["sums"], a["res"], a["gates"],
                                              a["photo_res"], a["photo_counts"])


# what both entries refuse, with the sentence after "<who>: ": the robust entries' list, then the joint arguments
JOINT = SHARED + [
    (dict(photo_scale_m=-1e-6), "photo_scale_m must be >= 0 (and not NaN; 0 = no photometric term)"),
    (dict(photo_scale_m=NAN), "photo_scale_m must be >= 0 (and not NaN; 0 = no photometric term)"),
    (dict(photo_huber_grey=-1.0), "photo_huber_grey must be >= 0 (and not NaN; 0 = no Huber weight)"),
    (dict(photo_huber_grey=NAN), "photo_huber_grey must be >= 0 (and not NaN; 0 = no Huber weight)"),
    (dict(list_gray=None), "photo_scale_m > 0 needs the grey levels of the list and of the frame"),
    (dict(frame_gray=None), "photo_scale_m > 0 needs the grey levels of the list and of the frame"),
    (dict(photo_res=at(PHOTO_RES, 2)), "the photo residuals and the photo counts must be 4-byte aligned"),
    (dict(photo_counts=at(PHOTO_COUNTS, 2)), "the photo residuals and the photo counts must be 4-byte aligned"),
]


def refused(call, fault, message):
    for o in OUTPUTS:
        o[:] = 7
    assert call(**fault) == INVALID
    assert last_error() == message
    assert all((o == 7).all() for o in OUTPUTS)  # nothing written


@pytest.mark.parametrize("who, call", [("icp_points_joint", device_call), ("icp_points_joint_host", host_call)])
@pytest.mark.parametrize("k", range(len(JOINT)))
def test_shared_refusals(who, call, k):
    fault, sentence = JOINT[k]
    refused(call, fault, f"{who}: {sentence}")


@pytest.mark.parametrize("k", range(len(DEVICE_ONLY)))
def test_device_entry_refusals(k):
    fault, sentence = DEVICE_ONLY[k]
    refused(device_call, fault, f"icp_points_joint: {sentence}")


def test_the_bounds_themselves_and_the_nullable_arguments_are_accepted_on_the_host():
    for ok in (dict(photo_huber_grey=0.0), dict(photo_scale_m=0.0), dict(photo_scale_m=0.0, list_gray=None, frame_gray=None),
               dict(photo_res=None), dict(photo_counts=None),
               dict(stats=None, sums=None, res=None, ranges=None, gates=None, frame_normals=None, photo_res=None, photo_counts=None)):
        assert host_call(**ok) == 0, ok


def test_icp_map_joint_refuses_a_null_handle():
    assert V.lib().vors_trackers_icp_map_joint(None, at(DEPTH), at(FRAME_GRAY), 0.1, 0.0, 1e-5, 4, 6, None, 0, None, 0, at(FRAME_NORMALS), 0.5, 0.01,
                                               0.0005, 10.0, at(WS), at(OUT), None, None, None, at(GATES), None, at(PHOTO_COUNTS), None) == INVALID
    assert last_error() == "icp_map: the handle t is NULL"


def test_python_layer():
    assert V.ICP_PHOTO_COUNTS == 2
    with pytest.raises(V.VorsError):  # a grey frame of another shape
        V.icp_points_joint_host(np.zeros((4, 3)), np.zeros((4, 3)), np.zeros(4, np.uint8), np.zeros((3, 3), np.uint16), np.zeros((3, 4), np.uint8),
                                CAM5, 5000.0, np.zeros(7), 0.1, photo_scale_m=0.001)
    with pytest.raises(V.VorsError):  # a list of grey levels of another length
        V.icp_points_joint_host(np.zeros((4, 3)), np.zeros((4, 3)), np.zeros(5, np.uint8), np.zeros((3, 3), np.uint16), np.zeros((3, 3), np.uint8),
                                CAM5, 5000.0, np.zeros(7), 0.1, photo_scale_m=0.001)
