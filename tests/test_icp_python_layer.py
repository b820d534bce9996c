"""The Python layer over the nine ICP entries (vors_amd/__init__.py): what a caller sees of it without a device.

  1. the signatures and docstrings of the nine public functions and methods, of the map ICP parameter builders, verdict helpers and
     decoders, and of the six Trackers getters
  2. argtypes and restype of the nine C entries, written out here as include/vors_hip.h declares them
  3. the refusals of the three device wrappers on CPU tensors (judged before the library computes anything), whole messages
  4. the refusals of the three host wrappers, whole messages, and one accepted call per form: keys and dtypes
  5. map_icp_params / map_icp_joint_params / _map_icp_arg: refusals and every field of the record
"""
import ctypes as C
import inspect
import zlib

import numpy as np
import pytest
import torch

import vors_amd as V

# ------------------------------------------------------------------------------------------------------------------ 1.
SIGNATURES = {
    "icp_points": "(xyz, normals, list_counts, depth, cam5, depth_scale, poses, dist_m, damping=0.0, step_eps=1e-05, iters=8, min_points=6, "
                  "ranges=None, workspace=None, stats=True, sums29=False, residuals=False)",
    "icp_points_robust": "(xyz, normals, list_counts, depth, cam5, depth_scale, poses, dist_m, damping=0.0, step_eps=1e-05, iters=8, "
                         "min_points=6, frame_normals=None, min_cos=0.0, huber_m=0.0, ranges=None, workspace=None, stats=True, sums29=False, "
                         "residuals=False, gate_counts=False)",
    "icp_points_joint": "(xyz, normals, list_gray, list_counts, depth, frame_gray, cam5, depth_scale, poses, dist_m, damping=0.0, "
                        "step_eps=1e-05, iters=8, min_points=6, frame_normals=None, min_cos=0.0, huber_m=0.0, photo_scale_m=0.0, "
                        "photo_huber_grey=0.0, ranges=None, workspace=None, stats=True, sums29=False, residuals=False, gate_counts=False, "
                        "photo_residuals=False, photo_counts=False)",
    "icp_points_host": "(xyz, normals, depth, cam5, depth_scale, pose7, dist_m, damping=0.0, step_eps=1e-05, iters=8, min_points=6, count=None, "
                       "range2=None, residuals=None)",
    "icp_points_robust_host": "(xyz, normals, depth, cam5, depth_scale, pose7, dist_m, damping=0.0, step_eps=1e-05, iters=8, min_points=6, "
                              "frame_normals=None, min_cos=0.0, huber_m=0.0, count=None, range2=None, residuals=None)",
    "icp_points_joint_host": "(xyz, normals, list_gray, depth, frame_gray, cam5, depth_scale, pose7, dist_m, damping=0.0, step_eps=1e-05, "
                             "iters=8, min_points=6, frame_normals=None, min_cos=0.0, huber_m=0.0, photo_scale_m=0.0, photo_huber_grey=0.0, "
                             "count=None, range2=None, residuals=None, photo_residuals=None)",
    "Trackers.icp_map": "(self, depth, dist_m, damping=0.0, step_eps=1e-05, iters=8, min_points=6, poses=None, ranges=None, workspace=None, "
                        "stats=True, sums29=False, residuals=False)",
    "Trackers.icp_map_robust": "(self, depth, dist_m, damping=0.0, step_eps=1e-05, iters=8, min_points=6, frame_normals=None, min_cos=0.0, "
                               "huber_m=0.0, poses=None, ranges=None, workspace=None, stats=True, sums29=False, residuals=False, "
                               "gate_counts=False)",
    "Trackers.icp_map_joint": "(self, depth, dist_m, frame_gray=None, damping=0.0, step_eps=1e-05, iters=8, min_points=6, frame_normals=None, "
                              "min_cos=0.0, huber_m=0.0, photo_scale_m=0.0, photo_huber_grey=0.0, poses=None, ranges=None, workspace=None, "
                              "stats=True, sums29=False, residuals=False, gate_counts=False, photo_residuals=False, photo_counts=False)",
    "map_icp_params": "(dist_m=_REQUIRED, **params)",
    "map_icp_joint_params": "(dist_m=_REQUIRED, **params)",
    "map_icp_verdict_host": "(params, stats, pose_before, pose_after)",
    "map_icp_verdict_joint_host": "(params, stats, pose_before, pose_after, dilution_t, dilution_r)",
    "decode_map_icp_records": "(records)",
    "decode_map_icp_joint_records": "(records)",
    "_map_icp_arg": "(spec)",
    "Trackers.keyframe_depth": "(self, copy=True)",
    "Trackers.map": "(self, copy=True)",
    "Trackers.map_normals": "(self, copy=True)",
    "Trackers.map_voxels": "(self, copy=True)",
    "Trackers.map_icp": "(self, copy=True)",
    "Trackers.map_icp_joint": "(self, copy=True)",
}

# zlib.crc32 of inspect.getdoc() of each: the docstrings are part of what stays
DOC_CRC32 = {
    "icp_points": 1933623362, "icp_points_robust": 2502540823, "icp_points_joint": 1489779827, "icp_points_host": 2293538739,
    "icp_points_robust_host": 3703965104, "icp_points_joint_host": 2054864505, "Trackers.icp_map": 3663530926,
    "Trackers.icp_map_robust": 3569641151, "Trackers.icp_map_joint": 194508560, "map_icp_params": 806365749, "map_icp_joint_params": 1388798211,
    "map_icp_verdict_host": 2304700328, "map_icp_verdict_joint_host": 4181385864, "decode_map_icp_records": 2571515442,
    "decode_map_icp_joint_records": 27553497, "_map_icp_arg": 2919401672, "Trackers.keyframe_depth": 2434520171, "Trackers.map": 2757720100,
    "Trackers.map_normals": 394323334, "Trackers.map_voxels": 936475977, "Trackers.map_icp": 1492237991, "Trackers.map_icp_joint": 73726070,
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signature(name):
    obj = V
    for part in name.split("."):
        obj = getattr(obj, part)
    assert str(inspect.signature(obj)).replace(repr(V._REQUIRED), "_REQUIRED") == SIGNATURES[name]
    assert zlib.crc32(inspect.getdoc(obj).encode()) == DOC_CRC32[name]


# ------------------------------------------------------------------------------------------------------------------ 2.
vp, i, f, sz, u32 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_uint32
ARGTYPES = {
    "vors_icp_points": [i, vp, vp, vp, i, vp, sz, vp, sz, vp, vp, i, i, f, f, f, f, i, i, vp, vp, vp, vp, vp, vp],
    "vors_icp_points_host": [vp, vp, u32, i, vp, vp, vp, vp, i, i, f, f, f, f, i, i, vp, vp, vp, vp],
    "vors_trackers_icp_map": [vp, vp, f, f, f, i, i, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp],
    "vors_icp_points_robust": [i, vp, vp, vp, i, vp, sz, vp, sz, vp, vp, i, i, f, f, f, f, i, i, vp, f, f, vp, vp, vp, vp, vp, vp, vp],
    "vors_icp_points_robust_host": [vp, vp, u32, i, vp, vp, vp, vp, i, i, f, f, f, f, i, i, vp, f, f, vp, vp, vp, vp, vp],
    "vors_trackers_icp_map_robust": [vp, vp, f, f, f, i, i, vp, sz, vp, sz, vp, f, f, vp, vp, vp, vp, vp, vp, vp],
    "vors_icp_points_joint": [i, vp, vp, vp, vp, i, vp, sz, vp, sz, vp, vp, vp, i, i, f, f, f, f, i, i, vp, f, f, f, f, vp, vp, vp, vp, vp, vp,
                              vp, vp, vp],
    "vors_icp_points_joint_host": [vp, vp, vp, u32, i, vp, vp, vp, vp, vp, i, i, f, f, f, f, i, i, vp, f, f, f, f, vp, vp, vp, vp, vp, vp, vp],
    "vors_trackers_icp_map_joint": [vp, vp, vp, f, f, f, i, i, vp, sz, vp, sz, vp, f, f, f, f, vp, vp, vp, vp, vp, vp, vp, vp, vp],
}


@pytest.mark.parametrize("name", sorted(ARGTYPES))
def test_argtypes_and_restype(name):
    fn = getattr(V.lib(), name)
    assert list(fn.argtypes) == ARGTYPES[name]
    assert fn.restype is C.c_int


# ------------------------------------------------------------------------------------------------------------------ 3.
N, CAP, ROWS, COLS = 2, 4, 3, 4
CAM = (1.5, 1.0, 2.0, 2.0, 0.0)
DEVICE_FORMS = ("icp_points", "icp_points_robust", "icp_points_joint")
LISTS = "{who}: xyz and normals float32 [n, capacity, 3], list_counts int32 [n], contiguous"
DEPTH = "{who}: depth int16 [n, rows, cols], contiguous"


def device_args():
    return dict(xyz=torch.zeros((N, CAP, 3)), normals=torch.zeros((N, CAP, 3)), list_counts=torch.zeros(N, dtype=torch.int32),
                depth=torch.zeros((N, ROWS, COLS), dtype=torch.int16), cam5=CAM, depth_scale=5000.0, poses=torch.zeros((N, 7)), dist_m=0.1)


def device_call(who, **over):
    a = device_args()
    if who == "icp_points_joint":
        a.update(list_gray=torch.zeros((N, CAP), dtype=torch.uint8), frame_gray=torch.zeros((N, ROWS, COLS), dtype=torch.uint8))
    a.update(over)
    return getattr(V, who)(**a)


DEVICE_FAULTS = [
    ("xyz dtype", DEVICE_FORMS, dict(xyz=torch.zeros((N, CAP, 3), dtype=torch.float64)), LISTS),
    ("normals shape", DEVICE_FORMS, dict(normals=torch.zeros((N, CAP + 1, 3))), LISTS),
    ("list_counts dtype", DEVICE_FORMS, dict(list_counts=torch.zeros(N, dtype=torch.int64)), LISTS),
    ("depth dtype", DEVICE_FORMS, dict(depth=torch.zeros((N, ROWS, COLS), dtype=torch.int32)), DEPTH),
    ("depth leading dimension", DEVICE_FORMS, dict(depth=torch.zeros((N + 1, ROWS, COLS), dtype=torch.int16)), DEPTH),
    ("no poses", DEVICE_FORMS, dict(poses=None), "{who}: poses are required"),
    ("small workspace", DEVICE_FORMS, dict(workspace=torch.zeros(327, dtype=torch.uint8)),
     "icp: expected a contiguous uint8 workspace of at least 328 bytes"),
    ("frame_normals shape", DEVICE_FORMS[1:], dict(frame_normals=torch.zeros((N, ROWS, COLS + 1, 3))),
     "{who}: frame_normals float32 (2, 3, 4, 3), contiguous (depth_normals() of the same depth without poses)"),
    ("list_gray shape", DEVICE_FORMS[2:], dict(list_gray=torch.zeros((N, CAP + 1), dtype=torch.uint8)), "{who}: list_gray uint8 (2, 4), contiguous"),
    ("frame_gray shape", DEVICE_FORMS[2:], dict(frame_gray=torch.zeros((N, ROWS + 1, COLS), dtype=torch.uint8)),
     "{who}: frame_gray uint8 (2, 3, 4), contiguous"),
]


@pytest.mark.parametrize("fault,who", [(k, who) for k, (_, forms, _, _) in enumerate(DEVICE_FAULTS) for who in forms],
                         ids=lambda v: DEVICE_FAULTS[v][0] if isinstance(v, int) else v)
def test_device_wrapper_refusal(fault, who):
    _, _, over, sentence = DEVICE_FAULTS[fault]
    with pytest.raises(V.VorsError) as e:
        device_call(who, **over)
    assert str(e.value) == sentence.format(who=who)


# ------------------------------------------------------------------------------------------------------------------ 4.
HOST_FORMS = ("icp_points_host", "icp_points_robust_host", "icp_points_joint_host")
HOST_SHAPES = {
    "icp_points_host": "icp_points_host: xyz and normals [capacity, 3], depth [rows, cols], cam5 [5], pose7 [7], range2 [2] or None",
    "icp_points_robust_host": "icp_points_robust_host: xyz and normals [capacity, 3], depth [rows, cols], cam5 [5], pose7 [7], range2 [2] or None, "
                              "frame_normals [rows, cols, 3] or None",
    "icp_points_joint_host": "icp_points_joint_host: xyz and normals [capacity, 3], list_gray [capacity] or None, depth [rows, cols], frame_gray "
                             "[rows, cols] or None, cam5 [5], pose7 [7], range2 [2] or None, frame_normals [rows, cols, 3] or None",
}
POSE = (0, 0, 0, 0, 0, 0, 1)


def host_call(who, **over):
    xyz = np.array([[0, 0, 1], [0.2, 0, 1], [0, 0.2, 1], [0.2, 0.2, 1]], np.float32)
    a = dict(xyz=xyz, normals=np.tile(np.float32([0, 0, -1]), (4, 1)), depth=np.full((ROWS, COLS), 5000, np.uint16), cam5=CAM, depth_scale=5000.0,
             pose7=POSE, dist_m=0.1, iters=2)
    if who == "icp_points_joint_host":
        a.update(list_gray=np.zeros(4, np.uint8), frame_gray=np.zeros((ROWS, COLS), np.uint8))
    a.update(over)
    return getattr(V, who)(**a)


HOST_FAULTS = [
    ("lengths", HOST_FORMS, dict(normals=np.zeros((3, 3), np.float32)), None),
    ("cam5 of four", HOST_FORMS, dict(cam5=CAM[:4]), None),
    ("pose7 of six", HOST_FORMS, dict(pose7=POSE[:6]), None),
    ("range2 of three", HOST_FORMS, dict(range2=(0, 1, 2)), None),
    ("frame_normals shape", HOST_FORMS[1:], dict(frame_normals=np.zeros((ROWS, COLS, 2), np.float32)), None),
    ("list_gray shape", HOST_FORMS[2:], dict(list_gray=np.zeros(5, np.uint8)), None),
    ("frame_gray shape", HOST_FORMS[2:], dict(frame_gray=np.zeros((ROWS, COLS + 1), np.uint8)), None),
    ("residuals dtype", HOST_FORMS, dict(residuals=np.zeros(4, np.float64)), "{who}: residuals must be a contiguous float32 array (4,)"),
    ("photo_residuals dtype", HOST_FORMS[2:], dict(photo_residuals=np.zeros(4, np.float64)),
     "{who}: photo_residuals must be a contiguous float32 array (4,)"),
]


@pytest.mark.parametrize("fault,who", [(k, who) for k, (_, forms, _, _) in enumerate(HOST_FAULTS) for who in forms],
                         ids=lambda v: HOST_FAULTS[v][0] if isinstance(v, int) else v)
def test_host_wrapper_refusal(fault, who):
    _, _, over, sentence = HOST_FAULTS[fault]
    with pytest.raises(V.VorsError) as e:
        host_call(who, **over)
    assert str(e.value) == (HOST_SHAPES[who] if sentence is None else sentence.format(who=who))


HOST_KEYS = {"pose": (np.float32, (7,)), "sums29": (np.float32, (29,)), "residuals": (np.float32, (4,))}
HOST_ROBUST_KEYS = dict(HOST_KEYS, gate_counts=(np.uint32, (4,)))
HOST_JOINT_KEYS = dict(HOST_ROBUST_KEYS, photo_residuals=(np.float32, (4,)), photo_counts=(np.uint32, (2,)))


@pytest.mark.parametrize("who,keys", zip(HOST_FORMS, (HOST_KEYS, HOST_ROBUST_KEYS, HOST_JOINT_KEYS)))
def test_host_wrapper_accepts(who, keys):
    out = host_call(who)
    assert set(out) == set(keys) | {"stats"}
    for k, (dtype, shape) in keys.items():
        assert out[k].dtype == dtype and out[k].shape == shape, k
    assert out["stats"].dtype == V.ICP_STATS_DTYPE and out["stats"].shape == ()
    assert int(out["stats"]["considered"]) == 4 and np.isfinite(out["pose"]).all()


# ------------------------------------------------------------------------------------------------------------------ 5.
NAMES = "dist_m, damping, step_eps, iters, min_points, normal_gate, min_cos, huber_m, last_keyframes, min_match_ratio, max_rms, max_trans_m, max_rot_rad"


def fields(p):
    return {name: getattr(p, name) for name, _ in p._fields_}


def as_stored(values):
    """What a record holds of these values: the floats rounded to float32, the ints as they are."""
    return {k: v if isinstance(v, int) else float(np.float32(v)) for k, v in values.items()}


@pytest.mark.parametrize("build,own", [(V.map_icp_params, "map_icp"), (V.map_icp_joint_params, "map_icp_joint")])
def test_map_icp_params_refusals(build, own):
    for kwargs, sentence in [
        (dict(), "map_icp: dist_m is required"),
        (dict(dist_m=0.1, foo=1), f"map_icp: unknown parameter 'foo' ({NAMES})"),
        (dict(dist_m=0.1, damping="x"), "map_icp: damping must be a number, got 'x'"),
        (dict(dist_m=None), "map_icp: dist_m must be a number, got None"),
        (dict(dist_m=0.1, iters=2.5), "map_icp: iters must be an integer that fits a C int, got 2.5"),
        (dict(dist_m=0.1, iters=True), "map_icp: iters must be a number, got True"),
        (dict(dist_m=0.1, last_keyframes=2 ** 31), f"map_icp: last_keyframes must be an integer that fits a C int, got {2 ** 31}"),
    ] + ([] if own == "map_icp" else [
        (dict(dist_m=0.1, photo_scale_m="x"), "map_icp_joint: photo_scale_m must be a number, got 'x'"),
        (dict(dist_m=0.1, max_dilution_t=True), "map_icp_joint: max_dilution_t must be a number, got True"),
    ]):
        with pytest.raises(V.VorsError) as e:
            build(**kwargs)
        assert str(e.value) == sentence, kwargs


def test_map_icp_params_fields():
    assert fields(V.map_icp_params(dist_m=0.05)) == as_stored(dict(V.MAP_ICP_DEFAULTS, dist_m=0.05))
    over = dict(dist_m=0.2, damping=1e-3, step_eps=1e-6, iters=np.int64(3), min_points=40, normal_gate=False, min_cos=0.5, huber_m=0.01,
                last_keyframes=2, min_match_ratio=0.25, max_rms=0.02, max_trans_m=0.1, max_rot_rad=np.float32(0.2))
    assert fields(V.map_icp_params(**over)) == as_stored(dict(over, iters=3, normal_gate=0, max_rot_rad=float(np.float32(0.2))))
    assert V.map_icp_params(dist_m=1, normal_gate=np.bool_(True)).normal_gate == 1


def test_map_icp_joint_params_fields():
    p = V.map_icp_joint_params(dist_m=0.05)
    assert fields(p.icp) == as_stored(dict(V.MAP_ICP_DEFAULTS, dist_m=0.05))
    assert {k: getattr(p, k) for k in V.MAP_ICP_JOINT_DEFAULTS} == as_stored(V.MAP_ICP_JOINT_DEFAULTS)
    own = dict(photo_scale_m=0.004, photo_huber_grey=12, max_dilution_t=3.5, max_dilution_r=np.float32(1.5))
    p = V.map_icp_joint_params(0.2, iters=3, min_cos=0.5, **own)
    assert fields(p.icp) == as_stored(dict(V.MAP_ICP_DEFAULTS, dist_m=0.2, iters=3, min_cos=0.5))
    assert {k: getattr(p, k) for k in own} == as_stored(dict(own, photo_huber_grey=12.0, max_dilution_r=1.5))


def test_map_icp_arg():
    assert V._map_icp_arg(None) is None
    assert fields(V._map_icp_arg(0.05)) == as_stored(dict(V.MAP_ICP_DEFAULTS, dist_m=0.05))
    assert fields(V._map_icp_arg(dict(dist_m=0.05, iters=2))) == as_stored(dict(V.MAP_ICP_DEFAULTS, dist_m=0.05, iters=2))
    with pytest.raises(V.VorsError) as e:
        V._map_icp_arg(dict(iters=2))
    assert str(e.value) == "map_icp: dist_m is required"
