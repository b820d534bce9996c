"""The exact text of the refusals that need no device. One fault per case, whole messages compared with ==.

  1. the six batch products on a NULL handle;
  2. vors_render_points, vors_depth_normals, vors_points_normals, vors_render_points_host and vors_depth_normals_host: every refusal that
     comes before the device is asked for (each NULL, each range, each stride fault, each misalignment);
  3. the four switch parsers of the Python layer (depth_filter, map, map_voxels, map_normals).

The expected strings are the library's own sentences, written out here so that a changed sentence is noticed. Needs no GPU: a refused
call touches none of its pointers, and the buffers below are real all the same."""
import numpy as np
import pytest

import vors_amd as V

INVALID = -1
ROWS, COLS, CAP, N = 6, 8, 16, 2
TOO_LARGE = 0x80000000   # the first stride above the limit of the handle-free operators

# (64-bit items: every base address is 8-byte aligned, so `+ 1` and `+ 2` below are misaligned for certain)
XYZ = np.zeros(N * CAP * 3 * 2, np.float64)
LIST_GRAY = np.zeros(N * CAP, np.uint64)
LIST_COUNTS = np.zeros(N, np.uint64)
PIXEL = np.zeros(N * CAP, np.uint64)
RANGES = np.zeros(N * 2, np.uint64)
POSES = np.zeros(N * 7, np.float64)
CAM5 = np.array([3.5, 2.5, 9.0, -9.5, 0.0], np.float32)
ZKEY = np.zeros(N * ROWS * COLS, np.uint64)
DEPTH = np.zeros(N * ROWS * COLS, np.uint64)
GRAY_OUT = np.zeros(N * ROWS * COLS, np.uint64)
COUNTS = np.zeros(N * 4, np.uint64)
NORMALS = np.zeros(N * ROWS * COLS * 3, np.float64)


def at(a, offset=0):
    return a.ctypes.data + offset


def last_error():
    return V.lib().vors_last_error().decode()


# ------------------------------------------------------------------------------------------------------------ 1
def null_handle_calls():
    lib, p = V.lib(), at(XYZ)
    return {
        "eval_pairs": lambda: lib.vors_batch_eval_pairs(None, 1, 0, 1, p, 0, V.ARITH_EXACT, 0, p, None),
        "pose_information": lambda: lib.vors_batch_pose_information(None, 1, 0, p, 0, p, p, p, p, None),
        "residual_maps": lambda: lib.vors_batch_residual_maps(None, 1, 0, p, 0, p, None, None, None, None),
        "reproject_depth": lambda: lib.vors_batch_reproject_depth(None, 1, 0, p, 0, None, 0.0, p, None, None, None, None),
        "fuse_depth": lambda: lib.vors_batch_fuse_depth(None, 1, p, 0, p, 0.0, None, 255, 0, p, None, None, None, None),
        "point_cloud": lambda: lib.vors_batch_point_cloud(None, 1, 0, None, 0, None, 4, p, None, None, None, None),
    }


@pytest.mark.parametrize("product", ["eval_pairs", "pose_information", "residual_maps", "reproject_depth", "fuse_depth", "point_cloud"])
def test_batch_products_refuse_a_null_handle(product):
    assert null_handle_calls()[product]() == INVALID
    assert last_error() == f"{product}: the handle b is NULL"


# ------------------------------------------------------------------------------------------------------------ 2
def render_points(**o):
    a = dict(n=N, xyz=at(XYZ), list_gray=at(LIST_GRAY), list_counts=at(LIST_COUNTS), capacity=CAP, ranges=at(RANGES), range_stride=0, cam5=at(CAM5),
             rows=ROWS, cols=COLS, scale=5000.0, poses=at(POSES), pose_stride=0, footprint=1, zkey=at(ZKEY), depth=at(DEPTH), gray=at(GRAY_OUT),
             counts=at(COUNTS))
    a.update(o)
    return V.lib().vors_render_points(a["n"], a["xyz"], a["list_gray"], a["list_counts"], a["capacity"], a["ranges"], a["range_stride"], a["cam5"],
                                      a["rows"], a["cols"], a["scale"], a["poses"], a["pose_stride"], a["footprint"], a["zkey"], a["depth"], a["gray"],
                                      a["counts"], None)


def render_points_host(**o):
    a = dict(xyz=at(XYZ), list_gray=at(LIST_GRAY), count=CAP, capacity=CAP, range2=None, cam5=at(CAM5), rows=ROWS, cols=COLS, scale=5000.0, pose=None,
             footprint=1, zkey=at(ZKEY), depth=at(DEPTH), gray=at(GRAY_OUT), counts=at(COUNTS))
    a.update(o)
    return V.lib().vors_render_points_host(a["xyz"], a["list_gray"], a["count"], a["capacity"], a["range2"], a["cam5"], a["rows"], a["cols"], a["scale"],
                                           a["pose"], a["footprint"], a["zkey"], a["depth"], a["gray"], a["counts"])


# what vors_render_points and vors_render_points_host refuse alike, in the words of both (the key names the host entry's arguments)
RENDER_SHARED = [
    (dict(xyz=None), "a list (xyz, list_gray) is NULL"),
    (dict(list_gray=None), "a list (xyz, list_gray) is NULL"),
    (dict(cam5=None), "cam5 is NULL"),
    (dict(zkey=None), "zkey is NULL (the pass keeps no plane of its own)"),
    (dict(zkey=at(ZKEY, 4)), "zkey must be 8-byte aligned"),
    (dict(footprint=0), "footprint must be 1, 2 or 3"),
    (dict(footprint=4), "footprint must be 1, 2 or 3"),
    (dict(rows=0), "rows and cols must be >= 1"),
    (dict(cols=0), "rows and cols must be >= 1"),
    (dict(capacity=0), "capacity must be >= 1"),
    (dict(rows=65536), "rows / cols must not exceed 65535 and rows * cols must not exceed 2^28 pixels"),
    (dict(cols=65536), "rows / cols must not exceed 65535 and rows * cols must not exceed 2^28 pixels"),
    (dict(rows=20000, cols=20000), "rows / cols must not exceed 65535 and rows * cols must not exceed 2^28 pixels"),
    (dict(scale=0.0), "depth_scale must be > 0"),
    (dict(scale=float("nan")), "depth_scale must be > 0"),
]
RENDER_DEVICE_ONLY = [
    (dict(n=0), "n must be >= 1"),
    (dict(list_counts=None), "a list (d_list_counts) is NULL"),
    (dict(pose_stride=24), "pose_stride_bytes must be 0 or a multiple of 4 of at least 28"),
    (dict(pose_stride=30), "pose_stride_bytes must be 0 or a multiple of 4 of at least 28"),
    (dict(pose_stride=TOO_LARGE), "pose_stride_bytes must be 0 or a multiple of 4 of at least 28"),
    (dict(range_stride=4), "range_stride_bytes must be 0 or a multiple of 4 of at least 8"),
    (dict(range_stride=10), "range_stride_bytes must be 0 or a multiple of 4 of at least 8"),
    (dict(range_stride=TOO_LARGE), "range_stride_bytes must be 0 or a multiple of 4 of at least 8"),
    (dict(ranges=at(RANGES, 2)), "d_ranges must be 4-byte aligned"),
    (dict(xyz=at(XYZ, 2)), "d_xyz, d_list_counts and d_poses7 must be 4-byte aligned"),
    (dict(list_counts=at(LIST_COUNTS, 2)), "d_xyz, d_list_counts and d_poses7 must be 4-byte aligned"),
    (dict(poses=at(POSES, 2)), "d_xyz, d_list_counts and d_poses7 must be 4-byte aligned"),
    (dict(depth=at(DEPTH, 1)), "d_depth must be 2-byte aligned"),
    (dict(counts=at(COUNTS, 2)), "d_counts must be 4-byte aligned"),
]


@pytest.mark.parametrize("bad, text", RENDER_SHARED + RENDER_DEVICE_ONLY, ids=lambda v: None if isinstance(v, dict) else v[:40])
def test_render_points_refusals_before_the_device(bad, text):
    assert render_points(**bad) == INVALID, bad
    assert last_error() == "render_points: " + text


@pytest.mark.parametrize("bad, text", RENDER_SHARED, ids=lambda v: None if isinstance(v, dict) else v[:40])
def test_render_points_host_refusals(bad, text):
    before = ZKEY.copy()
    assert render_points_host(**bad) == INVALID, bad
    assert last_error() == "render_points_host: " + text
    assert (ZKEY == before).all()


def depth_normals(**o):
    a = dict(n=N, depth=at(DEPTH), cam5=at(CAM5), rows=ROWS, cols=COLS, scale=5000.0, step=1, jump_m=0.5, poses=at(POSES), pose_stride=0,
             normals=at(NORMALS), counts=at(COUNTS))
    a.update(o)
    return V.lib().vors_depth_normals(a["n"], a["depth"], a["cam5"], a["rows"], a["cols"], a["scale"], a["step"], a["jump_m"], a["poses"],
                                      a["pose_stride"], a["normals"], a["counts"], None)


def points_normals(**o):
    a = dict(n=N, depth=at(DEPTH), pixel=at(PIXEL), list_counts=at(LIST_COUNTS), capacity=CAP, ranges=at(RANGES), range_stride=0, cam5=at(CAM5),
             rows=ROWS, cols=COLS, scale=5000.0, step=1, jump_m=0.5, poses=at(POSES), pose_stride=0, normals=at(NORMALS), counts=at(COUNTS))
    a.update(o)
    return V.lib().vors_points_normals(a["n"], a["depth"], a["pixel"], a["list_counts"], a["capacity"], a["ranges"], a["range_stride"], a["cam5"],
                                       a["rows"], a["cols"], a["scale"], a["step"], a["jump_m"], a["poses"], a["pose_stride"], a["normals"],
                                       a["counts"], None)


def depth_normals_host(**o):
    a = dict(depth=at(DEPTH), cam5=at(CAM5), rows=ROWS, cols=COLS, scale=5000.0, step=1, jump_m=0.5, pose=None, pixel=None, count=0, capacity=0,
             range2=None, normals=at(NORMALS), counts=at(COUNTS))
    a.update(o)
    return V.lib().vors_depth_normals_host(a["depth"], a["cam5"], a["rows"], a["cols"], a["scale"], a["step"], a["jump_m"], a["pose"], a["pixel"],
                                           a["count"], a["capacity"], a["range2"], a["normals"], a["counts"])


# what all three normals entries refuse alike
NORMAL_SHARED = [
    (dict(depth=None), "depth is NULL"),
    (dict(cam5=None), "cam5 is NULL"),
    (dict(normals=None, counts=None), "normals and counts are both NULL (at least one output is required)"),
    (dict(step=0), "step must be in 1..8"),
    (dict(step=9), "step must be in 1..8"),
    (dict(jump_m=-1.0), "jump_m must be >= 0 (and not NaN)"),
    (dict(jump_m=float("nan")), "jump_m must be >= 0 (and not NaN)"),
    (dict(scale=0.0), "depth_scale must be > 0"),
    (dict(scale=float("nan")), "depth_scale must be > 0"),
    (dict(rows=0), "rows and cols must be >= 1"),
    (dict(cols=0), "rows and cols must be >= 1"),
    (dict(rows=65536), "rows / cols must not exceed 65535 and rows * cols must not exceed 2^28 pixels"),
    (dict(cols=65536), "rows / cols must not exceed 65535 and rows * cols must not exceed 2^28 pixels"),
    (dict(rows=20000, cols=20000), "rows / cols must not exceed 65535 and rows * cols must not exceed 2^28 pixels"),
    (dict(depth=at(DEPTH, 1)), "depth must be 2-byte aligned"),
    (dict(normals=at(NORMALS, 2)), "pixel, normals and counts must be 4-byte aligned"),
    (dict(counts=at(COUNTS, 2)), "pixel, normals and counts must be 4-byte aligned"),
]
# ... and what the list forms add
NORMAL_LIST = [
    (dict(capacity=0), "capacity must be >= 1"),
    (dict(pixel=at(PIXEL, 2)), "pixel, normals and counts must be 4-byte aligned"),
]
POSE_STRIDES = [
    (dict(pose_stride=24), "pose_stride_bytes must be 0 or a multiple of 4 of at least 28"),
    (dict(pose_stride=30), "pose_stride_bytes must be 0 or a multiple of 4 of at least 28"),
    (dict(pose_stride=TOO_LARGE), "pose_stride_bytes must be 0 or a multiple of 4 of at least 28"),
    (dict(poses=at(POSES, 2)), "d_ranges and d_poses7 must be 4-byte aligned"),
]
RANGE_STRIDES = [
    (dict(range_stride=4), "range_stride_bytes must be 0 or a multiple of 4 of at least 8"),
    (dict(range_stride=10), "range_stride_bytes must be 0 or a multiple of 4 of at least 8"),
    (dict(range_stride=TOO_LARGE), "range_stride_bytes must be 0 or a multiple of 4 of at least 8"),
    (dict(ranges=at(RANGES, 2)), "d_ranges and d_poses7 must be 4-byte aligned"),
]


@pytest.mark.parametrize("bad, text", [(dict(n=0), "n must be >= 1")] + NORMAL_SHARED + POSE_STRIDES,
                         ids=lambda v: None if isinstance(v, dict) else v[:40])
def test_depth_normals_refusals_before_the_device(bad, text):
    assert depth_normals(**bad) == INVALID, bad
    assert last_error() == "depth_normals: " + text


@pytest.mark.parametrize("bad, text", [(dict(n=0), "n must be >= 1"), (dict(list_counts=None), "a list (d_list_counts) is NULL"),
                                       (dict(list_counts=at(LIST_COUNTS, 2)), "d_list_counts must be 4-byte aligned"),
                                       (dict(pixel=None), "a list (pixel) is NULL")] + NORMAL_SHARED + NORMAL_LIST + POSE_STRIDES + RANGE_STRIDES,
                         ids=lambda v: None if isinstance(v, dict) else v[:40])
def test_points_normals_refusals_before_the_device(bad, text):
    assert points_normals(**bad) == INVALID, bad
    assert last_error() == "points_normals: " + text


@pytest.mark.parametrize("form, bad, text", [("plane", b, t) for b, t in NORMAL_SHARED] + [("list", b, t) for b, t in NORMAL_SHARED + NORMAL_LIST],
                         ids=lambda v: None if isinstance(v, dict) else v[:40])
def test_depth_normals_host_refusals(form, bad, text):
    listed = dict(pixel=at(PIXEL), count=CAP, capacity=CAP) if form == "list" else {}
    before = NORMALS.copy()
    assert depth_normals_host(**{**listed, **bad}) == INVALID, bad
    assert last_error() == "depth_normals_host: " + text
    assert (NORMALS == before).all()


# ------------------------------------------------------------------------------------------------------------ 3
class Opaque:
    def __repr__(self):
        return "<opaque>"


DEPTH_FILTER_SIG = "(tol_m[, max_weight[, fill_min_weight]])"
MAP_SIG = "(level, capacity, max_keyframes[, min_weight])"
PARSER_REFUSALS = [
    (V._depth_filter_args, Opaque(), f"depth_filter: expected None or {DEPTH_FILTER_SIG}, got <opaque>"),
    (V._depth_filter_args, True, f"depth_filter: expected None or {DEPTH_FILTER_SIG}, got True"),
    (V._depth_filter_args, (), f"depth_filter: expected 1 to 3 values {DEPTH_FILTER_SIG}, got 0"),
    (V._depth_filter_args, (0.1, 2, 3, 4), f"depth_filter: expected 1 to 3 values {DEPTH_FILTER_SIG}, got 4"),
    (V._depth_filter_args, (0.1, 2.5), "depth_filter: max_weight must be an integer, got 2.5"),
    (V._depth_filter_args, (0.1, True), "depth_filter: max_weight must be an integer, got True"),
    (V._depth_filter_args, (0.1, 2, "3"), "depth_filter: fill_min_weight must be an integer, got '3'"),
    (V._depth_filter_args, (0.1, 2, False), "depth_filter: fill_min_weight must be an integer, got False"),
    (V._depth_filter_args, ("x",), "depth_filter: tol_m must be a number, got 'x'"),
    (V._depth_filter_args, (None, 2), "depth_filter: tol_m must be a number, got None"),
    (V._map_args, 5, f"map: expected None or {MAP_SIG}, got 5"),
    (V._map_args, (0, 100), f"map: expected 3 or 4 values {MAP_SIG}, got 2"),
    (V._map_args, (0, 100, 4, 0, 0), f"map: expected 3 or 4 values {MAP_SIG}, got 5"),
    (V._map_args, (0.0, 100, 4), "map: level must be an integer, got 0.0"),
    (V._map_args, (0, "100", 4), "map: capacity must be an integer, got '100'"),
    (V._map_args, (0, 100, True), "map: max_keyframes must be an integer, got True"),
    (V._map_args, (0, 100, 4, 1.0), "map: min_weight must be an integer, got 1.0"),
    (V._map_args, (2 ** 31, 100, 4), f"map: level does not fit the C int it is passed as, got {2 ** 31}"),
    (V._map_args, (0, -2 ** 31 - 1, 4), f"map: capacity does not fit the C int it is passed as, got {-2 ** 31 - 1}"),
    (V._map_args, (0, 100, 2 ** 40), f"map: max_keyframes does not fit the C int it is passed as, got {2 ** 40}"),
    (V._map_args, (0, 100, 4, 2 ** 31), f"map: min_weight does not fit the C int it is passed as, got {2 ** 31}"),
    (V._map_voxels_args, 0.05, "map_voxels: expected None or (voxel_m, table_slots), got 0.05"),
    (V._map_voxels_args, (0.05,), "map_voxels: expected 2 values (voxel_m, table_slots), got 1"),
    (V._map_voxels_args, (0.05, 64, 1), "map_voxels: expected 2 values (voxel_m, table_slots), got 3"),
    (V._map_voxels_args, ("0.05", 64), "map_voxels: voxel_m must be a number, got '0.05'"),
    (V._map_voxels_args, (True, 64), "map_voxels: voxel_m must be a number, got True"),
    (V._map_voxels_args, (0.05, 64.0), "map_voxels: table_slots must be an integer, got 64.0"),
    (V._map_voxels_args, (0.05, False), "map_voxels: table_slots must be an integer, got False"),
    (V._map_voxels_args, (0.05, 2 ** 31), f"map_voxels: table_slots does not fit the C int it is passed as, got {2 ** 31}"),
    (V._map_normals_args, 2, "map_normals: expected None or (step, jump_m), got 2"),
    (V._map_normals_args, (2,), "map_normals: expected 2 values (step, jump_m), got 1"),
    (V._map_normals_args, (2, 0.1, 0), "map_normals: expected 2 values (step, jump_m), got 3"),
    (V._map_normals_args, (2.0, 0.1), "map_normals: step must be an integer, got 2.0"),
    (V._map_normals_args, (True, 0.1), "map_normals: step must be an integer, got True"),
    (V._map_normals_args, (2 ** 31, 0.1), f"map_normals: step does not fit the C int it is passed as, got {2 ** 31}"),
    (V._map_normals_args, (2, "0.1"), "map_normals: jump_m must be a number, got '0.1'"),
    (V._map_normals_args, (2, False), "map_normals: jump_m must be a number, got False"),
]


@pytest.mark.parametrize("parse, spec, text", PARSER_REFUSALS, ids=[f"{p.__name__}-{i}" for i, (p, _, _) in enumerate(PARSER_REFUSALS)])
def test_switch_parsers_refuse_in_these_words(parse, spec, text):
    with pytest.raises(V.VorsError) as e:
        parse(spec)
    assert str(e.value) == text


def test_switch_parsers_accept_and_fill_in_the_defaults():
    assert [V._depth_filter_args(s) for s in (None, 0.05, (0.05,), (0.05, 9), [0.05, 9, 2], np.float32(0.5))] == \
        [None, (0.05, 255, 0), (0.05, 255, 0), (0.05, 9, 0), (0.05, 9, 2), (0.5, 255, 0)]
    assert V._depth_filter_args(("0.25", 2 ** 40)) == (0.25, 2 ** 40, 0)   # this parser converts tol_m and leaves the range of the ints to the library
    assert [V._map_args(s) for s in (None, (0, 100, 4), [1, 100, 4, 3], (np.int64(2), 100, 4))] == [None, (0, 100, 4, 0), (1, 100, 4, 3), (2, 100, 4, 0)]
    assert [V._map_voxels_args(s) for s in (None, (0.05, 64), (1, np.int32(128)))] == [None, (0.05, 64), (1.0, 128)]
    assert [V._map_normals_args(s) for s in (None, (2, 0.1), [np.int32(1), 1])] == [None, (2, 0.1), (1, 1.0)]
    assert all(type(v) is t for v, t in zip(V._map_voxels_args((1, np.int32(128))) + V._map_normals_args((np.int32(1), 1)), (float, int, int, float)))
