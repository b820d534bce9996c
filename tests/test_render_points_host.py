"""Rendering of point lists into a camera on the host (vors_render_points_host) and the refusals of the device entry
(vors_render_points), which come before any device is asked for. No GPU.

  1. independent restatement: numpy, from camera_project's (u w, v w, w) and the rule of include/vors_hip.h section 2c, bit for bit on keys,
     depth, grey and counters — 48x64, footprints 1..3, with and without a pose, with and without a range, a count above capacity, an
     empty list; the list holds duplicates, points behind the camera, NaN and infinities, points around every border, a Z' whose depth
     saturates and one whose depth rounds to 0
  2. round trip: every pixel of a 120x160 depth map back-projected through a random pose and rendered at that pose returns to its own
     pixel, its depth within one unit (20 poses; measured with the library's own text: 0 misplaced of 19 200 per pose, 0 units)
  3. refusals
"""
import functools

import numpy as np
import pytest

import vors_amd as V

ROWS, COLS = 48, 64
SCALE = 5000.0
EMPTY = np.uint64(V.ZKEY_EMPTY)
F32 = np.float32


def cam(rows, cols):
    return np.asarray(V.scaled_intrinsics(rows, cols), np.float32)


def random_pose(rng, angle=0.15, shift=0.2):
    w = rng.uniform(-angle, angle, 3)
    th = np.linalg.norm(w)
    q = np.concatenate([np.sin(th / 2) * w / th, [np.cos(th / 2)]]).astype(np.float32)
    q /= np.sqrt((q * q).sum(dtype=np.float32))
    return np.concatenate([rng.uniform(-shift, shift, 3).astype(np.float32), q]).astype(np.float32)


POSE = random_pose(np.random.default_rng(7))


@functools.lru_cache(maxsize=None)
def hostile_list(with_pose):
    """(xyz [n, 3] f32, gray [n] u8): about 5000 world points, most of them in view of the camera at POSE (or of the identity camera)."""
    rng = np.random.default_rng(11)
    pose = POSE if with_pose else None
    k = cam(ROWS, COLS)
    parts = []

    def add(xy, depth):
        parts.append(V.camera_back_project(k, pose, np.asarray(xy, np.float32), np.asarray(depth, np.float32)))

    n = 3600
    # (the lower third of the image gets no random point: pixels stay empty under every footprint)
    add(np.stack([rng.uniform(-3, COLS + 3, n), rng.uniform(-3, 0.66 * ROWS, n)], 1), rng.uniform(0.5, 6.0, n))
    # around every border, at the fractions where each footprint's anchor changes pixel
    edge = np.array([-5.2, -4.6, -4.4, -3.6, -2.6, -2.4, -1.6, -1.4, -1.0, -0.6, -0.4, 0.0, 0.4, 0.6])
    xs = np.concatenate([edge, COLS - 1 + edge[::-1] * -1])
    ys = np.concatenate([edge, ROWS - 1 + edge[::-1] * -1])
    gx, gy = np.meshgrid(xs, ys)
    add(np.stack([gx.ravel(), gy.ravel()], 1), rng.uniform(1.0, 2.0, gx.size))
    # behind the camera; a depth that saturates to 65535; one that rounds to 0
    m = 60
    add(np.stack([rng.uniform(0, COLS, m), rng.uniform(0, ROWS, m)], 1), -rng.uniform(0.5, 3.0, m))
    add(np.stack([rng.uniform(0, COLS, m), rng.uniform(0, ROWS, m)], 1), np.full(m, 20.0))
    add(np.stack([rng.uniform(5, COLS - 5, m), rng.uniform(5, ROWS - 5, m)], 1), np.full(m, 1e-5))
    xyz = np.concatenate(parts)
    # NaN and infinities in every coordinate
    bad = xyz[:24].copy()
    for i, v in enumerate([np.nan, np.inf, -np.inf, 3e38] * 6):
        bad[i, i % 3] = v
    bad[20] = np.nan
    bad[21] = np.inf
    xyz = np.concatenate([xyz, bad])
    # duplicates: equal Z' bits on one pixel, at a higher rank and (moved to the front) at a lower one
    xyz = np.concatenate([xyz[300:420], xyz, xyz[100:300]])
    gray = rng.integers(1, 256, len(xyz)).astype(np.uint8)
    return np.ascontiguousarray(xyz, np.float32), gray


def round_half_away(x):
    """roundf for x >= 0 (f32::round): exact, x - trunc(x) is representable."""
    t = np.trunc(x)
    return t + (x - t >= F32(0.5)).astype(np.float32)


def restatement(xyz, gray, count, rng2, k, rows, cols, scale, pose, f):
    """include/vors_hip.h section 2c in numpy float32 from camera_project's output."""
    n = min(int(count), len(xyz))
    first, last = 0, n
    if rng2 is not None:
        first = min(int(rng2[0]), n)
        last = n if int(rng2[1]) > n - first else first + int(rng2[1])
    zkey = np.full(rows * cols, EMPTY, np.uint64)
    counts = np.zeros(4, np.uint32)
    counts[0] = last - first
    if last > first:
        uvw = V.camera_project(k, pose, xyz[first:last])
        z = uvw[:, 2]
        with np.errstate(all="ignore"):
            u, v = uvw[:, 0] / z, uvw[:, 1] / z
            assert u.dtype == np.float32
            x0f = np.floor(u) if f == 2 else np.floor(u + F32(0.5))
            y0f = np.floor(v) if f == 2 else np.floor(v + F32(0.5))
            front = z > 0
            cand = front & (x0f >= F32(-4)) & (x0f < F32(cols) + F32(4)) & (y0f >= F32(-4)) & (y0f < F32(rows) + F32(4))
        counts[1] = front.sum()
        idx = np.nonzero(cand)[0]
        x0, y0 = x0f[idx].astype(np.int64), y0f[idx].astype(np.int64)
        key = (z[idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (idx + first).astype(np.uint64)
        offs = {1: [0], 2: [0, 1], 3: [-1, 0, 1]}[f]
        landed = np.zeros(len(idx), bool)
        for dy in offs:
            for dx in offs:
                x, y = x0 + dx, y0 + dy
                ok = (x >= 0) & (x < cols) & (y >= 0) & (y < rows)
                np.minimum.at(zkey, (y * cols + x)[ok], key[ok])
                landed |= ok
        counts[2] = landed.sum()
    covered = zkey != EMPTY
    counts[3] = covered.sum()
    zp = (zkey >> np.uint64(32)).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        r = round_half_away(F32(scale) / (F32(1.0) / zp))
    depth = np.where(r >= F32(65535), 65535, np.where(r > 0, r, 0)).astype(np.uint16)
    depth[~covered] = 0
    g = np.zeros(rows * cols, np.uint8)
    g[covered] = gray[(zkey[covered] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    return dict(zkey=zkey.reshape(rows, cols), depth=depth.reshape(rows, cols), gray=g.reshape(rows, cols), counts=counts)


def assert_same(got, want, where):
    for name in ("zkey", "depth", "gray", "counts"):
        a, b = got[name], want[name]
        assert a.dtype == b.dtype and a.shape == b.shape, f"{where}: {name} {a.dtype} {a.shape} against {b.dtype} {b.shape}"
        assert a.tobytes() == b.tobytes(), f"{where}: {name} differs at {np.argwhere(a != b)[:5].tolist()}"


# ------------------------------------------------------------------------------------------------------------ 1
CASES = [("whole", None, None), ("range", None, (700, 2900)), ("range_past_end", None, (4000, 1 << 31)), ("range_beyond", None, (1 << 30, 5)),
         ("count_above_capacity", 1 << 20, None), ("count_short", 1234, (1000, 1000)), ("empty", 0, None), ("empty_range", None, (10, 0))]


@pytest.mark.parametrize("footprint", [1, 2, 3])
@pytest.mark.parametrize("with_pose", [False, True], ids=["no_pose", "pose"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_entry_equals_restatement(footprint, with_pose, case):
    _, count, rng2 = case
    xyz, gray = hostile_list(with_pose)
    assert 4500 <= len(xyz) <= 5500
    k, pose = cam(ROWS, COLS), (POSE if with_pose else None)
    got = V.render_points_host(xyz, gray, k, ROWS, COLS, SCALE, pose7=pose, footprint=footprint, count=count, range2=rng2)
    want = restatement(xyz, gray, len(xyz) if count is None else count, rng2, k, ROWS, COLS, SCALE, pose, footprint)
    assert_same(got, want, f"footprint {footprint}")
    c = got["counts"]
    assert c[0] >= c[1] >= c[2] and c[3] <= c[2] * footprint * footprint


@pytest.mark.parametrize("with_pose", [False, True], ids=["no_pose", "pose"])
def test_the_list_reaches_the_cases(with_pose):
    xyz, gray = hostile_list(with_pose)
    k, pose = cam(ROWS, COLS), (POSE if with_pose else None)
    for f in (1, 2, 3):
        out = V.render_points_host(xyz, gray, k, ROWS, COLS, SCALE, pose7=pose, footprint=f)
        c = out["counts"]
        assert c[0] == len(xyz) and c[0] > c[1] > c[2] > 0 and 0 < c[3] < ROWS * COLS
        covered = out["zkey"] != EMPTY
        assert (out["depth"][covered] == 65535).any(), "no pixel whose depth saturates"
        assert (out["depth"][covered] == 0).any(), "no covered pixel whose depth rounds to 0"
        # duplicates: a winner whose exact copy sits at a higher rank lost to it only by rank
        rank = (out["zkey"][covered] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        _, inverse, copies = np.unique(xyz.view(np.uint32), axis=0, return_inverse=True, return_counts=True)
        inverse = inverse.ravel()
        lowest = np.full(len(copies), len(xyz), np.int64)   # the LOWEST rank of every distinct point
        np.minimum.at(lowest, inverse, np.arange(len(xyz)))
        dup_winners = rank[copies[inverse[rank]] > 1]
        assert len(dup_winners), "no duplicated point wins a pixel"
        assert (lowest[inverse[dup_winners]] == dup_winners).all(), "among equal Z' bits the lower rank must win"
    # partial footprints: with footprint 3 points whose anchor is outside still write border pixels
    uvw = V.camera_project(k, pose, xyz)
    with np.errstate(all="ignore"):
        x0 = np.floor(uvw[:, 0] / uvw[:, 2] + F32(0.5))
        y0 = np.floor(uvw[:, 1] / uvw[:, 2] + F32(0.5))
    for sel in (x0 == -1, x0 == COLS, y0 == -1, y0 == ROWS, x0 == -2, x0 == COLS + 1, x0 < -4, x0 >= COLS + 4):
        assert (sel & (uvw[:, 2] > 0)).any(), "a border case is missing from the list"
    assert not np.isfinite(xyz).all() and (uvw[:, 2] < 0).any()


# ------------------------------------------------------------------------------------------------------------ 2
def test_round_trip_every_pixel_returns_to_its_own():
    rows, cols = 120, 160
    k = cam(rows, cols)
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:rows, 0:cols]
    xy = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float32)
    own = np.arange(rows * cols, dtype=np.uint64).reshape(rows, cols)
    worst_du, worst_dd, misplaced = 0.0, 0, 0
    for _ in range(20):
        depth = rng.integers(2500, 30001, rows * cols).astype(np.uint16)
        pose = random_pose(rng, angle=0.5, shift=1.0)
        xyz = V.camera_back_project(k, pose, xy, depth.astype(np.float32) / F32(SCALE))
        out = V.render_points_host(xyz, np.full(len(xyz), 9, np.uint8), k, rows, cols, SCALE, pose7=pose, footprint=1)
        uvw = V.camera_project(k, pose, xyz)
        worst_du = max(worst_du, float(np.abs(uvw[:, :2] / uvw[:, 2:] - xy).max()))
        misplaced += int(((out["zkey"] & np.uint64(0xFFFFFFFF)) != own).sum())
        worst_dd = max(worst_dd, int(np.abs(out["depth"].astype(np.int64).ravel() - depth.astype(np.int64)).max()))
        assert (out["counts"] == rows * cols).all()
    print(f"round trip: misplaced {misplaced}, largest |u - x| {worst_du:.3g}, largest depth deviation {worst_dd} units")
    assert misplaced == 0, f"{misplaced} points did not return to their own pixel"
    assert worst_dd <= 1, f"a depth deviates by {worst_dd} units"


# ------------------------------------------------------------------------------------------------------------ 3
INVALID = -1


def device_args(**over):
    """A legal argument list of vors_render_points on host stand-ins (a refused call dereferences nothing)."""
    a = dict(n=1, xyz=np.zeros((8, 3), np.float32), gray=np.zeros(8, np.uint8), list_counts=np.zeros(1, np.uint32), capacity=8, ranges=None,
             range_stride=0, cam5=cam(ROWS, COLS), rows=ROWS, cols=COLS, scale=SCALE, poses=None, pose_stride=0, footprint=1,
             zkey=np.zeros(ROWS * COLS + 1, np.uint64), depth=None, gray_out=None, counts=None)
    a.update(over)
    return a


def call_device(a):
    p = lambda x: x if isinstance(x, (int, type(None))) else x.ctypes.data
    return V.lib().vors_render_points(a["n"], p(a["xyz"]), p(a["gray"]), p(a["list_counts"]), a["capacity"], p(a["ranges"]), a["range_stride"],
                                      p(a["cam5"]), a["rows"], a["cols"], a["scale"], p(a["poses"]), a["pose_stride"], a["footprint"],
                                      p(a["zkey"]), p(a["depth"]), p(a["gray_out"]), p(a["counts"]), None)


ZK = np.zeros(8, np.uint64)
REFUSALS = {
    "n_0": dict(n=0), "null_xyz": dict(xyz=None), "null_gray": dict(gray=None), "null_counts": dict(list_counts=None), "null_cam": dict(cam5=None),
    "null_zkey": dict(zkey=None), "misaligned_zkey": dict(zkey=ZK.ctypes.data + 4), "footprint_0": dict(footprint=0), "footprint_4": dict(footprint=4),
    "rows_0": dict(rows=0), "cols_0": dict(cols=0), "rows_negative": dict(rows=-3), "capacity_0": dict(capacity=0), "capacity_negative": dict(capacity=-1),
    "rows_65536": dict(rows=65536, cols=2), "plane_beyond_2_28": dict(rows=20000, cols=20000), "scale_0": dict(scale=0.0), "scale_negative": dict(scale=-5000.0),
    "scale_nan": dict(scale=float("nan")), "pose_stride_27": dict(pose_stride=27), "pose_stride_8": dict(pose_stride=8), "pose_stride_30": dict(pose_stride=30),
    "range_stride_4": dict(range_stride=4), "range_stride_10": dict(range_stride=10), "ranges_misaligned": dict(ranges=ZK.ctypes.data + 2),
    "xyz_misaligned": dict(xyz=ZK.ctypes.data + 2), "list_counts_misaligned": dict(list_counts=ZK.ctypes.data + 1), "poses_misaligned": dict(poses=ZK.ctypes.data + 2),
    "depth_misaligned": dict(depth=ZK.ctypes.data + 1), "counts_misaligned": dict(counts=ZK.ctypes.data + 2),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_device_entry_refusals_come_before_the_device(name):
    st = call_device(device_args(**REFUSALS[name]))
    assert st == INVALID, f"{name}: status {st} ({V.lib().vors_last_error().decode()})"
    assert "render_points" in V.lib().vors_last_error().decode()


def test_host_entry_refusals_write_nothing():
    xyz, gray = hostile_list(False)
    k = cam(ROWS, COLS)
    for kw in (dict(footprint=0), dict(footprint=4), dict(rows=0), dict(cols=0), dict(depth_scale=0.0), dict(depth_scale=float("nan")),
               dict(rows=65536, cols=2)):
        args = dict(rows=ROWS, cols=COLS, depth_scale=SCALE, footprint=1)
        args.update(kw)
        with pytest.raises(V.VorsError):
            V.render_points_host(xyz, gray, k, **args)
    with pytest.raises(V.VorsError):   # capacity 0
        V.render_points_host(np.zeros((0, 3), np.float32), np.zeros(0, np.uint8), k, ROWS, COLS, SCALE)
    lib = V.lib()
    zk = np.full(ROWS * COLS + 1, 5, np.uint64)
    ok = lambda **o: lib.vors_render_points_host(o.get("xyz", xyz.ctypes.data), o.get("gray", gray.ctypes.data), len(xyz), len(xyz), None, k.ctypes.data,
                                                 ROWS, COLS, SCALE, None, o.get("f", 1), o.get("zkey", zk.ctypes.data), None, None, None)
    assert ok(xyz=None) == INVALID and ok(gray=None) == INVALID and ok(zkey=None) == INVALID and ok(zkey=zk.ctypes.data + 4) == INVALID
    assert ok(f=9) == INVALID and (zk == 5).all(), "a refused call wrote the key plane"
    assert ok() == 0 and (zk[:-1] != 5).all() and zk[-1] == 5
