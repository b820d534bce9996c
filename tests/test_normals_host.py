"""Surface normals of depth planes on the host (vors_depth_normals_host; needs no GPU): lie.h depth_normal, the text the kernels run.

Tilted planes, measured here (the largest angle in degrees between the f32 normal and a float64 numpy evaluation of the same stencil on
the same quantised depths, 120x160, depth scale 5000, fu = 130, fv = 131):

    tilt A  step 1: 0.00131   step 2: 0.000771   step 4: 0.000324
    tilt B  step 1: 0.00127   step 2: 0.000652   step 4: 0.000369

The differences P(x + step) - P(x - step) cancel all but ~step / f of the operands, so the f32 rounding of a back-projected point, eps |P|,
shows in the tangents as an angle of about eps f / step; other focal lengths scale it. The bound asserted is 4 x the largest figure above.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-odometry-rs_amd"))
import vors_amd  # noqa: E402

SCALE = 5000.0
CAM = np.array([79.5, 59.5, 130.0, 131.0, 0.0], np.float32)
ROWS, COLS = 120, 160
MEASURED_MAX_ANGLE_DEG = 0.00131  # the table above
ANGLE_BOUND_DEG = 4 * MEASURED_MAX_ANGLE_DEG


def normals(depth, step=1, jump_m=1.0, cam=CAM, scale=SCALE, **kw):
    return vors_amd.depth_normals_host(depth, cam, scale, step, jump_m, **kw)


def tilted_depth(normal, dist, cam=CAM, rows=ROWS, cols=COLS, scale=SCALE):
    """The plane normal . X = dist seen through cam, quantised like a depth map."""
    cu, cv, fu, fv, skew = [float(v) for v in cam]
    x, y = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    ry = (y - cv) / fv
    rx = ((x - cu) - skew * ry) / fu
    z = dist / (normal[0] * rx + normal[1] * ry + normal[2])
    d = np.rint(z * scale)
    assert d.min() >= 1 and d.max() <= 65535
    return d.astype(np.uint16)


TILTS = {"A": ((0.35, -0.2, 1.0), 1.6), "B": ((-0.15, 0.5, 1.0), 2.2)}


def reference64(depth, cam, step, jump_m, scale=SCALE):
    """The stencil of depth_normal in float64, vectorised -> (normals [rows, cols, 3], has_normal [rows, cols])."""
    cu, cv, fu, fv, skew = [float(v) for v in cam]
    rows, cols = depth.shape
    z = depth.astype(np.float64) / scale
    x, y = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    py = (y - cv) * z / fv
    px = ((x - cu) * z - skew * py) / fu
    P = np.stack([px, py, z], -1)
    ok = depth > 0

    def shifted(a, dy, dx, fill):
        out = np.full_like(a, fill)
        ys, yd = (slice(dy, None), slice(None, rows - dy)) if dy >= 0 else (slice(None, dy), slice(-dy, None))
        xs, xd = (slice(dx, None), slice(None, cols - dx)) if dx >= 0 else (slice(None, dx), slice(-dx, None))
        out[yd, xd] = a[ys, xs]
        return out

    def tangent(dy, dx):
        use, pts = [], []
        for sgn in (-1, 1):
            okn = shifted(ok, sgn * dy, sgn * dx, False)
            zn = shifted(z, sgn * dy, sgn * dx, 0.0)
            use.append(okn & (np.abs(zn - z) <= jump_m))
            pts.append(shifted(P, sgn * dy, sgn * dx, 0.0))
        a = np.where(use[0][..., None], pts[0], P)
        b = np.where(use[1][..., None], pts[1], P)
        return b - a, use[0] | use[1]

    tx, okx = tangent(0, step)
    ty, oky = tangent(step, 0)
    m = np.cross(ty, tx)
    l2 = (m * m).sum(-1)
    has = ok & okx & oky & (l2 > 0)
    n = m / np.sqrt(np.where(has, l2, 1.0))[..., None]
    flip = (n * P).sum(-1) > 0
    n = np.where(flip[..., None], -n, n)
    return np.where(has[..., None], n, 0.0), has


def angles_deg(a, b):
    c = (a.astype(np.float64) * b).sum(-1) / np.linalg.norm(a.astype(np.float64), axis=-1) / np.linalg.norm(b, axis=-1)
    return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))


def enough_normals(out):
    c = out["counts"]
    assert 2 * int(c[2]) >= int(c[1]), f"fewer than half of the pixels with depth get a normal: {c}"


def test_constant_plane_is_exactly_minus_z():
    d = np.full((31, 45), 7500, np.uint16)
    for step in (1, 2, 8):
        out = normals(d, step)
        want = np.zeros((31, 45, 3), np.float32)
        want[..., 2] = -1.0
        assert np.array_equal(out["normals"].view(np.uint32), want.view(np.uint32)), step  # +0, +0, -1: bit for bit
        assert out["counts"].tolist() == [31 * 45, 31 * 45, 31 * 45]


def test_one_sided_at_the_four_borders():
    d = tilted_depth(*TILTS["A"], rows=24, cols=30)
    for step in (1, 3):
        out = normals(d, step)
        ref, has = reference64(d, CAM, step, 1.0)
        assert has.all() and int(out["counts"][2]) == d.size
        for border in (np.s_[:step, :], np.s_[-step:, :], np.s_[:, :step], np.s_[:, -step:]):
            assert angles_deg(out["normals"][border], ref[border]).max() <= ANGLE_BOUND_DEG
    # no neighbour at all on an axis: no normal (a single row; a step as wide as the plane)
    assert normals(np.full((1, 9), 5000, np.uint16))["counts"].tolist() == [9, 9, 0]
    out = normals(np.full((9, 5), 5000, np.uint16), step=5)
    assert out["counts"].tolist() == [45, 45, 0] and not out["normals"].any()


def test_centre_and_neighbour_without_depth():
    d = tilted_depth(*TILTS["B"], rows=20, cols=20)
    d[10, 10] = 0
    out = normals(d)
    ref, has = reference64(d, CAM, 1, 1.0)
    assert np.array_equal(out["normals"][10, 10].view(np.uint32), np.zeros(3, np.uint32))  # three +0.0f
    assert out["counts"].tolist() == [400, 399, 399]
    # its four neighbours fall back to one side and still agree with the one-sided stencil
    for y, x in ((10, 9), (10, 11), (9, 10), (11, 10)):
        assert has[y, x] and angles_deg(out["normals"][y, x], ref[y, x]) <= ANGLE_BOUND_DEG
    assert (angles_deg(out["normals"][has], ref[has]) <= ANGLE_BOUND_DEG).all()
    enough_normals(out)


def test_depth_jumps():
    minus_z = np.array([0.0, 0.0, -1.0], np.float32)
    # a step on ONE side: two fronto-parallel halves a metre apart; the columns at the edge use their own half only
    d = np.full((12, 16), 5000, np.uint16)
    d[:, 8:] = 10000
    out = normals(d, step=1, jump_m=0.1)
    assert out["counts"].tolist() == [192, 192, 192]
    assert np.array_equal(out["normals"].reshape(-1, 3), np.tile(minus_z, (192, 1)))
    # without the test the edge columns would tilt
    assert not np.array_equal(normals(d, step=1, jump_m=2.0)["normals"][:, 7:9].reshape(-1, 3), np.tile(minus_z, (24, 1)))
    # a step on BOTH sides: one column alone at another depth has no horizontal neighbour, so no normal
    d = np.full((12, 16), 5000, np.uint16)
    d[:, 5] = 15000
    out = normals(d, step=1, jump_m=0.1)
    assert out["counts"].tolist() == [192, 192, 192 - 12]
    assert not out["normals"][:, 5].any()
    assert np.array_equal(np.delete(out["normals"], 5, axis=1).reshape(-1, 3), np.tile(minus_z, (180, 1)))
    # the comparison is <=: a neighbour exactly jump_m away is used (1.0 m vs 1.5 m, both exact in f32)
    d = np.full((3, 3), 5000, np.uint16)
    d[:, 2] = 7500
    assert int(normals(d, 1, 0.5)["counts"][2]) == 9
    enough_normals(out)


@pytest.mark.parametrize("tilt", sorted(TILTS))
@pytest.mark.parametrize("step", [1, 2, 4])
def test_tilted_planes_against_float64(tilt, step):
    d = tilted_depth(*TILTS[tilt])
    out = normals(d, step)
    ref, has = reference64(d, CAM, step, 1.0)
    assert has.all() and out["counts"].tolist() == [d.size] * 3
    n = out["normals"]
    worst = angles_deg(n, ref).max()
    print(f"tilt {tilt} step {step}: largest angle {worst:.3g} deg")
    assert worst <= ANGLE_BOUND_DEG
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=-1) - 1.0).max() <= 1e-6
    # ... and it is the plane's normal, up to the quantisation of the depth (1 / 5000 m over 2 step pixels)
    want = -np.array(TILTS[tilt][0]) / np.linalg.norm(TILTS[tilt][0])
    assert np.median(angles_deg(n, np.broadcast_to(want, n.shape))) < 1.0
    enough_normals(out)


def test_negative_focal_length_and_skew_still_face_the_camera():
    for cam in (np.array([79.5, 59.5, 130.0, -131.0, 0.0], np.float32), np.array([79.5, 59.5, -130.0, 131.0, 0.7], np.float32)):
        d = tilted_depth(*TILTS["A"], cam=cam, rows=40, cols=50)
        out = normals(d, 2, cam=cam)
        assert int(out["counts"][2]) == d.size
        y, x = np.mgrid[0:40, 0:50]
        P = vors_amd.camera_back_project(cam, None, np.stack([x, y], -1).reshape(-1, 2).astype(np.float32),
                                         (1.0 / (SCALE / d.astype(np.float32))).reshape(-1))
        assert ((out["normals"].reshape(-1, 3).astype(np.float64) * P).sum(-1) < 0).all()
        ref, _ = reference64(d, cam, 2, 1.0)
        assert angles_deg(out["normals"], ref).max() <= ANGLE_BOUND_DEG
        enough_normals(out)


def test_pose_rotates_and_does_not_translate():
    d = tilted_depth(*TILTS["B"], rows=30, cols=40)
    q = np.array([0.1, -0.2, 0.3, 0.0], np.float64)
    q[3] = np.sqrt(1.0 - (q[:3] ** 2).sum())
    pose = np.concatenate([[5.0, -7.0, 11.0], q]).astype(np.float32)
    cam_frame = normals(d)["normals"]
    world = normals(d, pose7=pose)["normals"]
    no_shift = normals(d, pose7=np.concatenate([[0, 0, 0], pose[3:]]).astype(np.float32))["normals"]
    assert np.array_equal(world.view(np.uint32), no_shift.view(np.uint32))  # the translation is not read
    qv, w = pose[3:6].astype(np.float64), float(pose[6])
    n = cam_frame.astype(np.float64)
    t = 2.0 * np.cross(qv, n)
    want = n + w * t + np.cross(qv, t)
    assert np.abs(world - want).max() <= 1e-6
    ident = normals(d, pose7=np.array([1, 2, 3, 0, 0, 0, 1], np.float32))["normals"]
    assert np.abs(ident - cam_frame).max() <= 1e-7


def test_list_form_is_the_plane_form_gathered():
    rng = np.random.default_rng(5)
    d = tilted_depth(*TILTS["A"], rows=33, cols=47)
    d[rng.random(d.shape) < 0.03] = 0
    plane = normals(d, 2, 0.05)
    enough_normals(plane)
    xs, ys = rng.integers(0, 47, 300), rng.integers(0, 33, 300)
    xs[7], ys[7] = 47, 3     # outside the plane: no normal
    xs[8], ys[8] = 2, 40000
    pixel = (xs | (ys << 16)).astype(np.uint32)
    lst = normals(d, 2, 0.05, pixel=pixel)
    want = np.zeros((300, 3), np.float32)
    inside = (xs < 47) & (ys < 33)
    want[inside] = plane["normals"][ys[inside], xs[inside]]
    assert np.array_equal(lst["normals"].view(np.uint32), want.view(np.uint32))
    has_depth = np.zeros(300, bool)
    has_depth[inside] = d[ys[inside], xs[inside]] > 0
    assert lst["counts"].tolist() == [300, int(has_depth.sum()), int(want.any(-1).sum())]
    # count clipped to capacity, a range that overruns the prefix, everything outside the range left untouched
    sentinel = np.full((300, 3), 123.0, np.float32)
    out = normals(d, 2, 0.05, pixel=pixel, count=250, range2=(200, 1000), normals=sentinel.copy())
    assert np.array_equal(out["normals"][200:250], want[200:250]) and int(out["counts"][0]) == 50
    assert np.array_equal(out["normals"][:200], sentinel[:200]) and np.array_equal(out["normals"][250:], sentinel[250:])
    out = normals(d, 2, 0.05, pixel=pixel, count=100000, normals=sentinel.copy())
    assert np.array_equal(out["normals"].view(np.uint32), want.view(np.uint32))
    out = normals(d, 2, 0.05, pixel=pixel, range2=(400, 5), normals=sentinel.copy())
    assert np.array_equal(out["normals"], sentinel) and out["counts"].tolist() == [0, 0, 0]


def test_refusals():
    import ctypes as C
    lib = vors_amd.lib()
    d = np.full((6, 8), 5000, np.uint16)
    px = np.zeros(4, np.uint32)
    sentinel = np.full((6, 8, 3), 9.0, np.float32)
    out = sentinel.copy()
    counts = np.full(3, 77, np.uint32)
    p = vors_amd._ptr

    def call(depth=d, cam=CAM, rows=6, cols=8, scale=SCALE, step=1, jump=0.1, pixel=None, count=0, cap=0, nrm=out, cnt=counts):
        return lib.vors_depth_normals_host(p(depth), p(cam), rows, cols, scale, step, jump, None, p(pixel), count, cap, None, p(nrm), p(cnt))

    assert call() == 0
    out[:] = sentinel
    counts[:] = 77
    bad = [dict(depth=None), dict(cam=None), dict(nrm=None, cnt=None), dict(step=0), dict(step=9), dict(jump=-0.001), dict(jump=float("nan")),
           dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(rows=0), dict(cols=0), dict(rows=65536), dict(rows=65535, cols=65535),
           dict(pixel=px, count=4, cap=0), dict(pixel=px, count=4, cap=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw  # VORS_ERR_INVALID_ARGUMENT
        assert lib.vors_last_error().decode().startswith("depth_normals_host:"), kw
        assert np.array_equal(out, sentinel) and counts.tolist() == [77, 77, 77], kw  # nothing written
    odd = np.zeros(2 * 48 + 2, np.uint8)  # a depth pointer off its alignment
    assert lib.vors_depth_normals_host(C.c_void_p(odd.ctypes.data | 1), p(CAM), 6, 8, SCALE, 1, 0.1, None, None, 0, 0, None, p(out), p(counts)) == -1
    assert call(nrm=None) == 0 and call(cnt=None) == 0  # one output is enough
    assert vors_amd.lib().vors_abi_version() == 5
