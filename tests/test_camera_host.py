"""Camera::back_project / Camera::project on the host (vors_camera_back_project, vors_camera_project). No GPU needed: the entries are host
arithmetic, the lie.h texts the point-cloud kernel runs per point.

Tolerance of the float64 comparison: 4 ulp of float32 at the magnitude of the LARGEST TERM of the evaluation, where the terms are every
intermediate value of the float64 restatement below — camera.rs:135-140 and `pose * point` as nalgebra evaluates it (t = 2 qv x p;
p' = p + w t + qv x t; + translation). An ulp at magnitude m is at most 2^-23 m.
Round trip: project(back_project(xy, d)) / w must return xy within 1e-3 px for depths 0.3 - 10 m. With |t| <= 0.3 m the world coordinates are
at most |P| + 0.3, each carries a few roundings of 2^-24 relative, and a pixel moves by f / z per metre: 525 / 0.3 * 4 * 6e-8 * 0.7 = 3e-4 px
at the near end, 525 / 10 * 4 * 6e-8 * 13 = 1.6e-4 px at the far end."""
import numpy as np
import pytest

import vors_amd as V

CAMS = {"fr1": (318.6, 255.3, 517.3, 516.5, 0.0), "skewed": (318.6, 255.3, 517.3, 516.5, 1.75), "quarter": (79.275, 63.45, 129.325, 129.125, -0.5)}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def unit_pose(rng, angle, dist):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    q = np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]]).astype(np.float32)
    t = rng.normal(size=3)
    t = (dist * t / np.linalg.norm(t)).astype(np.float32)
    return np.concatenate([t, q]).astype(np.float32)


def samples(rng, n, cols=640, rows=480):
    xy = np.stack([rng.integers(0, cols, n), rng.integers(0, rows, n)], axis=1).astype(np.float32)
    depth = rng.uniform(0.3, 10.0, n).astype(np.float32)
    return xy, depth


def back_project64(cam5, pose7, xy, depth):
    """float64 restatement on the float32 inputs -> (points [n, 3], largest |term| per point [n])."""
    cu, cv, fu, fv, sk = (np.float64(np.float32(c)) for c in cam5)
    px, py, z = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64), depth.astype(np.float64)
    terms = [z, (py - cv) * z]
    y = (py - cv) * z / fv
    a, b = (px - cu) * z, sk * y
    x = (a - b) / fu
    terms += [y, a, b, a - b, x]
    P = np.stack([x, y, z], axis=1)
    if pose7 is not None:
        p7 = np.asarray(pose7, np.float32).astype(np.float64)
        t, qv, w = p7[:3], p7[3:6], p7[6]
        c1 = np.cross(np.broadcast_to(qv, P.shape), P)
        tt = 2.0 * c1
        c2 = np.cross(np.broadcast_to(qv, P.shape), tt)
        R = tt * w + c2 + P
        terms += [np.abs(qv).max() * np.abs(P).max(axis=1), np.abs(c1).max(axis=1), np.abs(tt).max(axis=1), np.abs(tt * w).max(axis=1),
                  np.abs(c2).max(axis=1), np.abs(R).max(axis=1), np.full(len(P), np.abs(t).max())]
        P = R + t
    terms.append(np.abs(P).max(axis=1))
    return P, np.max(np.abs(np.stack(terms)), axis=0)


@pytest.mark.parametrize("cam", list(CAMS))
def test_back_project_against_the_float64_restatement(cam):
    rng = np.random.default_rng(7)
    xy, depth = samples(rng, 4000)
    for pose in (None, unit_pose(rng, 0.0, 0.0), unit_pose(rng, 0.3, 0.3), unit_pose(rng, 2.5, 3.0)):
        got = V.camera_back_project(CAMS[cam], pose, xy, depth)
        assert got.dtype == np.float32 and got.shape == (4000, 3)
        want, largest = back_project64(CAMS[cam], pose, xy, depth)
        err = np.abs(got.astype(np.float64) - want).max(axis=1)
        bound = 4.0 * 2.0 ** -23 * largest
        print(f"{cam} pose {None if pose is None else pose.round(3).tolist()}: max err / bound = {(err / bound).max():.3f}")
        assert (err <= bound).all(), (cam, pose)


@pytest.mark.parametrize("cam", list(CAMS))
def test_project_of_back_project_returns_the_pixel(cam):
    rng = np.random.default_rng(8)
    xy, depth = samples(rng, 4000)
    for pose in (None, unit_pose(rng, 0.0, 0.0), unit_pose(rng, 0.3, 0.3), unit_pose(rng, 0.1, 0.05)):
        uvw = V.camera_project(CAMS[cam], pose, V.camera_back_project(CAMS[cam], pose, xy, depth))
        assert uvw.dtype == np.float32 and uvw.shape == (4000, 3)
        uv = uvw[:, :2].astype(np.float64) / uvw[:, 2:3].astype(np.float64)
        err = np.abs(uv - xy).max()
        print(f"{cam} pose {None if pose is None else pose.round(3).tolist()}: max |uv - xy| = {err:.3e} px")
        assert err <= 1e-3, (cam, pose)
        assert np.abs(uvw[:, 2].astype(np.float64) - depth).max() <= 1e-5 * 10.0   # w is the depth in the camera frame


def test_project_against_the_float64_restatement():
    rng = np.random.default_rng(9)
    cam = CAMS["skewed"]
    pose = unit_pose(rng, 0.7, 1.2)
    P = rng.uniform(-3, 3, (2000, 3)).astype(np.float32)
    p7 = pose.astype(np.float64)
    t, qv, w = p7[:3], -p7[3:6], p7[6]   # rotation.inverse() * (translation.inverse() * point), camera.rs:70-72
    d = P.astype(np.float64) - t
    tt = 2.0 * np.cross(np.broadcast_to(qv, d.shape), d)
    c = tt * w + np.cross(np.broadcast_to(qv, d.shape), tt) + d
    cu, cv, fu, fv, sk = (np.float64(np.float32(v)) for v in cam)
    want = np.stack([fu * c[:, 0] + sk * c[:, 1] + cu * c[:, 2], fv * c[:, 1] + cv * c[:, 2], c[:, 2]], axis=1)   # camera.rs:126-132
    got = V.camera_project(cam, pose, P).astype(np.float64)
    # the largest term is at most fu * |c| (a focal length times a coordinate of at most |P| + |t|)
    bound = 8.0 * 2.0 ** -23 * float(np.float32(cam[2])) * (np.abs(P).max() * np.sqrt(3.0) + 1.2)
    assert np.abs(got - want).max() <= bound


@pytest.mark.parametrize("cam", list(CAMS))
def test_null_pose_is_the_identity_bit_for_bit(cam):
    rng = np.random.default_rng(10)
    xy, depth = samples(rng, 4000)
    xy[:4] = [[0, 0], [639, 479], [319, 255], [0, 479]]
    ident = np.array([0, 0, 0, 0, 0, 0, 1], np.float32)
    a, b = V.camera_back_project(CAMS[cam], None, xy, depth), V.camera_back_project(CAMS[cam], ident, xy, depth)
    assert (bits(a) == bits(b)).all()
    # ... and the camera-frame bits are those of camera.rs:135-140 evaluated in float32, operation by operation
    cu, cv, fu, fv, sk = (np.float32(c) for c in CAMS[cam])
    z = depth
    y = (xy[:, 1] - cv) * z / fv
    x = ((xy[:, 0] - cu) * z - sk * y) / fu
    assert (bits(a) == bits(np.stack([x, y, z], axis=1))).all()
    pa, pb = V.camera_project(CAMS[cam], None, a), V.camera_project(CAMS[cam], ident, a)
    assert (bits(pa) == bits(pb)).all()


def test_empty_input_is_legal():
    for pose in (None, np.array([0, 0, 0, 0, 0, 0, 1], np.float32)):
        out = V.camera_back_project(CAMS["fr1"], pose, np.empty((0, 2), np.float32), np.empty(0, np.float32))
        assert out.shape == (0, 3)
        assert V.camera_project(CAMS["fr1"], pose, out).shape == (0, 3)
    with pytest.raises(V.VorsError):
        V.camera_back_project(CAMS["fr1"], None, np.zeros((3, 2), np.float32), np.zeros(2, np.float32))
