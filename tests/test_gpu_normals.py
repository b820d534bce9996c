"""Surface normals of depth planes on the device (vors_depth_normals, vors_points_normals) against the host entry
(vors_depth_normals_host), which runs the same text (lie.h depth_normal): equality of BITS, and equal counts. GPU only.

Shapes: 3 planes of 37x29 — odd sizes, so a thread's four pixels are a workgroup width apart and the last workgroup has a tail — and 2 of
64x48, where a thread takes four adjacent pixels (cols % 4 == 0, aligned planes). Steps 1, 3 and 8 (8 is wider than a quarter of 29
columns: most pixels of a row use a one-sided difference or have no horizontal neighbour on one side). The depth has 2 % zeros, a blob of
zeros and a depth step.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V

SCALE = 5000.0
JUMP_M = 0.08
SHAPES = {"odd": (3, 37, 29), "wide": (2, 64, 48)}
SHAPE = pytest.mark.parametrize("shape", list(SHAPES))
STEP = pytest.mark.parametrize("step", [1, 3, 8])
POSED = pytest.mark.parametrize("posed", [False, True], ids=["camera_frame", "posed"])


def cam_of(rows, cols):
    return np.array([0.5 * cols - 0.5, 0.5 * rows - 0.5, 0.9 * cols, -0.95 * cols, 0.3], np.float32)  # fv < 0 and a skew


@functools.lru_cache(maxsize=None)
def planes(shape):
    """depth [n, rows, cols] u16: a tilted plane per map, the right third 0.4 m further away, a blob of zeros, 2 % zeros."""
    n, rows, cols = SHAPES[shape]
    rng = np.random.default_rng(rows)
    y, x = np.mgrid[0:rows, 0:cols]
    d = np.empty((n, rows, cols), np.uint16)
    for i in range(n):
        z = 1.2 + 0.3 * i + 0.003 * (1 + i) * x - 0.004 * y
        z[:, 2 * cols // 3:] += 0.4
        q = np.rint(z * SCALE)
        q[rows // 4:rows // 4 + 5, cols // 5:cols // 5 + 6] = 0
        q[rng.random(q.shape) < 0.02] = 0
        d[i] = q
    return d


@functools.lru_cache(maxsize=None)
def poses_of(n):
    rng = np.random.default_rng(11)
    p = rng.normal(size=(n, 7)).astype(np.float32)
    p[:, 3:] /= np.linalg.norm(p[:, 3:], axis=1, keepdims=True)
    return p


@functools.lru_cache(maxsize=None)
def host_planes(shape, step, posed):
    n, rows, cols = SHAPES[shape]
    outs = [V.depth_normals_host(planes(shape)[i], cam_of(rows, cols), SCALE, step, JUMP_M, pose7=poses_of(n)[i] if posed else None) for i in range(n)]
    for o in outs:
        assert 2 * int(o["counts"][2]) >= int(o["counts"][1]) > 0, o["counts"]  # at least half of the pixels with depth get a normal
        assert int(o["counts"][2]) < int(o["counts"][1]), "the depth step and the holes must cost some pixels their normal"
    return np.stack([o["normals"] for o in outs]), np.stack([o["counts"] for o in outs])


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.cpu().numpy().view(np.uint32)


@SHAPE
@STEP
@POSED
def test_plane_form_equals_the_host_bit_for_bit(shape, step, posed):
    import torch
    n, rows, cols = SHAPES[shape]
    want_n, want_c = host_planes(shape, step, posed)
    depth = dev(planes(shape).view(np.int16))
    poses = dev(poses_of(n)) if posed else None
    out = V.depth_normals(depth, cam_of(rows, cols), SCALE, step, JUMP_M, poses=poses, counts=True)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out["normals"]), want_n.view(np.uint32))
    assert np.array_equal(bits(out["counts"]), want_c)
    # counts only (d_normals NULL) and normals only (d_counts NULL)
    only_c = V.depth_normals(depth, cam_of(rows, cols), SCALE, step, JUMP_M, poses=poses, normals=False, counts=True)
    only_n = V.depth_normals(depth, cam_of(rows, cols), SCALE, step, JUMP_M, poses=poses)
    torch.cuda.synchronize()
    assert set(only_c) == {"counts"} and np.array_equal(bits(only_c["counts"]), want_c)
    assert set(only_n) == {"normals"} and np.array_equal(bits(only_n["normals"]), want_n.view(np.uint32))


def test_plane_form_misaligned_planes_take_the_scattered_path():
    """64x48 planes that start 2 bytes off the 8-byte alignment the four-adjacent path needs: same bits."""
    import torch
    n, rows, cols = SHAPES["wide"]
    flat = torch.zeros(n * rows * cols + 1, dtype=torch.int16, device="cuda")
    flat[1:] = dev(planes("wide").view(np.int16)).reshape(-1)
    out = V.depth_normals(flat[1:].view(n, rows, cols), cam_of(rows, cols), SCALE, 3, JUMP_M, counts=True)
    torch.cuda.synchronize()
    want_n, want_c = host_planes("wide", 3, False)
    assert np.array_equal(bits(out["normals"]), want_n.view(np.uint32)) and np.array_equal(bits(out["counts"]), want_c)


@SHAPE
@POSED
def test_list_form(shape, posed):
    """Lists with a count above capacity, ranges that overrun the written prefix, a pixel outside the plane; a sentinel fill proves that
    the ranks outside the range are left untouched."""
    import torch
    n, rows, cols = SHAPES[shape]
    step, cap = 3, 700
    rng = np.random.default_rng(3)
    xs, ys = rng.integers(0, cols, (n, cap)), rng.integers(0, rows, (n, cap))
    xs[:, 5], ys[:, 5] = cols, 1          # outside the plane
    xs[:, 6], ys[:, 6] = 0, rows + 1000
    pixel = (xs | (ys << 16)).astype(np.uint32)
    list_counts = np.array([cap + 50, 300, 0][:n], np.uint32)   # above capacity; a prefix; (odd shape) an empty list
    ranges = np.array([[650, 500], [100, 4000], [0, 10]][:n], np.uint32)  # each overruns the written prefix
    cam, depth = cam_of(rows, cols), planes(shape)
    poses = poses_of(n) if posed else None
    for rg in (None, ranges):
        want = np.full((n, cap, 3), -7.0, np.float32)
        want_c = np.zeros((n, 3), np.uint32)
        for i in range(n):
            o = V.depth_normals_host(depth[i], cam, SCALE, step, JUMP_M, pose7=None if poses is None else poses[i], pixel=pixel[i],
                                     count=int(list_counts[i]), range2=None if rg is None else rg[i], normals=want[i])
            want_c[i] = o["counts"]
        out = V.points_normals(dev(depth.view(np.int16)), dev(pixel.view(np.int32)), dev(list_counts.view(np.int32)), cam, SCALE, step, JUMP_M,
                               poses=None if poses is None else dev(poses), ranges=None if rg is None else dev(rg.view(np.int32)),
                               normals=torch.full((n, cap, 3), -7.0, device="cuda"), counts=True)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out["normals"]), want.view(np.uint32))
        assert np.array_equal(bits(out["counts"]), want_c)
        first = 0 if rg is None else 650
        assert want_c[0, 0] == cap - first and (want[0, :first] == -7.0).all() and (want[0, first:] != -7.0).all()
        assert (want[1, 300:] == -7.0).all(), "ranks beyond the list's count are never written"
        assert not want[0, 5].any() or rg is not None  # the pixel outside the plane: three zeros where it is in range
    # the list form is the plane form gathered
    plane_n, _ = host_planes(shape, step, posed)
    inside = (xs[0] < cols) & (ys[0] < rows)
    o = V.depth_normals_host(depth[0], cam, SCALE, step, JUMP_M, pose7=None if poses is None else poses[0], pixel=pixel[0])
    assert np.array_equal(o["normals"][inside].view(np.uint32), plane_n[0][ys[0][inside], xs[0][inside]].view(np.uint32))


def test_device_refusals_enqueue_nothing():
    import torch
    n, rows, cols = SHAPES["odd"]
    depth = dev(planes("odd").view(np.int16))
    cam = cam_of(rows, cols)
    sentinel = torch.full((n, rows, cols, 3), 5.0, device="cuda")
    for kw in (dict(step=0), dict(step=9), dict(jump_m=-1.0), dict(jump_m=float("nan")), dict(depth_scale=0.0)):
        args = dict(depth_scale=SCALE, step=1, jump_m=0.1)
        args.update(kw)
        with pytest.raises(V.VorsError):
            V.depth_normals(depth, cam, normals=sentinel, **args)
    with pytest.raises(V.VorsError):
        V.depth_normals(depth, cam, SCALE, 1, 0.1, normals=False, counts=False)  # at least one output
    pixel, counts = torch.zeros((n, 8), dtype=torch.int32, device="cuda"), torch.full((n,), 8, dtype=torch.int32, device="cuda")
    with pytest.raises(V.VorsError):
        V.points_normals(depth, pixel, counts, cam, SCALE, 0, 0.1)
    with pytest.raises(V.VorsError):
        V.points_normals(depth, pixel, counts, cam, SCALE, 1, 0.1, normals=False)
    torch.cuda.synchronize()
    assert (sentinel == 5.0).all()
