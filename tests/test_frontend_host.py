"""The sensor front end on the host (vors_undistort_frame_host, vors_undistort_source_host, vors_register_depth_host): the
texts the device kernels run, checked here against numpy on cases whose answer is known exactly, and against a float64 restatement of the
source-coordinate formula. Needs no GPU.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import vors_amd as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS = 48, 64
INVALID = -1  # VORS_ERR_INVALID_ARGUMENT


def exact_cam(rows=ROWS, cols=COLS):
    """Power-of-two focals and a half-integer centre: every step of the source coordinate is exact in f32."""
    return np.array([cols / 2 - 0.5, rows / 2 - 0.5, 64.0, 32.0, 0.0], np.float32)


# the two distorted cases: (rows, cols, camera, coefficients)
def small_case():
    rows, cols = 37, 53
    return rows, cols, np.array([0.5 * cols - 0.5, 0.5 * rows - 0.5, 0.9 * cols, -0.95 * cols, 0.3], np.float32), \
        np.array([0.2, -0.3, 0.01, -0.02, 0.1], np.float32)


def large_case():
    return 480, 640, np.array([318.6, 255.3, 517.3, 516.5, 0.0], np.float32), np.array([0.26, -0.95, -0.005, 0.003, 1.16], np.float32)


CASES = {"small": small_case, "large": large_case}
# The bound of the coordinate test: 4 x the maximum |twin - float64 restatement| measured (profiles/frontend_summary.md: 6.5997e-06 px on
# the small case, 1.1423e-04 px on the large one), the factor for f32 rounding that varies with the compiler's constant folding.
COORD_BOUND = {"small": 4 * 6.5997e-06, "large": 4 * 1.1423e-04}


@functools.lru_cache(maxsize=None)
def frame(rows=ROWS, cols=COLS, seed=0):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    d = rng.integers(1, 60000, (rows, cols)).astype(np.uint16)
    d[rng.random(d.shape) < 0.02] = 0
    return g, d


def source64(cam_in, dist, cam_out, rows, cols):
    """The formula of include/vors_hip.h 2f in float64, from the f32 values of the cameras and coefficients."""
    cu_i, cv_i, fu_i, fv_i, sk_i = [np.float64(v) for v in np.asarray(cam_in, np.float32)]
    cu_o, cv_o, fu_o, fv_o, sk_o = [np.float64(v) for v in np.asarray(cam_out, np.float32)]
    k1, k2, p1, p2, k3 = [np.float64(v) for v in np.asarray(dist, np.float32)]
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    Y = (y - cv_o) / fv_o
    X = ((x - cu_o) - sk_o * Y) / fu_o
    xx, yy, xy = X * X, Y * Y, X * Y
    r2 = xx + yy
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    Xd = (X * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx)
    Yd = (Y * rad + p1 * (r2 + 2.0 * yy)) + (2.0 * p2) * xy
    return (fu_i * Xd + sk_i * Yd) + cu_i, fv_i * Yd + cv_i


def pixels(rows, cols):
    y, x = np.mgrid[0:rows, 0:cols]
    return np.stack([x.ravel(), y.ravel()], axis=1).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ undistortion
def test_identity_returns_the_input_exactly():
    g, d = frame()
    cam = exact_cam()
    for dist in (None, np.zeros(5, np.float32)):
        for border in (0, 1):
            o = V.undistort_frame_host(g, d, cam, dist, cam, ROWS, COLS, border=border)
            assert np.array_equal(o["gray"], g) and np.array_equal(o["depth"], d)
            assert tuple(o["counts"]) == (ROWS * COLS, ROWS * COLS, int((d != 0).sum()))
            assert np.array_equal(o["map"].reshape(-1, 2), pixels(ROWS, COLS).astype(np.float32))


def test_integer_shift():
    g, d = frame()
    cam = exact_cam()
    out = cam.copy()
    out[0] -= 3
    for border in (0, 1):
        o = V.undistort_frame_host(g, d, cam, None, out, ROWS, COLS, border=border)
        assert np.array_equal(o["gray"][:, :-3], g[:, 3:]) and np.array_equal(o["depth"][:, :-3], d[:, 3:])
        assert (o["depth"][:, -3:] == 0).all(), "depth is never invented, whatever the border mode"
        if border == 0:
            assert (o["gray"][:, -3:] == 0).all()
        else:
            assert np.array_equal(o["gray"][:, -3:], np.repeat(g[:, -1:], 3, axis=1))
        assert int(o["counts"][1]) == ROWS * (COLS - 3), "the inside count does not depend on the border mode"


def test_half_pixel_shift():
    g, d = frame()
    cam = exact_cam()
    out = cam.copy()
    out[0] -= 0.5
    o = V.undistort_frame_host(g, d, cam, None, out, ROWS, COLS)
    gi = g.astype(np.int32)
    assert np.array_equal(o["gray"][:, :-1], ((gi[:, :-1] + gi[:, 1:] + 1) >> 1).astype(np.uint8))
    assert np.array_equal(o["depth"][:, :-1], d[:, 1:])
    assert (o["gray"][:, -1] == 0).all() and (o["depth"][:, -1] == 0).all()
    # and rows likewise
    out = cam.copy()
    out[1] -= 0.5
    o = V.undistort_frame_host(g, d, cam, None, out, ROWS, COLS)
    assert np.array_equal(o["gray"][:-1], ((gi[:-1] + gi[1:] + 1) >> 1).astype(np.uint8)) and np.array_equal(o["depth"][:-1], d[1:])


@pytest.mark.parametrize("case", list(CASES))
def test_coordinates_against_float64(case):
    rows, cols, cam, dist = CASES[case]()
    uv = V.undistort_source_host(cam, dist, cam, pixels(rows, cols)).astype(np.float64)
    u64, v64 = source64(cam, dist, cam, rows, cols)
    err = max(np.abs(uv[:, 0] - u64.ravel()).max(), np.abs(uv[:, 1] - v64.ravel()).max())
    print(f"{case}: max |twin - float64| = {err:.4e} px (bound {COORD_BOUND[case]:.4e})")
    assert err <= COORD_BOUND[case]
    # the frame entry's coordinate table is the same text
    g, d = frame(rows, cols, 1)
    o = V.undistort_frame_host(g, d, cam, dist, cam, rows, cols)
    assert np.array_equal(o["map"].reshape(-1, 2).view(np.uint32), V.undistort_source_host(cam, dist, cam, pixels(rows, cols)).view(np.uint32))
    # non-vacuity: the distortion moves a fair share of the pixels outside, and not all of them
    inside64 = (u64 >= 0) & (u64 <= cols - 1) & (v64 >= 0) & (v64 <= rows - 1)
    n_in = int(o["counts"][1])
    assert 0.5 * rows * cols < n_in < rows * cols
    assert abs(n_in - int(inside64.sum())) <= 0.01 * rows * cols


def test_distorted_frame_against_a_numpy_restatement():
    """Grey and depth of the small distorted case from the twin's own coordinates, restated with numpy in f32."""
    rows, cols, cam, dist = small_case()
    g, d = frame(rows, cols, 2)
    for border in (0, 1):
        o = V.undistort_frame_host(g, d, cam, dist, cam, rows, cols, border=border)
        u, v = o["map"][..., 0], o["map"][..., 1]
        inside = (u >= 0) & (u <= cols - 1) & (v >= 0) & (v <= rows - 1)
        uc, vc = (np.clip(u, 0, cols - 1), np.clip(v, 0, rows - 1)) if border else (np.where(inside, u, 0), np.where(inside, v, 0))
        x0, y0 = np.floor(uc).astype(int), np.floor(vc).astype(int)
        a, b = (uc - np.floor(uc)).astype(np.float32), (vc - np.floor(vc)).astype(np.float32)
        x1, y1 = np.minimum(x0 + 1, cols - 1), np.minimum(y0 + 1, rows - 1)
        f = g.astype(np.float32)
        t0 = f[y0, x0] + a * (f[y0, x1] - f[y0, x0])
        t1 = f[y1, x0] + a * (f[y1, x1] - f[y1, x0])
        val = np.floor((t0 + b * (t1 - t0)) + np.float32(0.5)).clip(0, 255).astype(np.uint8)
        want = val if border else np.where(inside, val, 0)
        assert np.array_equal(o["gray"], want)
        xs, ys = np.floor(u + np.float32(0.5)), np.floor(v + np.float32(0.5))
        ok = (xs >= 0) & (xs <= cols - 1) & (ys >= 0) & (ys <= rows - 1)
        want_d = np.where(ok, d[np.where(ok, ys, 0).astype(int), np.where(ok, xs, 0).astype(int)], 0)
        assert np.array_equal(o["depth"], want_d)
        assert tuple(o["counts"]) == (rows * cols, int(inside.sum()), int((want_d != 0).sum()))


def test_depth_is_never_interpolated():
    rows, cols, cam, dist = small_case()
    y, x = np.mgrid[0:rows, 0:cols]
    z = 1.2 + 0.003 * x - 0.004 * y
    z[:, 2 * cols // 3:] += 0.4  # a 0.4 m step
    d = np.rint(z * 5000.0).astype(np.uint16)
    near_max, far_min = int(d[:, :2 * cols // 3].max()), int(d[:, 2 * cols // 3:].min())
    assert far_min - near_max > 1000
    out = cam.copy()
    out[0] -= 0.37  # a fractional shift on top of the distortion: a bilinear sample would mix the two sides
    o = V.undistort_frame_host(None, d, cam, dist, out, rows, cols)
    assert set(o) == {"depth", "map", "counts"}
    vals = np.unique(o["depth"])
    assert np.isin(vals[vals != 0], d).all(), "every output depth value occurs in the input"
    assert not ((o["depth"] > near_max) & (o["depth"] < far_min)).any(), "no value between the two sides of the step"
    assert (o["depth"] >= far_min).any() and ((o["depth"] <= near_max) & (o["depth"] > 0)).any()


def test_output_size_different_from_input():
    rows, cols, cam, dist = small_case()
    g, d = frame(rows, cols, 3)
    out = cam.copy()
    out[0] -= 3.0  # the crop 31x47 at offset (3, 3) of the full-size ideal image
    out[1] -= 3.0
    full = V.undistort_frame_host(g, d, cam, dist, cam, rows, cols)
    crop = V.undistort_frame_host(g, d, cam, dist, out, 31, 47)
    assert crop["gray"].shape == (31, 47) and crop["map"].shape == (31, 47, 2) and int(crop["counts"][0]) == 31 * 47
    # (cu - 3 and cv - 3 are exact here, but (x - (cu - 3)) and ((x + 3) - cu) may round differently once divided: compare coordinates
    # to the bound of the coordinate test, and the planes wherever the coordinates agree in bits)
    a, b = crop["map"], full["map"][3:34, 3:50]
    assert np.abs(a.astype(np.float64) - b).max() <= COORD_BOUND["small"]
    same = (a.view(np.uint32) == b.view(np.uint32)).all(axis=2)
    assert same.mean() > 0.5
    assert np.array_equal(crop["gray"][same], full["gray"][3:34, 3:50][same]) and np.array_equal(crop["depth"][same], full["depth"][3:34, 3:50][same])


# ------------------------------------------------------------------------------------------------------------ registration
def test_registration_identity():
    _, d = frame()
    d = np.minimum(d, 12000)
    cam = exact_cam()
    for scale_out in (1000.0, 5000.0):
        o = V.register_depth_host(d, cam, 1000.0, cam, ROWS, COLS, scale_out)
        want = V.to_depth(scale_out, V.from_depth(1000.0, d))
        assert np.array_equal(o["depth"], want.reshape(d.shape))
        assert np.array_equal(o["depth"], (d.astype(np.uint32) * int(scale_out / 1000.0)).astype(np.uint16))
        s = np.arange(ROWS * COLS, dtype=np.uint32).reshape(ROWS, COLS)
        assert np.array_equal(o["src_index"], np.where(d != 0, s, V.SRC_NONE))
        n = int((d != 0).sum())
        assert tuple(o["counts"]) == (n, n, n, n)
        assert np.array_equal(o["zkey"] == V.ZKEY_EMPTY, d == 0)


def test_registration_integer_baseline():
    rows, cols = 24, 40
    cam = np.array([cols / 2 - 0.5, rows / 2 - 0.5, 100.0, 100.0, 0.0], np.float32)
    d = np.full((rows, cols), 5000, np.uint16)  # 1 m
    pose = np.array([0.05, 0, 0, 0, 0, 0, 1], np.float32)
    o = V.register_depth_host(d, cam, 5000.0, cam, rows, cols, 5000.0, pose7=pose)
    assert (o["depth"][:, 5:] == 5000).all() and (o["depth"][:, :5] == 0).all()
    s = np.arange(rows * cols, dtype=np.uint32).reshape(rows, cols)
    assert np.array_equal(o["src_index"][:, 5:], s[:, :-5]) and (o["src_index"][:, :5] == V.SRC_NONE).all()
    assert tuple(o["counts"]) == (rows * cols, rows * cols, rows * (cols - 5), rows * (cols - 5))


def test_registration_occlusion():
    rows, cols = 24, 40
    cam = np.array([cols / 2 - 0.5, rows / 2 - 0.5, 100.0, 100.0, 0.0], np.float32)
    d = np.full((rows, cols), 10000, np.uint16)  # a far plane at 2 m: shifts by 2.5 columns
    d[:, 10:16] = 5000  # a near strip at 1 m: shifts by 5 columns, onto far pixels
    pose = np.array([0.05, 0, 0, 0, 0, 0, 1], np.float32)
    o = V.register_depth_host(d, cam, 5000.0, cam, rows, cols, 5000.0, pose7=pose)
    assert (o["depth"][:, 15:21] == 5000).all(), "where both land the near surface is kept"
    src_cols = o["src_index"][:, 15:21] % cols
    assert ((src_cols >= 10) & (src_cols < 16)).all()
    assert int(o["counts"][3]) < int(o["counts"][2])  # covered < landed
    keys = o["zkey"][o["zkey"] != V.ZKEY_EMPTY]
    assert np.array_equal((keys & 0xFFFFFFFF).astype(np.uint32), o["src_index"][o["src_index"] != V.SRC_NONE])


def test_registration_tie_break_takes_the_lowest_source_index():
    rows, cols = 32, 48
    dcam = np.array([cols / 2 - 0.5, rows / 2 - 0.5, 64.0, 64.0, 0.0], np.float32)
    ccam = np.array([cols / 4 - 0.5, rows / 4 - 0.5, 32.0, 32.0, 0.0], np.float32)
    d = np.full((rows, cols), 7500, np.uint16)
    o = V.register_depth_host(d, dcam, 5000.0, ccam, rows // 2, cols // 2, 5000.0)
    assert tuple(o["counts"]) == (rows * cols, rows * cols, rows * cols, rows * cols // 4)
    assert (o["depth"] == 7500).all()
    # every colour pixel gets several source pixels at equal Z' bits: the lowest index of them must have won
    src = o["src_index"].astype(np.int64)
    sy, sx = src // cols, src % cols
    # restate the landing in float64 (u = 0.5 (x - cu_d) + cu_c is far from a rounding boundary at .25 / .75 offsets)
    y, x = np.mgrid[0:rows, 0:cols]
    lx = np.floor(0.5 * (x - dcam[0]) + ccam[0] + 0.5).astype(int)
    ly = np.floor(0.5 * (y - dcam[1]) + ccam[1] + 0.5).astype(int)
    want = np.full((rows // 2, cols // 2), rows * cols, np.int64)
    ok = (lx >= 0) & (lx < cols // 2) & (ly >= 0) & (ly < rows // 2)
    np.minimum.at(want, (ly[ok], lx[ok]), (y * cols + x)[ok])
    assert np.array_equal(src, want)
    assert (np.bincount((ly[ok] * (cols // 2) + lx[ok])) > 1).any(), "the case must have ties"
    assert sy.max() < rows and sx.max() < cols


def test_registration_holes_contribute_nothing():
    _, d = frame()
    d = np.minimum(d, 12000)
    d[10:20, 30:40] = 0
    cam = exact_cam()
    o = V.register_depth_host(d, cam, 1000.0, cam, ROWS, COLS, 1000.0)
    assert (o["depth"][d == 0] == 0).all() and (o["src_index"][d == 0] == V.SRC_NONE).all()
    assert int(o["counts"][0]) == int((d != 0).sum())
    o = V.register_depth_host(np.zeros_like(d), cam, 1000.0, cam, ROWS, COLS, 1000.0)
    assert not o["depth"].any() and (o["zkey"] == V.ZKEY_EMPTY).all() and tuple(o["counts"]) == (0, 0, 0, 0)


def test_registration_footprint_fills_an_upscaled_plane():
    rows, cols = 24, 32
    dcam = np.array([cols / 2 - 0.5, rows / 2 - 0.5, 32.0, 32.0, 0.0], np.float32)
    ccam = np.array([cols - 0.5, rows - 0.5, 64.0, 64.0, 0.0], np.float32)
    d = np.full((rows, cols), 6000, np.uint16)
    one = V.register_depth_host(d, dcam, 5000.0, ccam, 2 * rows, 2 * cols, 5000.0, footprint=1)
    two = V.register_depth_host(d, dcam, 5000.0, ccam, 2 * rows, 2 * cols, 5000.0, footprint=2)
    assert int(one["counts"][3]) == rows * cols and (one["depth"] == 0).sum() == 3 * rows * cols, "footprint 1 leaves holes"
    assert (two["depth"][1:, 1:] == 6000).all(), "footprint 2 fills them"
    assert int(two["counts"][3]) > int(one["counts"][3])


# ------------------------------------------------------------------------------------------------------------ refusals
def test_undistortion_refusals_write_nothing():
    g, d = frame()
    cam = exact_cam()
    nan, inf = float("nan"), float("inf")

    def bad(i, v):
        c = cam.copy()
        c[i] = v
        return c

    def call(gray=g, depth=d, cam_in=cam, dist=None, cam_out=cam, out_rows=ROWS, out_cols=COLS, border=0, want=("gray", "depth", "map", "counts")):
        outs = dict(gray=np.full((max(out_rows, 1), max(out_cols, 1)), 7, np.uint8), depth=np.full((max(out_rows, 1), max(out_cols, 1)), 7, np.uint16),
                    map=np.full((max(out_rows, 1), max(out_cols, 1), 2), 7, np.float32), counts=np.full(3, 7, np.uint32))
        k = [np.ascontiguousarray(c, np.float32) if c is not None else None for c in (cam_in, dist, cam_out)]
        ptr = [V._ptr(outs[name]) if name in want else None for name in ("gray", "depth", "map", "counts")]
        in_rows, in_cols = (gray if gray is not None else depth if depth is not None else g).shape
        st = V.lib().vors_undistort_frame_host(V._ptr(gray), V._ptr(depth), in_rows, in_cols, V._ptr(k[0]), V._ptr(k[1]), V._ptr(k[2]), out_rows,
                                               out_cols, border, *ptr)
        assert all((o == 7).all() for o in outs.values()), "a refused call writes nothing"
        return st

    refused = [dict(gray=None, depth=None), dict(gray=None, want=("gray", "map")), dict(depth=None, want=("depth",)), dict(want=()),
               dict(cam_in=None), dict(cam_out=None), dict(cam_in=bad(0, nan)), dict(cam_out=bad(4, inf)), dict(cam_in=bad(2, 0.0)),
               dict(cam_in=bad(3, 0.0)), dict(cam_out=bad(2, 0.0)), dict(cam_out=bad(3, 0.0)), dict(dist=[0, 0, nan, 0, 0]),
               dict(dist=[inf, 0, 0, 0, 0]), dict(border=-1), dict(border=2), dict(out_rows=0), dict(out_cols=0), dict(out_rows=65536),
               dict(out_cols=65536), dict(out_rows=32768, out_cols=16384)]
    for kw in refused:
        if kw.get("out_rows", 0) > 1000 or kw.get("out_cols", 0) > 1000:  # (no sentinel planes of that size: the pointers are not followed)
            k = V._ptr(cam)
            st = V.lib().vors_undistort_frame_host(V._ptr(g), V._ptr(d), ROWS, COLS, k, None, k, kw.get("out_rows", ROWS), kw.get("out_cols", COLS), 0,
                                                   V._ptr(g), None, None, None)
        else:
            st = call(**kw)
        assert st == INVALID, kw
    # the input sizes, and pointers off their natural alignment
    k = V._ptr(cam)
    out = np.full((ROWS, COLS), 7, np.uint16)
    for in_rows, in_cols in ((0, COLS), (ROWS, 0), (65536, 1), (1, 65536), (16385, 16384)):
        assert V.lib().vors_undistort_frame_host(V._ptr(g), V._ptr(d), in_rows, in_cols, k, None, k, ROWS, COLS, 0, None, V._ptr(out), None, None) == INVALID
    buf = np.zeros(2 * ROWS * COLS + 8, np.uint8)
    odd = buf.ctypes.data + 1
    assert V.lib().vors_undistort_frame_host(None, odd, ROWS, COLS, k, None, k, ROWS, COLS, 0, None, V._ptr(out), None, None) == INVALID
    assert V.lib().vors_undistort_frame_host(None, V._ptr(d), ROWS, COLS, k, None, k, ROWS, COLS, 0, None, odd, None, None) == INVALID
    assert V.lib().vors_undistort_frame_host(None, V._ptr(d), ROWS, COLS, k, None, k, ROWS, COLS, 0, None, None, odd + 1, None) == INVALID
    assert V.lib().vors_undistort_frame_host(None, V._ptr(d), ROWS, COLS, k, None, k, ROWS, COLS, 0, None, None, None, odd + 1) == INVALID
    assert (out == 7).all() and not buf.any()
    # the Python layer raises on each of them
    with pytest.raises(V.VorsError):
        V.undistort_frame_host(None, None, cam, None, cam, ROWS, COLS)
    with pytest.raises(V.VorsError):
        V.undistort_frame_host(g, d, cam, None, cam, ROWS, COLS, border=2)
    with pytest.raises(V.VorsError):
        V.undistort_frame_host(g, d, cam[:4], None, cam, ROWS, COLS)
    with pytest.raises(V.VorsError):
        V.undistort_frame_host(g, d[:-1], cam, None, cam, ROWS, COLS)
    with pytest.raises(V.VorsError):
        V.undistort_source_host(cam, None, bad(2, 0.0), pixels(2, 2))
    with pytest.raises(V.VorsError):
        V.undistort_source_host(cam, [0, 0, 0, 0, nan], cam, pixels(2, 2))


def test_registration_refusals_write_nothing():
    _, d = frame()
    cam = exact_cam()
    sent = dict(zkey=np.full((ROWS, COLS), 7, np.uint64), depth=np.full((ROWS, COLS), 7, np.uint16), src=np.full((ROWS, COLS), 7, np.uint32),
                counts=np.full(4, 7, np.uint32))
    k = V._ptr(cam)

    def call(depth=V._ptr(d), dcam=k, d_rows=ROWS, d_cols=COLS, scale_in=1000.0, ccam=k, c_rows=ROWS, c_cols=COLS, scale_out=1000.0, footprint=1,
             zkey=V._ptr(sent["zkey"]), depth_out=V._ptr(sent["depth"]), src=V._ptr(sent["src"]), counts=V._ptr(sent["counts"])):
        st = V.lib().vors_register_depth_host(depth, dcam, d_rows, d_cols, scale_in, None, ccam, c_rows, c_cols, scale_out, footprint, zkey, depth_out,
                                              src, counts)
        assert all((o == 7).all() for o in sent.values()), "a refused call writes nothing"
        return st

    odd = sent["zkey"].ctypes.data
    for kw in (dict(depth=None), dict(dcam=None), dict(ccam=None), dict(zkey=None), dict(zkey=odd + 4), dict(footprint=0), dict(footprint=4),
               dict(d_rows=0), dict(d_cols=0), dict(c_rows=0), dict(c_cols=0), dict(d_rows=65536), dict(c_cols=65536),
               dict(c_rows=32768, c_cols=16384), dict(scale_in=0.0), dict(scale_in=float("nan")), dict(scale_out=-1.0), dict(depth=d.ctypes.data + 1),
               dict(depth_out=odd + 1), dict(src=odd + 2), dict(counts=odd + 2)):
        assert call(**kw) == INVALID, kw
    with pytest.raises(V.VorsError):
        V.register_depth_host(d, cam, 1000.0, cam, ROWS, COLS, 1000.0, footprint=0)
    with pytest.raises(V.VorsError):
        V.register_depth_host(d, cam, 1000.0, cam[:3], ROWS, COLS, 1000.0)
    with pytest.raises(V.VorsError):
        V.register_depth_host(d, cam, 1000.0, cam, ROWS, COLS, 1000.0, pose7=np.zeros(6))


# ------------------------------------------------------------------------------------------------------------ sanitizers
def test_frontend_host_check_under_the_host_sanitizers():
    """`make frontend_host_check`: operators.cpp and csrc/frontend_host_check.cpp with ASan and UBSan on the host side, every plane a heap
    block of exactly its size. Runs without a GPU."""
    csrc = os.path.join(ROOT, "visual-odometry-rs_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "-s", "frontend_host_check"])
    r = subprocess.run([os.path.join(csrc, "frontend_host_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "frontend_host_check: ok" in r.stdout, r.stdout + r.stderr
