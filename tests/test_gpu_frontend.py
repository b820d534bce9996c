"""The sensor front end on the device (vors_undistort_frames, vors_register_depth) against the host entries
(vors_undistort_frame_host, vors_register_depth_host), which run the same texts (lie.h): equality of BITS of every output. GPU only.

Undistortion shapes: 3 planes of 37x53 -> 31x47 — odd sizes, so a thread's four pixels are a workgroup width apart and the last workgroup
has a tail — and 2 of 48x64 -> 48x64, where a thread takes four adjacent pixels (out_cols % 4 == 0, aligned planes). Registration shapes:
3 planes of 29x37 -> 45x61 with footprints 1 and 2, and 2 of 48x64 -> 48x64. The depth is a tilted plane with a depth step, a blob of
zeros and 2 % zeros; the grey is noise on a gradient. Every device output lies inside a sentinel-filled buffer with guard bands.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V

SCALE = 5000.0
U_SHAPES = {"odd": (3, 37, 53, 31, 47), "wide": (2, 48, 64, 48, 64)}  # n, in_rows, in_cols, out_rows, out_cols
R_SHAPES = {"odd": (3, 29, 37, 45, 61), "wide": (2, 48, 64, 48, 64)}  # n, d_rows, d_cols, c_rows, c_cols
DIST = np.array([0.2, -0.3, 0.01, -0.02, 0.1], np.float32)
GUARD = 64  # elements of sentinel on either side of a device output
OUTS = ("gray", "depth", "map", "counts")


def cam_of(rows, cols):
    return np.array([0.5 * cols - 0.5, 0.5 * rows - 0.5, 0.9 * cols, -0.95 * cols, 0.3], np.float32)  # fv < 0 and a skew


def out_cam(shape):
    n, in_rows, in_cols, out_rows, out_cols = U_SHAPES[shape]
    k = cam_of(in_rows, in_cols)
    k[0] -= 0.5 * (in_cols - out_cols) - 0.25  # the centred crop, a quarter pixel off
    k[1] -= 0.5 * (in_rows - out_rows)
    k[2:4] *= 0.8  # ... seen through a wider lens: the borders of the output look beyond the input plane
    return k


@functools.lru_cache(maxsize=None)
def planes(n, rows, cols):
    """depth [n, rows, cols] u16: a tilted plane per map, the right third 0.4 m further away, a blob of zeros, 2 % zeros; grey u8."""
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
    g = np.clip(2.0 * x + 1.5 * y + rng.normal(0, 30, (n, rows, cols)), 0, 255).astype(np.uint8)
    return g, d


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """A device tensor of `shape` inside a sentinel-filled flat buffer, `skew` elements off the buffer's own alignment."""

    def __init__(self, shape, dtype, sentinel, skew=0):
        import torch
        self.size = int(np.prod(shape))
        self.flat = torch.full((2 * GUARD + self.size + skew,), sentinel, dtype=dtype, device="cuda")
        self.lo = GUARD + skew
        self.t = self.flat[self.lo:self.lo + self.size].view(*shape)
        self.sentinel = sentinel

    def guards_intact(self):
        return bool((self.flat[:self.lo] == self.sentinel).all()) and bool((self.flat[self.lo + self.size:] == self.sentinel).all())

    def untouched(self):
        return bool((self.flat == self.sentinel).all())


# ------------------------------------------------------------------------------------------------------------ undistortion
@functools.lru_cache(maxsize=None)
def host_undistort(shape, distorted, border):
    n, in_rows, in_cols, out_rows, out_cols = U_SHAPES[shape]
    g, d = planes(n, in_rows, in_cols)
    outs = [V.undistort_frame_host(g[i], d[i], cam_of(in_rows, in_cols), DIST if distorted else None, out_cam(shape), out_rows, out_cols, border=border)
            for i in range(n)]
    for o in outs:
        assert 0 < int(o["counts"][2]) < int(o["counts"][0]), o["counts"]  # (a depth pixel may land where the grey sample is just outside)
        assert 2 * int(o["counts"][1]) > int(o["counts"][0]) > int(o["counts"][1]), "some pixels, and fewer than half, must look outside"
    return dict(gray=np.stack([o["gray"] for o in outs]), depth=np.stack([o["depth"] for o in outs]), map=outs[0]["map"],
                counts=np.stack([o["counts"] for o in outs]))


def undistort_outputs(shape, skew=0):
    import torch
    n, _, _, out_rows, out_cols = U_SHAPES[shape]
    return dict(gray=Guarded((n, out_rows, out_cols), torch.uint8, 0xA5, 2 * skew), depth=Guarded((n, out_rows, out_cols), torch.int16, 0x5A5A, skew),
                map=Guarded((out_rows, out_cols, 2), torch.float32, -7.0), counts=Guarded((n, V.UNDISTORT_COUNTS), torch.int32, 0x5A5A5A5A))


def run_undistort(shape, distorted, border, want=OUTS, skew=0, inputs=("gray", "depth")):
    import torch
    n, in_rows, in_cols, out_rows, out_cols = U_SHAPES[shape]
    g, d = planes(n, in_rows, in_cols)
    outs = undistort_outputs(shape, skew)
    kw = {name: (outs[name].t if name in want else False) for name in OUTS}
    res = V.undistort_frames(dev(g) if "gray" in inputs else None, dev(d.view(np.int16)) if "depth" in inputs else None, cam_of(in_rows, in_cols),
                             DIST if distorted else None, out_cam(shape), out_rows, out_cols, border=border, gray_out=kw["gray"],
                             depth_out=kw["depth"], map=kw["map"], counts=kw["counts"])
    torch.cuda.synchronize()
    assert set(res) == set(want)
    return outs


def check_undistort(outs, ref, want):
    for name in OUTS:
        if name not in want:
            assert outs[name].untouched(), f"{name} was not asked for"
            continue
        got = outs[name].t.cpu().numpy()
        exp = ref[name]
        assert np.array_equal(got.view(exp.dtype).view(np.uint8), np.ascontiguousarray(exp).view(np.uint8)), name
        assert outs[name].guards_intact(), f"{name}: something was written beyond the planes"


@pytest.mark.parametrize("shape", list(U_SHAPES))
@pytest.mark.parametrize("distorted", [False, True], ids=["pinhole", "distorted"])
@pytest.mark.parametrize("border", [0, 1], ids=["zero", "replicate"])
def test_undistortion_equals_the_host_bit_for_bit(shape, distorted, border):
    ref = host_undistort(shape, distorted, border)
    check_undistort(run_undistort(shape, distorted, border), ref, OUTS)
    # each output alone (the others NULL)
    for name in OUTS:
        check_undistort(run_undistort(shape, distorted, border, want=(name,)), ref, (name,))


@pytest.mark.parametrize("shape", list(U_SHAPES))
def test_undistortion_of_one_kind_of_plane(shape):
    """Grey without a depth plane and depth without a grey plane: the counts of the missing plane are 0, the rest the same bits."""
    ref = dict(host_undistort(shape, True, 0))
    outs = run_undistort(shape, True, 0, want=("gray", "counts"), inputs=("gray",))
    ref_g = dict(ref, counts=ref["counts"] * np.array([1, 1, 0], np.uint32))
    check_undistort(outs, ref_g, ("gray", "counts"))
    check_undistort(run_undistort(shape, True, 0, want=("depth", "map", "counts"), inputs=("depth",)), ref, ("depth", "map", "counts"))


@pytest.mark.parametrize("border", [0, 1], ids=["zero", "replicate"])
def test_undistortion_misaligned_planes_take_the_scattered_path(border):
    """48x64 output planes that start 2 bytes off the alignment the four-adjacent path needs: same bits."""
    outs = run_undistort("wide", True, border, skew=1)
    assert outs["gray"].t.data_ptr() % 4 == 2 and outs["depth"].t.data_ptr() % 8 == 2
    check_undistort(outs, host_undistort("wide", True, border), OUTS)


def test_undistortion_refusals_enqueue_nothing():
    import torch
    shape = "odd"
    n, in_rows, in_cols, out_rows, out_cols = U_SHAPES[shape]
    g, d = planes(n, in_rows, in_cols)
    tg, td = dev(g), dev(d.view(np.int16))
    cam, out = cam_of(in_rows, in_cols), out_cam(shape)
    outs = undistort_outputs(shape)
    all_out = dict(gray_out=outs["gray"].t, depth_out=outs["depth"].t, map=outs["map"].t, counts=outs["counts"].t)

    def bad(i, v):
        c = cam.copy()
        c[i] = v
        return c

    nan = float("nan")
    cases = [dict(gray=None, depth=None), dict(gray=None, depth_out=False, map=False, counts=False), dict(depth=None, gray_out=False),
             dict(gray_out=False, depth_out=False, map=False, counts=False), dict(cam_in5=bad(2, 0.0)), dict(cam_in5=bad(3, 0.0)),
             dict(cam_out5=bad(2, 0.0)), dict(cam_out5=bad(0, nan)), dict(cam_in5=bad(4, float("inf"))), dict(dist5=[0, nan, 0, 0, 0]),
             dict(border=2), dict(border=-1)]
    for kw in cases:
        args = dict(gray=tg, depth=td, cam_in5=cam, dist5=DIST, cam_out5=out, out_rows=out_rows, out_cols=out_cols, border=0, **all_out)
        args.update(kw)
        with pytest.raises(V.VorsError):
            V.undistort_frames(**args)
    # sizes and alignment, at the C entry (the Python layer shapes its buffers from the sizes)
    k_in, k_out = V._ptr(cam), V._ptr(out)
    p = {name: o.t.data_ptr() for name, o in outs.items()}
    lib = V.lib()
    for sizes in ((0, in_cols, out_rows, out_cols), (in_rows, 0, out_rows, out_cols), (in_rows, in_cols, 0, out_cols), (in_rows, in_cols, out_rows, 0),
                  (65536, in_cols, out_rows, out_cols), (in_rows, in_cols, out_rows, 65536), (in_rows, in_cols, 32768, 16384)):
        assert lib.vors_undistort_frames(n, tg.data_ptr(), td.data_ptr(), sizes[0], sizes[1], k_in, None, k_out, sizes[2], sizes[3], 0, p["gray"],
                                         p["depth"], p["map"], p["counts"], None) == -1
    assert lib.vors_undistort_frames(0, tg.data_ptr(), td.data_ptr(), in_rows, in_cols, k_in, None, k_out, out_rows, out_cols, 0, p["gray"], p["depth"],
                                     p["map"], p["counts"], None) == -1
    for off in (dict(depth=1), dict(map=2), dict(counts=2)):
        q = {name: p[name] + off.get(name, 0) for name in p}
        assert lib.vors_undistort_frames(n, tg.data_ptr(), td.data_ptr(), in_rows, in_cols, k_in, None, k_out, out_rows, out_cols, 0, q["gray"],
                                         q["depth"], q["map"], q["counts"], None) == -1
    assert lib.vors_undistort_frames(n, None, td.data_ptr() + 1, in_rows, in_cols, k_in, None, k_out, out_rows, out_cols, 0, None, p["depth"], None,
                                     None, None) == -1
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs.values()), "a refused call writes nothing"


# ------------------------------------------------------------------------------------------------------------ registration
R_OUTS = ("zkey", "depth", "src_index", "counts")
POSE = np.array([0.04, -0.01, 0.02, 0.01, -0.02, 0.015, 0.0], np.float32)
POSE[6] = np.sqrt(1.0 - float((POSE[3:6].astype(np.float64) ** 2).sum()))


def color_cam(shape):
    n, d_rows, d_cols, c_rows, c_cols = R_SHAPES[shape]
    k = cam_of(c_rows, c_cols)
    k[2:4] *= 0.9  # a slightly wider colour camera: the depth plane does not cover all of it
    return k


@functools.lru_cache(maxsize=None)
def host_register(shape, footprint, posed):
    n, d_rows, d_cols, c_rows, c_cols = R_SHAPES[shape]
    _, d = planes(n, d_rows, d_cols)
    outs = [V.register_depth_host(d[i], cam_of(d_rows, d_cols), SCALE, color_cam(shape), c_rows, c_cols, 1000.0, pose7=POSE if posed else None,
                                  footprint=footprint) for i in range(n)]
    for o in outs:
        c = [int(v) for v in o["counts"]]
        assert 0 < c[3] < c_rows * c_cols and 0 < c[2] <= c[1] <= c[0], c
    return dict(zkey=np.stack([o["zkey"] for o in outs]), depth=np.stack([o["depth"] for o in outs]),
                src_index=np.stack([o["src_index"] for o in outs]), counts=np.stack([o["counts"] for o in outs]))


def run_register(shape, footprint, posed, want=R_OUTS):
    import torch
    n, d_rows, d_cols, c_rows, c_cols = R_SHAPES[shape]
    _, d = planes(n, d_rows, d_cols)
    plane = (n, c_rows, c_cols)
    outs = dict(zkey=Guarded(plane, torch.int64, 0x5A5A5A5A5A5A5A5A), depth=Guarded(plane, torch.int16, 0x5A5A), src_index=Guarded(plane, torch.int32, 0x5A5A5A5A),
                counts=Guarded((n, V.REGISTER_COUNTS), torch.int32, 0x5A5A5A5A))
    kw = {name: (outs[name].t if name in want else False) for name in R_OUTS}
    res = V.register_depth(dev(d.view(np.int16)), cam_of(d_rows, d_cols), SCALE, color_cam(shape), c_rows, c_cols, 1000.0, pose7=POSE if posed else None,
                           footprint=footprint, depth_out=kw["depth"], src_index=kw["src_index"], counts=kw["counts"], zkey=kw["zkey"])
    torch.cuda.synchronize()
    assert set(res) == set(want)
    return outs


def check_register(outs, ref, want):
    for name in R_OUTS:
        if name not in want:
            assert outs[name].untouched(), f"{name} was not asked for"
            continue
        got = outs[name].t.cpu().numpy()
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(ref[name]).view(np.uint8)), name
        assert outs[name].guards_intact(), f"{name}: something was written beyond the planes"


@pytest.mark.parametrize("shape,footprint", [("odd", 1), ("odd", 2), ("wide", 1), ("wide", 3)])
@pytest.mark.parametrize("posed", [False, True], ids=["no_pose", "posed"])
def test_registration_equals_the_host_bit_for_bit(shape, footprint, posed):
    ref = host_register(shape, footprint, posed)
    check_register(run_register(shape, footprint, posed), ref, R_OUTS)
    # the splat alone (the key plane only), and each resolved output alone beside it
    check_register(run_register(shape, footprint, posed, want=("zkey",)), ref, ("zkey",))
    for name in ("depth", "src_index", "counts"):
        check_register(run_register(shape, footprint, posed, want=("zkey", name)), ref, ("zkey", name))


def test_registration_refusals_enqueue_nothing():
    import torch
    n, d_rows, d_cols, c_rows, c_cols = R_SHAPES["odd"]
    _, d = planes(n, d_rows, d_cols)
    td = dev(d.view(np.int16))
    plane = (n, c_rows, c_cols)
    outs = dict(zkey=Guarded(plane, torch.int64, 0x5A5A5A5A5A5A5A5A), depth=Guarded(plane, torch.int16, 0x5A5A), src_index=Guarded(plane, torch.int32, 0x5A5A5A5A),
                counts=Guarded((n, V.REGISTER_COUNTS), torch.int32, 0x5A5A5A5A))
    dcam, ccam = cam_of(d_rows, d_cols), color_cam("odd")
    for kw in (dict(footprint=0), dict(footprint=4), dict(depth_scale_in=0.0), dict(depth_scale_out=float("nan")), dict(depth_scale_in=-1.0)):
        args = dict(depth_scale_in=SCALE, depth_scale_out=1000.0, footprint=1)
        args.update(kw)
        with pytest.raises(V.VorsError):
            V.register_depth(td, dcam, args["depth_scale_in"], ccam, c_rows, c_cols, args["depth_scale_out"], footprint=args["footprint"],
                             depth_out=outs["depth"].t, src_index=outs["src_index"].t, counts=outs["counts"].t, zkey=outs["zkey"].t)
    lib = V.lib()
    p = {name: o.t.data_ptr() for name, o in outs.items()}
    kd, kc = V._ptr(dcam), V._ptr(ccam)

    def call(n_=n, depth=td.data_ptr(), dc=kd, cc=kc, sizes=(d_rows, d_cols, c_rows, c_cols), zkey=p["zkey"], depth_out=p["depth"], src=p["src_index"],
             counts=p["counts"]):
        return lib.vors_register_depth(n_, depth, dc, sizes[0], sizes[1], SCALE, None, cc, sizes[2], sizes[3], 1000.0, 1, zkey, depth_out, src, counts, None)

    for kw in (dict(n_=0), dict(depth=None), dict(dc=None), dict(cc=None), dict(zkey=None), dict(zkey=p["zkey"] + 4), dict(sizes=(0, d_cols, c_rows, c_cols)),
               dict(sizes=(d_rows, d_cols, c_rows, 0)), dict(sizes=(65536, d_cols, c_rows, c_cols)), dict(sizes=(d_rows, d_cols, 32768, 16384)),
               dict(depth=td.data_ptr() + 1), dict(depth_out=p["depth"] + 1), dict(src=p["src_index"] + 2), dict(counts=p["counts"] + 2)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs.values()), "a refused call writes nothing"


# ------------------------------------------------------------------------------------------------------------ composition
def test_undistorted_planes_track_like_the_raw_planes():
    """The planes of an identity-distortion call (the camera has power-of-two focals: every step of the source coordinate is exact), fed
    to the sequence trackers at 96x128, give the poses of the raw planes bit for bit."""
    import torch
    rows, cols, n_seq, n_frames = 96, 128, 3, 4
    cam = np.array([cols / 2 - 0.5, rows / 2 - 0.5, 128.0, 128.0, 0.0], np.float32)
    step = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001])
    frames = [V.synth_render_frames([500 + q for q in range(n_seq)], [k] * n_seq, [step * k * (1 + q) for q in range(n_seq)], rows, cols, cam)
              for k in range(n_frames)]
    cfg = V.Config(nb_levels=4, intrinsics=V.Intrinsics(cam[:2], cam[2:4], cam[4]), arithmetic=V.ARITH_FUSED)
    results = []
    for undistort in (False, True):
        tr = V.Trackers(cfg, n_seq, rows, cols)
        for k, (g, d) in enumerate(frames):
            if undistort:
                o = V.undistort_frames(g, d, cam, np.zeros(5, np.float32), cam, rows, cols)
                assert torch.equal(o["gray"], g) and torch.equal(o["depth"], d)
                g, d = o["gray"], o["depth"]
            (tr.init if k == 0 else tr.track)(g, d)
        poses, status, _ = tr.current_frames()
        results.append((np.array(poses, np.float32), np.array(status)))
    (p0, s0), (p1, s1) = results
    assert np.array_equal(p0.view(np.uint32), p1.view(np.uint32)) and np.array_equal(s0, s1)
    assert np.abs(p0[:, :3]).max() > 1e-3, "the sequences must have moved"
