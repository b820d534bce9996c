"""Rendering of point lists and of the keyframe map into a camera (vors_render_points, vors_trackers_render_map, vors_tracker_render_map):
a keyed z-buffer splat and its resolve into a u16 depth map and a u8 grey image. GPU only.

  1. device == host entry, bytewise, on the hostile list of tests/test_render_points_host.py: 3 sequences of 0 / 300 / all points, with and
     without ranges and poses, footprints 1..3, all eight subsets of the nullable outputs
  2. the stride loop and the last partial workgroup (a list beyond the capped grid's 2^20 ranks), the narrow resolve (an odd plane)
  3. two runs are bitwise equal; a sequence does not depend on its company or on the stream; the pass only reads
  4. on a tracked run (the set-up of tests/test_gpu_trackers_map.py), voxel filter on and off: Trackers.render_map == the host entry on the
     downloaded map, at the current poses (read on the device) and at explicit ones; a keyframe rendered alone at its own pose puts every
     point on its own pixel
  5. Tracker.render_map == sequence 0 of an N = 1 handle
  6. the loop closes: the rendering is accepted as the keyframe of a fresh Batch and the real current frame tracks against it
  7. hostile scenes: no fault, the counter identities, guard bytes around the caller's planes intact, on aligned planes (the wide resolve)
     and on planes off that alignment (the narrow one), which give the same bytes
"""
import functools
import glob
import itertools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from test_render_points_host import COLS, POSE, ROWS, SCALE, cam, hostile_list, random_pose

EMPTY = np.uint64(V.ZKEY_EMPTY)
RANK = np.uint64(0xFFFFFFFF)
NAMES = ("zkey", "depth", "gray", "counts")


def to_host(out):
    """The tensors of a rendering as the host entry's dtypes."""
    import torch
    torch.cuda.synchronize()
    view = dict(zkey=np.uint64, depth=np.uint16, gray=np.uint8, counts=np.uint32)
    return {k: t.cpu().numpy().view(view[k]) for k, t in out.items()}


def host_render(xyz, gray, counts, k, rows, cols, scale, poses, ranges, f):
    """vors_render_points_host per sequence -> the four outputs stacked."""
    per = [V.render_points_host(xyz[s], gray[s], k, rows, cols, scale, pose7=None if poses is None else poses[s], footprint=f, count=int(counts[s]),
                                range2=None if ranges is None else ranges[s]) for s in range(len(xyz))]
    return {name: np.stack([p[name] for p in per]) for name in NAMES}


def assert_same(got, want, where, names=NAMES):
    for name in names:
        a, b = got[name], want[name]
        assert a.dtype == b.dtype and a.shape == b.shape, f"{where}: {name} {a.dtype} {a.shape} against {b.dtype} {b.shape}"
        assert a.tobytes() == b.tobytes(), f"{where}: {name} differs at {np.argwhere(a != b)[:5].tolist()}"


def check_identities(c, zkey, f, where):
    c = c.astype(np.int64)
    assert (c[:, 0] >= c[:, 1]).all() and (c[:, 1] >= c[:, 2]).all(), f"{where}: considered >= in_front >= landed fails: {c.tolist()}"
    assert (c[:, 3] <= c[:, 2] * f * f).all(), f"{where}: covered <= landed f^2 fails: {c.tolist()}"
    assert (c[:, 3] == (zkey != EMPTY).reshape(len(c), -1).sum(axis=1)).all(), f"{where}: covered differs from the non-empty keys"


def cuda(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dtype) if dtype is not None else a).cuda()


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("footprint", [1, 2, 3])
@pytest.mark.parametrize("with_pose", [False, True], ids=["no_pose", "pose"])
@pytest.mark.parametrize("with_ranges", [False, True], ids=["whole", "ranges"])
def test_device_equals_host(footprint, with_pose, with_ranges):
    xyz1, gray1 = hostile_list(with_pose)
    n, cap = 3, len(xyz1)
    xyz, gray = np.stack([xyz1] * n), np.stack([gray1, gray1[::-1].copy(), gray1])
    counts = np.array([0, 300, cap + 1000], np.uint32)   # less than one chunk, several chunks and not a multiple of the chunk, clipped
    assert cap % 1024 != 0 and cap > 4 * 1024
    poses = np.stack([POSE] * n) if with_pose else None
    ranges = np.array([[0, 5], [50, 200], [700, 2900]], np.uint32) if with_ranges else None
    k = cam(ROWS, COLS)
    want = host_render(xyz, gray, counts, k, ROWS, COLS, SCALE, poses, ranges, footprint)
    assert want["counts"][2, 2] > 0 and (want["counts"][0] == 0).all()
    args = (cuda(xyz), cuda(gray), cuda(counts, np.int32), k, ROWS, COLS, SCALE)
    kw = dict(poses=None if poses is None else cuda(poses), ranges=None if ranges is None else cuda(ranges, np.int32), footprint=footprint)
    # d_zkey is required at the C entry: the legal calls are the eight subsets of the nullable outputs
    nullable = ("depth", "gray", "counts")
    for r in range(len(nullable) + 1):
        for some in itertools.combinations(nullable, r):
            subset = ("zkey",) + some
            got = to_host(V.render_points(*args, **kw, **{name: name in subset for name in NAMES}))
            assert set(got) == set(subset)
            assert_same(got, want, f"outputs {subset}", subset)
    got = to_host(V.render_points(*args, **kw, zkey=False, depth=True, gray=True))   # (the mirror makes the key plane itself)
    assert set(got) == {"depth", "gray"}
    assert_same(got, want, "outputs without the key plane", ("depth", "gray"))
    check_identities(want["counts"], want["zkey"], footprint, "host entry")


# ------------------------------------------------------------------------------------------------------------ 2
@functools.lru_cache(maxsize=None)
def long_lists():
    """2 sequences beyond the capped grid's reach (1024 chunks of 1024 ranks): the stride loop, and a last partial workgroup."""
    rows, cols = 47, 63   # an odd plane: the resolve takes one pixel per access
    rng = np.random.default_rng(5)
    cap = (1 << 20) + 70_000
    k = cam(rows, cols)
    xy = np.stack([rng.uniform(-3, cols + 3, cap), rng.uniform(-3, rows + 3, cap)], 1).astype(np.float32)
    poses = np.stack([random_pose(rng), random_pose(rng)])
    xyz = np.stack([V.camera_back_project(k, poses[s], xy, rng.uniform(0.5, 6.0, cap).astype(np.float32)) for s in range(2)])
    gray = rng.integers(1, 256, (2, cap)).astype(np.uint8)
    counts = np.array([(1 << 20) + 1500, cap - 333], np.uint32)
    return rows, cols, k, xyz, gray, counts, poses


@pytest.mark.parametrize("footprint", [1, 3])
def test_stride_loop_and_partial_workgroup(footprint):
    rows, cols, k, xyz, gray, counts, poses = long_lists()
    ranges = np.array([[3, 1 << 31], [1 << 20, 1 << 20]], np.uint32) if footprint == 3 else None   # (the second: only the loop's second trip)
    want = host_render(xyz, gray, counts, k, rows, cols, SCALE, poses, ranges, footprint)
    got = to_host(V.render_points(cuda(xyz), cuda(gray), cuda(counts, np.int32), k, rows, cols, SCALE, poses=cuda(poses),
                                  ranges=None if ranges is None else cuda(ranges, np.int32), footprint=footprint, zkey=True, counts=True))
    assert_same(got, want, f"footprint {footprint}")
    assert (want["counts"][:, 0] == (counts if ranges is None else [counts[0] - 3, counts[1] - (1 << 20)])).all()
    # the winners come from beyond the grid's first pass too
    assert ((want["zkey"][want["zkey"] != EMPTY] & RANK) >= np.uint64(1 << 20)).any()


# ------------------------------------------------------------------------------------------------------------ 3
def test_reproducible_isolated_read_only():
    import torch
    xyz1, gray1 = hostile_list(True)
    rng = np.random.default_rng(9)
    n, cap = 4, len(xyz1)
    xyz = np.stack([xyz1[rng.permutation(cap)] for _ in range(n)])
    gray = rng.integers(1, 256, (n, cap)).astype(np.uint8)
    counts = np.array([cap, 17, 2000, cap - 5], np.uint32)
    ranges = np.array([[10, cap], [0, 17], [500, 900], [0, 1 << 30]], np.uint32)
    poses = np.stack([POSE] * n)
    k = cam(ROWS, COLS)
    dev = [cuda(xyz), cuda(gray), cuda(counts, np.int32), cuda(poses), cuda(ranges, np.int32)]
    before = [t.clone() for t in dev]

    def render(sel=slice(None), f=2):
        return to_host(V.render_points(dev[0][sel].contiguous(), dev[1][sel].contiguous(), dev[2][sel].contiguous(), k, ROWS, COLS, SCALE,
                                       poses=dev[3][sel].contiguous(), ranges=dev[4][sel].contiguous(), footprint=f, zkey=True, counts=True))

    first, second = render(), render()
    assert_same(second, first, "second run")
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(dev, before)), "the pass wrote one of its inputs"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for s, stream in ((0, None), (n - 1, side)):
        if stream is None:
            alone = render(slice(s, s + 1))
        else:
            with torch.cuda.stream(stream):
                alone = render(slice(s, s + 1))
        assert_same(alone, {name: first[name][s:s + 1] for name in NAMES}, f"sequence {s} alone")


# ------------------------------------------------------------------------------------------------------------ 4
N_SEQ, N_FRAMES = 6, 10
BASE = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001])
SPEED = np.array([4.0, 0.05, 9.0, 2.0, 6.0, 5.0])
SHAPES = {V.CANDIDATES_DENSE: (120, 160, 4), V.CANDIDATES_COARSE_TO_FINE: (96, 128, 4)}
MODES = pytest.mark.parametrize("mode", [V.CANDIDATES_DENSE, V.CANDIDATES_COARSE_TO_FINE], ids=["dense", "coarse_to_fine"])
VOXELS = pytest.mark.parametrize("voxels", [False, True], ids=["unfiltered", "voxels"])
VOXEL_M = {V.CANDIDATES_DENSE: 0.02, V.CANDIDATES_COARSE_TO_FINE: 0.10}
MAX_KF = 16


def config(mode, arith=V.ARITH_FUSED):
    rows, cols, L = SHAPES[mode]
    intr = V.scaled_intrinsics(rows, cols)
    return V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, arithmetic=arith)


@functools.lru_cache(maxsize=None)
def frames_of(mode):
    import torch
    rows, cols, _ = SHAPES[mode]
    intr = V.scaled_intrinsics(rows, cols)
    out = [V.synth_render_frames([1000 + s for s in range(N_SEQ)], [k] * N_SEQ, [BASE * SPEED[s] * k for s in range(N_SEQ)], rows, cols, intr,
                                 invalid_percent=2) for k in range(N_FRAMES)]
    torch.cuda.synchronize()
    return out


def snapshot(tr):
    """Everything the pass may not write: the map, poses, statuses, keyframes, stats."""
    import torch
    m = tr.map()
    torch.cuda.synchronize()
    poses, status, kf = tr.current_frames()
    out = {k: v.cpu().numpy() for k, v in m.items()}
    out.update(poses=poses, status=status, kf=kf, stats=tr.stats().copy())
    return out


@functools.lru_cache(maxsize=None)
def tracked(mode, voxels, seqs=None):
    """A mapped run over all frames -> (the handle, its state on the host)."""
    rows, cols, _ = SHAPES[mode]
    n = N_SEQ if seqs is None else len(seqs)
    tr = V.Trackers(config(mode), n, rows, cols)
    tr.enable_map(0, rows * cols * N_FRAMES, MAX_KF)
    if voxels:
        tr.enable_map_voxels(VOXEL_M[mode], 1 << 18)
    for k, (g, d) in enumerate(frames_of(mode)):
        if seqs is not None:
            g, d = g[list(seqs)].contiguous(), d[list(seqs)].contiguous()
        (tr.init if k == 0 else tr.track)(g, d)
    return tr, snapshot(tr)


def host_render_map(mode, st, poses, ranges, f):
    rows, cols, _ = SHAPES[mode]
    return host_render(st["xyz"], st["gray"], st["counts"].view(np.uint32), cam(rows, cols), rows, cols, V.DEPTH_SCALE, poses, ranges, f)


@MODES
@VOXELS
def test_tracked_map_equals_host_entry(mode, voxels):
    tr, st = tracked(mode, voxels)
    assert (st["counts"] > 0).all() and (st["n_segments"] >= 1).all() and st["n_segments"].max() >= 3
    # the current frame poses, read on the device
    for f in (1, 2, 3):
        got = to_host(tr.render_map(footprint=f, zkey=True, counts=True))
        assert_same(got, host_render_map(mode, st, st["poses"], None, f), f"current poses, footprint {f}")
        check_identities(got["counts"], got["zkey"], f, f"footprint {f}")
        assert (got["counts"][:, 2] > 0).all()
    # explicit poses
    rng = np.random.default_rng(2)
    poses = np.stack([random_pose(rng, angle=0.05, shift=0.05) for _ in range(N_SEQ)])
    got = to_host(tr.render_map(poses=cuda(poses), footprint=2, zkey=True, counts=True))
    assert_same(got, host_render_map(mode, st, poses, None, 2), "explicit poses")
    # the pass only reads
    after = snapshot(tr)
    for name in st:
        assert st[name].tobytes() == after[name].tobytes(), f"the rendering changed {name}"


@MODES
@VOXELS
def test_a_keyframe_alone_at_its_own_pose_returns_to_its_pixels(mode, voxels):
    tr, st = tracked(mode, voxels)
    seg = V.decode_map_segments(st["segments"])
    m = tr.map(copy=False)
    checked = 0
    for kf in (0, 1, 2):
        have = np.nonzero(st["n_segments"] > kf)[0]
        if len(have) == 0:
            continue
        poses = np.ascontiguousarray(seg[:, kf]["pose7"])
        poses[st["n_segments"] <= kf] = [0, 0, 0, 0, 0, 0, 1]   # (records never written: any pose, the range is clipped whatever it holds)
        got = to_host(tr.render_map(poses=cuda(poses), ranges=(m["segments"], 40 * kf + 4, 40 * MAX_KF), footprint=1, zkey=True, counts=True))
        ranges = np.stack([seg[:, kf]["first"], seg[:, kf]["count"]], 1).astype(np.uint32)
        assert_same(got, host_render_map(mode, st, poses, ranges, 1), f"keyframe {kf}")
        for s in have:
            first, count = int(seg[s, kf]["first"]), int(seg[s, kf]["count"])
            pix = st["pixel"][s, first:first + count].view(np.uint32)
            x, y = (pix & 0xFFFF).astype(np.int64), (pix >> 16).astype(np.int64)
            winner = (got["zkey"][s, y, x] & RANK).astype(np.int64)
            stray = int((winner != first + np.arange(count)).sum())
            assert stray == 0, f"keyframe {kf} of sequence {s}: {stray} of {count} points did not return to their own pixel"
            assert got["counts"][s].tolist() == [count] * 4
            checked += count
    assert checked > 0


# ------------------------------------------------------------------------------------------------------------ 5
@MODES
def test_single_tracker_equals_one_sequence_handle(mode):
    s = 4
    _, st = tracked(mode, False, seqs=(s,))
    rows, cols, _ = SHAPES[mode]
    host = [(g[s].cpu().numpy(), d[s].cpu().numpy().view(np.uint16)) for g, d in frames_of(mode)]
    one = V.Tracker(config(mode), 0.0, host[0][1], 0.0, host[0][0], map=(0, rows * cols * N_FRAMES, MAX_KF))
    for k in range(1, N_FRAMES):
        one.track(float(k), host[k][1], float(k), host[k][0])
    pose = random_pose(np.random.default_rng(4), angle=0.05, shift=0.05)
    for pose7, rng2, f in ((None, None, 1), (pose, None, 3), (None, (100, 5000), 2)):
        got = one.render_map(0, pose7=pose7, range2=rng2, footprint=f)
        want = host_render_map(mode, st, st["poses"] if pose7 is None else pose7[None], None if rng2 is None else np.array([rng2], np.uint32), f)
        assert_same({k: v[None] for k, v in got.items()}, want, f"pose {pose7 is not None}, range {rng2}, footprint {f}")
    with pytest.raises(V.VorsError, match="footprint"):
        one.render_map(0, footprint=0)
    with pytest.raises(V.VorsError, match="level"):
        one.render_map(7)


# ------------------------------------------------------------------------------------------------------------ 6
def test_the_loop_closes():
    import torch
    mode = V.CANDIDATES_DENSE
    rows, cols, _ = SHAPES[mode]
    tr, st = tracked(mode, False)
    out = tr.render_map(footprint=2)   # the model at the current pose: the arguments of prepare_keyframes
    cur_gray = frames_of(mode)[-1][0]
    b = V.Batch(config(mode), N_SEQ, rows, cols)
    poses = torch.zeros((N_SEQ, 7), dtype=torch.float32, device="cuda")
    status = torch.full((N_SEQ,), -1, dtype=torch.int32, device="cuda")
    b.prepare_keyframes(out["gray"], out["depth"])
    b.track_current(cur_gray, poses, status)
    torch.cuda.synchronize()
    poses, status = poses.cpu().numpy(), status.cpu().numpy()
    covered = (out["depth"] != 0).float().mean().item()
    print(f"frame to model: covered {covered:.3f}, |t| {np.linalg.norm(poses[:, :3], axis=1).round(5).tolist()}, "
          f"|q_xyz| {np.linalg.norm(poses[:, 3:6], axis=1).round(5).tolist()}")
    assert (status == V.TRACK_OK).all(), f"statuses {status.tolist()}"
    assert np.isfinite(poses).all()


# ------------------------------------------------------------------------------------------------------------ 7
GUARD = 64


def guarded(n_elements, dtype, fill, shift=0):
    """(the whole buffer, the plane inside it, `shift` elements off the buffer's alignment)."""
    import torch
    flat = torch.full((n_elements + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return flat, flat[GUARD + shift:GUARD + shift + n_elements]


def guards_intact(flat, view):
    a = (view.data_ptr() - flat.data_ptr()) // flat.element_size()
    return bool((flat[:a] == 0x55).all() and (flat[a + view.numel():] == 0x55).all())


@pytest.mark.parametrize("name", sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "adversarial", "*.npz"))))
def test_hostile_scenes(name):
    import torch
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "adversarial", name + ".npz"))
    L, mode, rows, cols, intr = int(g["L"]), int(g["mode"]), int(g["rows"]), int(g["cols"]), tuple(float(x) for x in g["intr"])
    kg, cg = (torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("kf_gray", "cur_gray"))
    kd = torch.from_numpy(np.ascontiguousarray(g["kf_depth"]).view(np.int16)).cuda()   # (stands in for the current depth as well)
    n = kg.shape[0]
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, huber_delta=float(g["huber"]),
                   arithmetic=V.ARITH_FUSED)
    tr = V.Trackers(cfg, n, rows, cols)   # every pair of the scene is one two-frame sequence
    tr.enable_map(0, 2 * rows * cols, 4)
    tr.init(kg, kd)
    tr.track(cg, kd)
    plane = n * rows * cols
    assert (rows * cols) % 4 == 0
    for f in (1, 3):
        aligned = None
        # shift 0: every plane allows the resolve's four pixels per thread; shift 1: keys 8 bytes, depth 2 bytes and grey 1 byte off that
        # alignment, so the resolve takes one pixel per access on planes whose size alone would allow four
        for shift in (0, 1):
            bufs = [guarded(plane, torch.int64, 0x55, shift), guarded(plane, torch.int16, 0x55, shift), guarded(plane, torch.uint8, 0x55, shift),
                    guarded(n * V.RENDER_COUNTS, torch.int32, 0x55)]
            assert shift == 0 or (bufs[0][1].data_ptr() % 16 == 8 and bufs[1][1].data_ptr() % 8 == 2 and bufs[2][1].data_ptr() % 4 == 1)
            views = [bufs[0][1].view(n, rows, cols), bufs[1][1].view(n, rows, cols), bufs[2][1].view(n, rows, cols), bufs[3][1].view(n, V.RENDER_COUNTS)]
            got = to_host(tr.render_map(footprint=f, zkey=views[0], depth=views[1], gray=views[2], counts=views[3]))
            for flat, view in bufs:
                assert guards_intact(flat, view), f"footprint {f}, shift {shift}: a store left its plane"
            check_identities(got["counts"], got["zkey"], f, f"footprint {f}")
            assert ((got["depth"] != 0) <= (got["zkey"] != EMPTY)).all() and (got["gray"][got["zkey"] == EMPTY] == 0).all()
            if aligned is None:
                aligned = got
            else:
                assert_same(got, aligned, f"footprint {f}: the narrow resolve against the wide one")
    poses, status, _ = tr.current_frames()
    assert len(status) == n
