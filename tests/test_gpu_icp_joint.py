"""The joint point-to-plane and photometric ICP on the device (vors_icp_points_joint, Trackers.icp_map_joint) against its host twin
(vors_icp_points_joint_host), bit for bit. GPU only.

The layout of tests/test_gpu_icp_robust.py with tests/test_icp_joint_host.py's texture as the grey of model and frames: n = 3 lists of
capacity 2500 in one call: list 0 of count 1 against a plane of zeros (frozen as TOO_FEW in the first round), list 1 of count 1025 against
the "step" frame, list 2 of count 2500 against the "both" frame through the range (7, 2400). Start poses 32 bytes apart. The frames' grey
is the texture, list 2's with a patch of foreign grey (so that the photo Huber's linear branch is taken).

  1. poses, stats, sums29, both residual arrays, gate counts and photo counts equal the host's for normals on / off x Huber on / off x
     photo Huber on / off, iters 0 and 6
  2. photo_scale_m = 0 (grey pointers NULL) equals the device's vors_icp_points_robust
  3. output poses aliasing the input: the same bits
  4. Trackers.icp_map_joint equals icp_points_joint on the handle's own pointers, and refuses without the map or its normals
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from test_icp_joint_host import PHOTO_HUBER_GREY, PHOTO_SCALE_M, texture
from test_icp_robust_host import CAM, DIST_M, HUBER_M, MIN_COS, P_TRUE, SCALE, frame_normals_of, patched, pose_from_xi, to_depth, corner_z

CAP, N = 2500, 3
COUNTS = (1, 1025, 2500)
RANGES = np.array([[0, 1], [0, 4000], [7, 2400]], np.int32)  # (list 0 and 1: the whole list)
START_XI = ([0.001, 0, 0, 0, 0, 0], [0.004, -0.003, 0.005, 0.004, -0.005, 0.003], [-0.003, 0.004, 0.002, -0.003, 0.004, 0.005])
STEP_EPS = 2e-5
SENTINEL = 42.0
COMBOS = {f"{'n' if nrm else '-'}{'h' if hub else '-'}{'p' if ph else '-'}": (nrm, hub, ph)
          for nrm in (False, True) for hub in (0.0, HUBER_M) for ph in (0.0, PHOTO_HUBER_GREY)}
KEYS = ("poses", "stats", "sums29", "residuals", "gate_counts", "photo_residuals", "photo_counts")


@functools.lru_cache(maxsize=None)
def scene():
    """-> host arrays: xyz / normals [N, CAP, 3], list grey [N, CAP], depth [N, rows, cols] u16, frame grey [N, rows, cols], frame normals
    [N, rows, cols, 3], start poses [N, 8]."""
    clean, tex = to_depth(corner_z()), texture()
    ys, xs = np.nonzero(clean)
    z = (np.float32(1.0) / (np.float32(SCALE) / clean[ys, xs].astype(np.float32))).astype(np.float32)
    p = V.camera_back_project(CAM, P_TRUE, np.stack([xs, ys], -1).astype(np.float32), z)
    q = V.depth_normals_host(clean, CAM, SCALE, 2, 0.05, pose7=P_TRUE)["normals"][ys, xs]
    g = tex[ys, xs]
    xyz, nrm, poses = np.zeros((N, CAP, 3), np.float32), np.zeros((N, CAP, 3), np.float32), np.zeros((N, 8), np.float32)
    gray = np.zeros((N, CAP), np.uint8)
    for s in range(N):
        pick = np.random.default_rng(s).permutation(len(p))[:CAP]
        xyz[s], nrm[s], gray[s] = p[pick], q[pick], g[pick]
        poses[s, :7] = V.iso_mul(P_TRUE, pose_from_xi(START_XI[s]))
    depth = np.stack([np.zeros_like(clean), patched("step"), patched("both")])
    fgray = np.stack([tex, tex, tex])
    fgray[2, 30:44, 4:30] = 255 - fgray[2, 30:44, 4:30]  # a patch of foreign grey
    fn = np.stack([frame_normals_of(d) for d in depth])
    return xyz, nrm, gray, depth, fgray, fn, poses


@functools.lru_cache(maxsize=None)
def host(combo, iters):
    xyz, nrm, gray, depth, fgray, fn, poses = scene()
    normals_on, huber_m, photo_huber = COMBOS[combo]
    out = {k: [] for k in KEYS}
    for s in range(N):
        o = V.icp_points_joint_host(xyz[s], nrm[s], gray[s], depth[s], fgray[s], CAM, SCALE, poses[s, :7], DIST_M, step_eps=STEP_EPS, iters=iters,
                                    min_points=6, frame_normals=fn[s] if normals_on else None, min_cos=MIN_COS, huber_m=huber_m,
                                    photo_scale_m=PHOTO_SCALE_M, photo_huber_grey=photo_huber, count=COUNTS[s],
                                    range2=RANGES[s] if s == 2 else None, residuals=np.full(CAP, SENTINEL, np.float32),
                                    photo_residuals=np.full(CAP, SENTINEL, np.float32))
        out["poses"].append(o["pose"])
        out["stats"].append(np.array([o["stats"]], V.ICP_STATS_DTYPE).view(np.uint32).reshape(-1))
        for k in KEYS[2:]:
            out[k].append(o[k])
    return {k: np.stack(v) for k, v in out.items()}


def device(combo, iters, alias=False, robust=False, photo_scale_m=PHOTO_SCALE_M):
    """vors_icp_points_joint (robust: vors_icp_points_robust) through ctypes -> dict of host arrays. photo_scale_m = 0: NULL grey pointers."""
    import torch
    xyz, nrm, gray, depth, fgray, fn, poses = scene()
    normals_on, huber_m, photo_huber = COMBOS[combo]
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_xyz, d_nrm, d_gray, d_depth, d_fgray, d_fn = t(xyz), t(nrm), t(gray), t(depth.view(np.int16)), t(fgray), t(fn)
    d_counts, d_ranges = t(np.array(COUNTS, np.int32)), t(RANGES)
    d_in = t(poses[:, :7]) if alias else t(poses)
    d_out = d_in if alias else torch.zeros((N, 7), dtype=torch.float32, device=dev)
    d_stats = torch.zeros((N, 6), dtype=torch.int32, device=dev)
    d_sums = torch.zeros((N, 29), dtype=torch.float32, device=dev)
    d_res = torch.full((N, CAP), SENTINEL, dtype=torch.float32, device=dev)
    d_pres = torch.full((N, CAP), SENTINEL, dtype=torch.float32, device=dev)
    d_gates = torch.full((N, 4), 77, dtype=torch.int32, device=dev)  # (the pass clears them itself)
    d_pcounts = torch.full((N, 2), 77, dtype=torch.int32, device=dev)
    ws = torch.empty(V.icp_workspace_bytes(N, CAP), dtype=torch.uint8, device=dev)
    p = V.Batch._dp
    rows, cols = depth.shape[1:]
    pose_args = (p(d_ranges), 0, p(d_in), 28 if alias else 32, p(d_depth))
    tail = (V._ptr(CAM), rows, cols, SCALE, DIST_M, 0.0, STEP_EPS, iters, 6, p(d_fn) if normals_on else None, MIN_COS, huber_m)
    outs = (p(ws), p(d_out), p(d_stats), p(d_sums), p(d_res), p(d_gates))
    if robust:
        V._check(V.lib().vors_icp_points_robust(N, p(d_xyz), p(d_nrm), p(d_counts), CAP, *pose_args, *tail, *outs, V.Batch._stream()))
    else:
        on = photo_scale_m > 0
        V._check(V.lib().vors_icp_points_joint(N, p(d_xyz), p(d_nrm), p(d_gray) if on else None, p(d_counts), CAP, *pose_args,
                                               p(d_fgray) if on else None, *tail, photo_scale_m, photo_huber, *outs, p(d_pres), p(d_pcounts),
                                               V.Batch._stream()))
    torch.cuda.synchronize()
    out = dict(poses=d_out.cpu().numpy(), stats=d_stats.cpu().numpy().view(np.uint32), sums29=d_sums.cpu().numpy(), residuals=d_res.cpu().numpy(),
               gate_counts=d_gates.cpu().numpy().view(np.uint32))
    if not robust:
        out.update(photo_residuals=d_pres.cpu().numpy(), photo_counts=d_pcounts.cpu().numpy().view(np.uint32))
    return out


def same(a, b, what, keys=None):
    for k in keys or b:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)), f"{what}: {k} differs"


# the ranges of list 0 and 1 cover their lists, so the host runs them without one
@pytest.mark.parametrize("iters", [0, 6])
@pytest.mark.parametrize("combo", list(COMBOS))
def test_device_equals_host(combo, iters):
    want = host(combo, iters)
    got = device(combo, iters)
    same(got, want, "device against host")
    st = want["stats"].view(V.ICP_STATS_DTYPE).reshape(-1)
    g, pc = want["gate_counts"], want["photo_counts"]
    print(combo, iters, "status", st["status"].tolist(), "iterations", st["iterations"].tolist(), "gate counts", g.tolist(), "photo counts", pc.tolist())
    assert st["considered"].tolist() == [1, 1025, 2400] and (g[:, 2] == st["matched"]).all() and g[0].tolist() == [0, 0, 0, 0]
    for key in ("residuals", "photo_residuals"):
        assert (want[key][2, :7] == SENTINEL).all() and (want[key][2, 2407:] == SENTINEL).all()
    if iters:
        assert st["status"][0] == V.ICP_TOO_FEW and st["iterations"][0] == 0 and (st["iterations"][1:] > 0).all()
    normals_on, huber_m, photo_huber = COMBOS[combo]
    assert (g[1:, 2] < g[1:, 1]).all() if normals_on else (g[:, 2] == g[:, 1]).all()
    assert (g[1:, 3] > 0).all() if huber_m else (g[:, 3] == 0).all()
    assert pc[0].tolist() == [0, 0] and (pc[1:, 0] > 0).all() and (pc[1:, 0] < g[1:, 2]).all()  # some matched points are not PHOTO
    assert pc[2, 1] > 0 if photo_huber else (pc[:, 1] == 0).all()


@pytest.mark.parametrize("iters", [0, 6])
def test_neutral_case_is_the_robust_pass_on_the_device(iters):
    got = device("nhp", iters, photo_scale_m=0.0)
    same(got, device("nhp", iters, robust=True), "joint without the photometric term against vors_icp_points_robust", KEYS[:5])
    assert (got["photo_counts"] == 0).all()
    pr = got["photo_residuals"]
    assert np.isnan(pr[0, :1]).all() and np.isnan(pr[1, :1025]).all() and np.isnan(pr[2, 7:2407]).all() and (pr[2, :7] == SENTINEL).all()


def test_output_poses_may_alias_the_input():
    same(device("nhp", 6, alias=True), host("nhp", 6), "output poses aliasing the input")


# ------------------------------------------------------------------------------------------------------------ the trackers form
def test_trackers_form():
    import torch
    from test_gpu_trackers_map import MAX_KF, N_SEQ, SHAPES, config, frames_of
    mode = V.CANDIDATES_COARSE_TO_FINE
    rows, cols, _ = SHAPES[mode]
    n_used = 4  # init + 3 tracked frames
    icp = dict(dist_m=0.05, damping=0.0, step_eps=1e-5, iters=6, min_points=50)
    cam = np.array(V.scaled_intrinsics(rows, cols), np.float32)

    def handle(map_on=True, normals=True):
        tr = V.Trackers(config(mode, V.ARITH_FUSED), N_SEQ, rows, cols)
        if map_on:
            tr.enable_map(0, rows * cols * n_used, MAX_KF, 0)
            if normals:
                tr.enable_map_normals(2, 0.05)
        for k, (g, d) in enumerate(frames_of(mode)[:n_used]):
            tr.init(g, d) if k == 0 else tr.track(g, d)
        return tr

    tr = handle()
    gray, depth = frames_of(mode)[n_used - 1]
    fn = V.depth_normals(depth, cam, V.DEPTH_SCALE, 2, 0.05)["normals"]
    joint = dict(frame_normals=fn, min_cos=MIN_COS, huber_m=0.01, photo_scale_m=PHOTO_SCALE_M, photo_huber_grey=PHOTO_HUBER_GREY)
    asked = dict(stats=True, sums29=True, residuals=True, gate_counts=True, photo_residuals=True, photo_counts=True)
    got = tr.icp_map_joint(depth, frame_gray=gray, **asked, **joint, **icp)
    m = tr.map()
    poses = torch.from_numpy(tr.current_frames()[0]).cuda()
    want = V.icp_points_joint(m["xyz"], tr.map_normals(), m["gray"], m["counts"], depth, gray, cam, V.DEPTH_SCALE, poses, **asked, **joint, **icp)
    torch.cuda.synchronize()
    for k in KEYS:
        assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    st, g, pc = V.decode_icp_stats(got["stats"]), got["gate_counts"].cpu().numpy(), got["photo_counts"].cpu().numpy()
    print("status", st["status"].tolist(), "matched", st["matched"].tolist(), "gate counts", g.tolist(), "photo counts", pc.tolist())
    assert (g[:, 2] == st["matched"]).all() and (st["matched"] > 0).all() and np.isfinite(got["poses"].cpu().numpy()).all()
    assert (pc[:, 0] > 0).all() and (pc[:, 0] <= g[:, 2]).all()
    for kw, sentence in ((dict(normals=False), "icp_map: the normals of the map are not enabled (vors_trackers_enable_map_normals)"),
                         (dict(map_on=False), "icp_map: the keyframe map is not enabled (vors_trackers_enable_map)")):
        with pytest.raises(V.VorsError) as e:
            handle(**kw).icp_map_joint(depth, frame_gray=gray, **joint, **icp)
        assert str(e.value) == f"vors_hip error -1: {sentence}"
