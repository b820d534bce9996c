"""The robust point-to-plane ICP on the device (vors_icp_points_robust, Trackers.icp_map_robust) against its host twin
(vors_icp_points_robust_host), bit for bit. GPU only.

The 48x64 scene of tests/test_icp_robust_host.py: the corner's model against frames with foreign patches. n = 3 lists of capacity 2500 in
one call: list 0 of count 1 against a plane of zeros (frozen as TOO_FEW in the first round: the frozen-list path, stale partials), list 1
of count 1025 against the "step" frame, list 2 of count 2500 against the "both" frame through the range (7, 2400). Start poses 32 bytes
apart.

  1. poses, stats, sums29, residuals and gate counts equal the host's for normals on / off x Huber on / off, iters 0 and 6
  2. the neutral case equals the device's vors_icp_points
  3. output poses aliasing the input: the same bits
  4. Trackers.icp_map_robust equals icp_points_robust on the handle's own pointers, and refuses without the map or its normals
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from test_icp_robust_host import CAM, DIST_M, HUBER_M, MIN_COS, P_TRUE, SCALE, frame_normals_of, patched, pose_from_xi, to_depth, corner_z

CAP, N = 2500, 3
COUNTS = (1, 1025, 2500)
RANGES = np.array([[0, 1], [0, 4000], [7, 2400]], np.int32)  # (list 0 and 1: the whole list)
START_XI = ([0.001, 0, 0, 0, 0, 0], [0.004, -0.003, 0.005, 0.004, -0.005, 0.003], [-0.003, 0.004, 0.002, -0.003, 0.004, 0.005])
STEP_EPS = 2e-5
SENTINEL = 42.0
COMBOS = {"neutral": (False, 0.0), "normals": (True, 0.0), "huber": (False, HUBER_M), "both": (True, HUBER_M)}
KEYS = ("poses", "stats", "sums29", "residuals", "gate_counts")


@functools.lru_cache(maxsize=None)
def scene():
    """-> host arrays: xyz / normals [N, CAP, 3], depth [N, rows, cols] u16, frame normals [N, rows, cols, 3], start poses [N, 8]."""
    clean = to_depth(corner_z())
    ys, xs = np.nonzero(clean)
    z = (np.float32(1.0) / (np.float32(SCALE) / clean[ys, xs].astype(np.float32))).astype(np.float32)
    p = V.camera_back_project(CAM, P_TRUE, np.stack([xs, ys], -1).astype(np.float32), z)
    q = V.depth_normals_host(clean, CAM, SCALE, 2, 0.05, pose7=P_TRUE)["normals"][ys, xs]
    xyz, nrm, poses = np.zeros((N, CAP, 3), np.float32), np.zeros((N, CAP, 3), np.float32), np.zeros((N, 8), np.float32)
    for s in range(N):
        pick = np.random.default_rng(s).permutation(len(p))[:CAP]
        xyz[s], nrm[s] = p[pick], q[pick]
        poses[s, :7] = V.iso_mul(P_TRUE, pose_from_xi(START_XI[s]))
    depth = np.stack([np.zeros_like(clean), patched("step"), patched("both")])
    fn = np.stack([frame_normals_of(d) for d in depth])
    assert not fn[0].any()
    return xyz, nrm, depth, fn, poses


@functools.lru_cache(maxsize=None)
def host(combo, iters):
    xyz, nrm, depth, fn, poses = scene()
    normals_on, huber_m = COMBOS[combo]
    out = {k: [] for k in KEYS}
    for s in range(N):
        o = V.icp_points_robust_host(xyz[s], nrm[s], depth[s], CAM, SCALE, poses[s, :7], DIST_M, step_eps=STEP_EPS, iters=iters, min_points=6,
                                     frame_normals=fn[s] if normals_on else None, min_cos=MIN_COS, huber_m=huber_m, count=COUNTS[s],
                                     range2=RANGES[s] if s == 2 else None, residuals=np.full(CAP, SENTINEL, np.float32))
        out["poses"].append(o["pose"])
        out["stats"].append(np.array([o["stats"]], V.ICP_STATS_DTYPE).view(np.uint32).reshape(-1))
        for k in ("sums29", "residuals", "gate_counts"):
            out[k].append(o[k])
    return {k: np.stack(v) for k, v in out.items()}


def device(combo, iters, alias=False, plain=False):
    """vors_icp_points_robust (plain: vors_icp_points) through ctypes -> dict of host arrays."""
    import torch
    xyz, nrm, depth, fn, poses = scene()
    normals_on, huber_m = COMBOS[combo]
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_xyz, d_nrm, d_depth, d_fn = t(xyz), t(nrm), t(depth.view(np.int16)), t(fn)
    d_counts, d_ranges = t(np.array(COUNTS, np.int32)), t(RANGES)
    d_in = t(poses[:, :7]) if alias else t(poses)
    d_out = d_in if alias else torch.zeros((N, 7), dtype=torch.float32, device=dev)
    d_stats = torch.zeros((N, 6), dtype=torch.int32, device=dev)
    d_sums = torch.zeros((N, 29), dtype=torch.float32, device=dev)
    d_res = torch.full((N, CAP), SENTINEL, dtype=torch.float32, device=dev)
    d_gates = torch.full((N, 4), 77, dtype=torch.int32, device=dev)  # (the pass clears them itself)
    ws = torch.empty(V.icp_workspace_bytes(N, CAP), dtype=torch.uint8, device=dev)
    p = V.Batch._dp
    rows, cols = depth.shape[1:]
    head = (N, p(d_xyz), p(d_nrm), p(d_counts), CAP, p(d_ranges), 0, p(d_in), 28 if alias else 32, p(d_depth), V._ptr(CAM), rows, cols, SCALE, DIST_M,
            0.0, STEP_EPS, iters, 6)
    if plain:
        V._check(V.lib().vors_icp_points(*head, p(ws), p(d_out), p(d_stats), p(d_sums), p(d_res), V.Batch._stream()))
    else:
        V._check(V.lib().vors_icp_points_robust(*head, p(d_fn) if normals_on else None, MIN_COS, huber_m, p(ws), p(d_out), p(d_stats), p(d_sums),
                                                p(d_res), p(d_gates), V.Batch._stream()))
    torch.cuda.synchronize()
    out = dict(poses=d_out.cpu().numpy(), stats=d_stats.cpu().numpy().view(np.uint32), sums29=d_sums.cpu().numpy(), residuals=d_res.cpu().numpy())
    if not plain:
        out["gate_counts"] = d_gates.cpu().numpy().view(np.uint32)
    return out


def same(a, b, what):
    for k in b:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)), f"{what}: {k} differs"


# the ranges of list 0 and 1 cover their lists, so the host runs them without one
@pytest.mark.parametrize("iters", [0, 6])
@pytest.mark.parametrize("combo", list(COMBOS))
def test_device_equals_host(combo, iters):
    want = host(combo, iters)
    got = device(combo, iters)
    same(got, want, "device against host")
    st = want["stats"].view(V.ICP_STATS_DTYPE).reshape(-1)
    g = want["gate_counts"]
    print(combo, iters, "status", st["status"].tolist(), "iterations", st["iterations"].tolist(), "gate counts", g.tolist())
    assert st["considered"].tolist() == [1, 1025, 2400] and (g[:, 2] == st["matched"]).all() and g[0].tolist() == [0, 0, 0, 0]
    assert (want["residuals"][2, :7] == SENTINEL).all() and (want["residuals"][2, 2407:] == SENTINEL).all()
    if iters:
        assert st["status"][0] == V.ICP_TOO_FEW and st["iterations"][0] == 0 and (st["iterations"][1:] > 0).all()
    normals_on, huber_m = COMBOS[combo]
    assert (g[1:, 2] < g[1:, 1]).all() if normals_on else (g[:, 2] == g[:, 1]).all()
    assert (g[1:, 3] > 0).all() if huber_m else (g[:, 3] == 0).all()


@pytest.mark.parametrize("iters", [0, 6])
def test_neutral_case_is_the_plain_pass_on_the_device(iters):
    got = device("neutral", iters)
    same(got, device("neutral", iters, plain=True), "robust neutral against vors_icp_points")


def test_output_poses_may_alias_the_input():
    same(device("both", 6, alias=True), host("both", 6), "output poses aliasing the input")


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
    depth = frames_of(mode)[n_used - 1][1]
    fn = V.depth_normals(depth, cam, V.DEPTH_SCALE, 2, 0.05)["normals"]
    robust = dict(frame_normals=fn, min_cos=MIN_COS, huber_m=0.01)
    got = tr.icp_map_robust(depth, stats=True, sums29=True, residuals=True, gate_counts=True, **robust, **icp)
    m = tr.map()
    poses = torch.from_numpy(tr.current_frames()[0]).cuda()
    want = V.icp_points_robust(m["xyz"], tr.map_normals(), m["counts"], depth, cam, V.DEPTH_SCALE, poses, stats=True, sums29=True, residuals=True,
                               gate_counts=True, **robust, **icp)
    torch.cuda.synchronize()
    for k in KEYS:
        assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    st, g = V.decode_icp_stats(got["stats"]), got["gate_counts"].cpu().numpy()
    print("status", st["status"].tolist(), "matched", st["matched"].tolist(), "gate counts", g.tolist())
    assert (g[:, 2] == st["matched"]).all() and (st["matched"] > 0).all() and np.isfinite(got["poses"].cpu().numpy()).all()
    for kw, sentence in ((dict(normals=False), "icp_map: the normals of the map are not enabled (vors_trackers_enable_map_normals)"),
                         (dict(map_on=False), "icp_map: the keyframe map is not enabled (vors_trackers_enable_map)")):
        with pytest.raises(V.VorsError) as e:
            handle(**kw).icp_map_robust(depth, **robust, **icp)
        assert str(e.value) == f"vors_hip error -1: {sentence}"
