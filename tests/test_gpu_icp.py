"""Point-to-plane ICP on the device (vors_icp_points) against its host twin (vors_icp_points_host), bit for bit. GPU only.

Planes of 37x29 and 64x48 pixels; n = 3 lists of capacity 2600 — three chunks of 1024 with a tail in the last — cut from the corner scene
of tests/test_icp_host.py at twice the plane's resolution, so that a list is longer than its plane. Case "clipped": counts {2650 (clipped
to 2600), 1025, 0}; case "few": counts {2500, 300, 1} with min_points 400. Start poses 32 bytes apart; with and without ranges.

  1. poses, stats, sums29 and residuals equal the host's for iters 0, 1 and 8 (uint32 views); the residual buffer starts as a sentinel,
     so ranks outside a range are seen to be untouched
  2. the lists stop at different rounds (one converges earlier, one is frozen as TOO_FEW) and each equals the list run alone
  3. output poses aliasing the input, each nullable output alone, a larger capacity: the same bits
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from test_icp_host import DIST_M, SCALE, corner_depth, model_of, pose_from_xi

SHAPES = {"37x29": (29, 37), "64x48": (48, 64)}
CAP, N = 2600, 3
CASES = {"clipped": ((CAP + 50, 1025, 0), 6), "few": ((2500, 300, 1), 400)}
RANGES = np.array([[7, 2200], [1000, 5000], [0, 3]], np.int32)
STEP_EPS = 2e-5
SENTINEL = 42.0
TRUE_XI = ([0.3, -0.2, 0.1, 0.05, -0.1, 0.08], [-0.1, 0.25, 0.2, -0.04, 0.06, 0.1], [0.0, 0.1, -0.2, 0.02, 0.03, -0.05])
START_XI = ([0.0004, 0, 0, 0, 0, 0], [0.012, -0.01, 0.015, 0.008, -0.01, 0.006], [0.01, 0, 0, 0, 0, 0])


def cam_of(rows, cols, up=1):
    return np.array([(cols / 2) * up - 0.5, (rows / 2) * up - 0.5, 0.94 * cols * up, 0.95 * cols * up, 0.0], np.float32)


@functools.lru_cache(maxsize=None)
def scene(shape, cap=CAP):
    """-> host arrays: xyz / normals [N, cap, 3], depth [N, rows, cols] u16, start poses [N, 8] (32 bytes apart), cam5."""
    rows, cols = SHAPES[shape]
    fine = corner_depth(2 * rows, 2 * cols, cam_of(rows, cols, 2))
    depth = corner_depth(rows, cols, cam_of(rows, cols))
    xyz, nrm, poses = np.zeros((N, cap, 3), np.float32), np.zeros((N, cap, 3), np.float32), np.zeros((N, 8), np.float32)
    for s in range(N):
        truth = pose_from_xi(TRUE_XI[s])
        p, q = model_of(fine, truth, cam_of(rows, cols, 2))
        pick = np.random.default_rng(s).permutation(len(p))[:CAP]
        xyz[s, :CAP], nrm[s, :CAP] = p[pick], q[pick]
        poses[s, :7] = V.iso_mul(truth, pose_from_xi(START_XI[s]))
    return xyz, nrm, np.stack([depth] * N), poses, cam_of(rows, cols)


def host(shape, case, iters, ranged, cap=CAP, lists=range(N)):
    xyz, nrm, depth, poses, cam = scene(shape, cap)
    counts, min_points = CASES[case]
    out = dict(poses=[], stats=[], sums29=[], residuals=[])
    for s in lists:
        o = V.icp_points_host(xyz[s], nrm[s], depth[s], cam, SCALE, poses[s, :7], DIST_M, step_eps=STEP_EPS, iters=iters, min_points=min_points,
                              count=counts[s], range2=RANGES[s] if ranged else None, residuals=np.full(cap, SENTINEL, np.float32))
        out["poses"].append(o["pose"])
        out["stats"].append(np.array([o["stats"]], V.ICP_STATS_DTYPE).view(np.uint32))
        out["sums29"].append(o["sums29"])
        out["residuals"].append(o["residuals"])
    return {k: np.stack(v) for k, v in out.items()}


def device(shape, case, iters, ranged, cap=CAP, lists=range(N), alias=False, only=None):
    """vors_icp_points through ctypes -> dict of host arrays of the outputs asked for (only = one of the nullable ones, None = all)."""
    import torch
    lists = list(lists)
    n = len(lists)
    xyz, nrm, depth, poses, cam = scene(shape, cap)
    counts, min_points = CASES[case]
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_xyz, d_nrm, d_depth = t(xyz[lists]), t(nrm[lists]), t(depth[lists].view(np.int16))
    d_counts, d_ranges = t(np.array(counts, np.int32)[lists]), t(RANGES[lists])
    d_in = t(poses[lists, :7]) if alias else t(poses[lists])
    d_out = d_in if alias else torch.zeros((n, 7), dtype=torch.float32, device=dev)
    want = lambda name: only is None or only == name  # noqa: E731
    d_stats = torch.zeros((n, 6), dtype=torch.int32, device=dev) if want("stats") else None
    d_sums = torch.zeros((n, 29), dtype=torch.float32, device=dev) if want("sums29") else None
    d_res = torch.full((n, cap), SENTINEL, dtype=torch.float32, device=dev) if want("residuals") else None
    ws = torch.empty(V.icp_workspace_bytes(n, cap), dtype=torch.uint8, device=dev)
    p = V.Batch._dp
    rows, cols = SHAPES[shape]
    V._check(V.lib().vors_icp_points(n, p(d_xyz), p(d_nrm), p(d_counts), cap, p(d_ranges) if ranged else None, 0, p(d_in), 28 if alias else 32,
                                     p(d_depth), V._ptr(cam), rows, cols, SCALE, DIST_M, 0.0, STEP_EPS, iters, min_points, p(ws), p(d_out),
                                     p(d_stats), p(d_sums), p(d_res), V.Batch._stream()))
    torch.cuda.synchronize()
    out = dict(poses=d_out.cpu().numpy())
    if d_stats is not None:
        out["stats"] = d_stats.cpu().numpy().view(np.uint32)
    if d_sums is not None:
        out["sums29"] = d_sums.cpu().numpy()
    if d_res is not None:
        out["residuals"] = d_res.cpu().numpy()
    return out


def same(a, b, what):
    for k in b:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), f"{what}: {k} differs"


def test_workspace_bytes():
    assert V.icp_workspace_bytes(N, CAP) == N * (3 * 29 * 4 + 48) and V.icp_workspace_bytes(1, 1024) == 29 * 4 + 48
    assert V.icp_workspace_bytes(0, CAP) == 0 and V.icp_workspace_bytes(N, 0) == 0


@pytest.mark.parametrize("ranged", [False, True])
@pytest.mark.parametrize("iters", [0, 1, 8])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_equals_host(shape, case, iters, ranged):
    want = host(shape, case, iters, ranged)
    got = device(shape, case, iters, ranged)
    same(got, want, "device against host")
    st = want["stats"].view(V.ICP_STATS_DTYPE).reshape(-1)
    counts, _ = CASES[case]
    if not ranged:
        assert st["considered"].tolist() == [min(c, CAP) for c in counts]
        assert (want["residuals"][1, counts[1]:] == SENTINEL).all()  # ranks beyond the list: untouched
    else:
        assert (want["residuals"][0, :7] == SENTINEL).all() and (want["residuals"][0, 2207:] == SENTINEL).all()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_lists_stop_on_their_own(shape):
    for case in CASES:
        got = device(shape, case, 8, False)
        st = got["stats"].view(V.ICP_STATS_DTYPE).reshape(-1)
        print(shape, case, st)
        if case == "clipped":
            assert st["status"].tolist() == [V.ICP_CONVERGED, V.ICP_CONVERGED, V.ICP_TOO_FEW]
            assert 0 < st["iterations"][0] < st["iterations"][1] <= 8 and st["iterations"][2] == 0
        else:
            assert st["status"].tolist() == [V.ICP_CONVERGED, V.ICP_TOO_FEW, V.ICP_TOO_FEW] and st["iterations"].tolist()[1:] == [0, 0]
            assert 0 < st["matched"][1] < 400
        for s in range(N):
            alone = device(shape, case, 8, False, lists=[s])
            same({k: v[s:s + 1] for k, v in got.items()}, alone, f"list {s} alone")


def test_aliasing_nullable_outputs_and_capacity():
    shape, case = "64x48", "clipped"
    want = device(shape, case, 8, True)
    same(device(shape, case, 8, True, alias=True), want, "output poses aliasing the input")
    for only in ("stats", "sums29", "residuals"):
        got = device(shape, case, 8, True, only=only)
        assert set(got) == {"poses", only}
        same(got, {k: want[k] for k in got}, f"{only} alone")
    big = device(shape, case, 8, True, cap=5000)
    assert np.array_equal(big["residuals"][:, :CAP].view(np.uint32), want["residuals"].view(np.uint32)) and (big["residuals"][:, CAP:] == SENTINEL).all()
    same({k: big[k] for k in ("poses", "stats", "sums29")}, {k: want[k] for k in ("poses", "stats", "sums29")}, "capacity 5000")
