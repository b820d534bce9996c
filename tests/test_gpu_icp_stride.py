"""The ICP evaluation's stride loop on the device (vors_icp_points, vors_icp_points_robust, vors_icp_points_joint) against the host twins,
bit for bit. GPU only.

The evaluation grid's x extent is capped at 1024 chunks of 1024 ranks; a longer range goes through the loop over chunks, where a second
trip reuses the LDS behind the last barrier and the counters of a thread carry over its trips. The 64x48 plane and the scenes of
tests/test_gpu_icp_robust.py / tests/test_gpu_icp_joint.py, their model points drawn with replacement to fill n = 2 lists of capacity
2^20 + 2600:

  list 0: count 2^20 + 1500, the whole list, against the "step" frame: 1026 chunks — workgroups 0 and 1 take two trips, and the last chunk
          is partial (476 ranks)
  list 1: count = capacity, the range (2^20, 2^20) clipped by the count, against the "both" frame with its patch of foreign grey: the
          2600 ranks behind 2^20, a partial last chunk again

The plain pass, the robust one with the normal gate and Huber weights, and the joint one with both and the photo Huber, at iters 0 and 2:
poses, stats, sums29, the residual arrays (a sentinel outside the ranges), gate counts and photo counts equal the host's.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from test_icp_joint_host import PHOTO_HUBER_GREY, PHOTO_SCALE_M, texture
from test_icp_robust_host import CAM, DIST_M, HUBER_M, MIN_COS, P_TRUE, SCALE, frame_normals_of, patched, pose_from_xi, to_depth, corner_z

N = 2
CAP = (1 << 20) + 2600
COUNTS = ((1 << 20) + 1500, CAP)
RANGES = np.array([[0, 0x7FFFFFFF], [1 << 20, 1 << 20]], np.int32)  # (list 0: the whole list)
WRITTEN = ((0, COUNTS[0]), (1 << 20, CAP))  # the ranks of each list's clipped range
START_XI = ([0.004, -0.003, 0.005, 0.004, -0.005, 0.003], [-0.003, 0.004, 0.002, -0.003, 0.004, 0.005])
STEP_EPS = 2e-5
SENTINEL = 42.0
FORMS = ("plain", "robust", "joint")
KEYS = {"plain": ("poses", "stats", "sums29", "residuals"),
        "robust": ("poses", "stats", "sums29", "residuals", "gate_counts"),
        "joint": ("poses", "stats", "sums29", "residuals", "gate_counts", "photo_residuals", "photo_counts")}
ICP = dict(step_eps=STEP_EPS, min_points=6)
ROBUST = dict(min_cos=MIN_COS, huber_m=HUBER_M)
JOINT = dict(photo_scale_m=PHOTO_SCALE_M, photo_huber_grey=PHOTO_HUBER_GREY)


@functools.lru_cache(maxsize=None)
def scene():
    """-> host arrays: xyz / normals [N, CAP, 3], list grey [N, CAP], depth [N, rows, cols] u16, frame grey [N, rows, cols], frame normals
    [N, rows, cols, 3], start poses [N, 7]."""
    clean, tex = to_depth(corner_z()), texture()
    ys, xs = np.nonzero(clean)
    z = (np.float32(1.0) / (np.float32(SCALE) / clean[ys, xs].astype(np.float32))).astype(np.float32)
    p = V.camera_back_project(CAM, P_TRUE, np.stack([xs, ys], -1).astype(np.float32), z)
    q = V.depth_normals_host(clean, CAM, SCALE, 2, 0.05, pose7=P_TRUE)["normals"][ys, xs]
    g = tex[ys, xs]
    pick = np.stack([np.random.default_rng(40 + s).integers(0, len(p), CAP) for s in range(N)])
    poses = np.stack([V.iso_mul(P_TRUE, pose_from_xi(xi)) for xi in START_XI]).astype(np.float32)
    depth = np.stack([patched("step"), patched("both")])
    fgray = np.stack([tex, tex])
    fgray[1, 30:44, 4:30] = 255 - fgray[1, 30:44, 4:30]  # a patch of foreign grey
    fn = np.stack([frame_normals_of(d) for d in depth])
    return p[pick], q[pick], g[pick], depth, fgray, fn, poses


@functools.lru_cache(maxsize=None)
def host(form, iters):
    xyz, nrm, gray, depth, fgray, fn, poses = scene()
    out = {k: [] for k in KEYS[form]}
    for s in range(N):
        kw = dict(ICP, iters=iters, count=COUNTS[s], range2=RANGES[s].view(np.uint32) if s == 1 else None,
                  residuals=np.full(CAP, SENTINEL, np.float32))
        if form == "plain":
            o = V.icp_points_host(xyz[s], nrm[s], depth[s], CAM, SCALE, poses[s], DIST_M, **kw)
        elif form == "robust":
            o = V.icp_points_robust_host(xyz[s], nrm[s], depth[s], CAM, SCALE, poses[s], DIST_M, frame_normals=fn[s], **ROBUST, **kw)
        else:
            o = V.icp_points_joint_host(xyz[s], nrm[s], gray[s], depth[s], fgray[s], CAM, SCALE, poses[s], DIST_M, frame_normals=fn[s], **ROBUST,
                                        **JOINT, photo_residuals=np.full(CAP, SENTINEL, np.float32), **kw)
        out["poses"].append(o["pose"])
        out["stats"].append(np.array([o["stats"]], V.ICP_STATS_DTYPE).view(np.uint32).reshape(-1))
        for k in KEYS[form][2:]:
            out[k].append(o[k])
    return {k: np.stack(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def device_scene():
    import torch
    xyz, nrm, gray, depth, fgray, fn, poses = scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return dict(xyz=t(xyz), nrm=t(nrm), gray=t(gray), depth=t(depth.view(np.int16)), fgray=t(fgray), fn=t(fn), poses=t(poses),
                counts=t(np.array(COUNTS, np.int32)), ranges=t(RANGES), ws=torch.empty(V.icp_workspace_bytes(N, CAP), dtype=torch.uint8).cuda())


def device(form, iters):
    import torch
    d = device_scene()
    sentinels = lambda: torch.full((N, CAP), SENTINEL, dtype=torch.float32).cuda()  # noqa: E731
    kw = dict(ICP, iters=iters, ranges=d["ranges"], workspace=d["ws"], stats=True, sums29=True, residuals=sentinels())
    if form == "plain":
        o = V.icp_points(d["xyz"], d["nrm"], d["counts"], d["depth"], CAM, SCALE, d["poses"], DIST_M, **kw)
    elif form == "robust":
        o = V.icp_points_robust(d["xyz"], d["nrm"], d["counts"], d["depth"], CAM, SCALE, d["poses"], DIST_M, frame_normals=d["fn"], **ROBUST,
                                gate_counts=True, **kw)
    else:
        o = V.icp_points_joint(d["xyz"], d["nrm"], d["gray"], d["counts"], d["depth"], d["fgray"], CAM, SCALE, d["poses"], DIST_M,
                               frame_normals=d["fn"], **ROBUST, **JOINT, gate_counts=True, photo_residuals=sentinels(), photo_counts=True, **kw)
    torch.cuda.synchronize()
    return {k: np.ascontiguousarray(v.cpu().numpy()).view(np.uint32) for k, v in o.items()}


@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("form", FORMS)
def test_stride_loop_equals_host(form, iters):
    want = host(form, iters)
    got = device(form, iters)
    assert sorted(got) == sorted(KEYS[form])
    for k in KEYS[form]:
        assert np.array_equal(got[k].reshape(N, -1), np.ascontiguousarray(want[k]).view(np.uint32).reshape(N, -1)), f"{form}, iters {iters}: {k} differs"
    st = want["stats"].view(V.ICP_STATS_DTYPE).reshape(-1)
    print(form, iters, "status", st["status"].tolist(), "iterations", st["iterations"].tolist(), "matched", st["matched"].tolist(),
          *[(k, want[k].tolist()) for k in ("gate_counts", "photo_counts") if k in want])
    # what the comparison is worth: the ranges are the ones described, work was done on both sides of every boundary, every counter counts
    assert st["considered"].tolist() == [COUNTS[0], 2600] and (st["iterations"] == iters).all()
    assert (st["matched"] > 1500).all() and st["matched"][0] > (1 << 20) // 2
    for k in ("residuals", "photo_residuals"):
        if k in want:
            for s, (a, b) in enumerate(WRITTEN):
                r = want[k][s]
                assert (r[:a] == SENTINEL).all() and (r[b:] == SENTINEL).all() and not (r[a:b] == SENTINEL).any()
                assert np.isfinite(r[a:a + 1024]).any() and np.isfinite(r[b - 476:b]).any()   # (the first chunk and the partial last one)
    if form != "plain":
        g = want["gate_counts"]
        assert (g[:, 2] == st["matched"]).all() and (g[:, 2] < g[:, 1]).all() and (g[:, 1] <= g[:, 0]).all() and (g[:, 3] > 0).all()
    if form == "joint":
        pc = want["photo_counts"]
        assert (pc[:, 0] > 0).all() and (pc[:, 0] < g[:, 2]).all() and pc[1, 1] > 0
