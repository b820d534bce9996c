"""The keyframe map aligned to depth frames on the sequence handle (vors_trackers_icp_map, Trackers.icp_map). GPU only.

Coarse-to-fine sequences of tests/test_gpu_trackers_map.py (96x128, six sequences), a level-0 map with normals, a few track calls.

  1. the entry equals icp_points() on the handle's own map, normals, counters, poses and the frame, bit for bit
  2. the call only reads: the tracker's poses and the next track call's results keep their bits with and without it
  3. refused without map normals, with the sentence pinned
  4. statuses are those of the enum and every output pose is finite; the refined-against-tracked pose differences are printed only
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from test_gpu_trackers_map import MAX_KF, N_SEQ, SHAPES, config, frames_of, same_bits

MODE, ARITH = V.CANDIDATES_COARSE_TO_FINE, V.ARITH_FUSED
N_USED = 4
ICP = dict(dist_m=0.05, damping=0.0, step_eps=1e-5, iters=6, min_points=50)


def tracked(with_icp, normals=True):
    """N_USED frames; with_icp: an icp_map call after every track -> (per frame poses / status / stats, the icp results of the last call, handle)."""
    rows, cols, _ = SHAPES[MODE]
    tr = V.Trackers(config(MODE, ARITH), N_SEQ, rows, cols)
    tr.enable_map(0, rows * cols * N_USED, MAX_KF, 0)
    if normals:
        tr.enable_map_normals(2, 0.05)
    rec, last = [], None
    for k, (g, d) in enumerate(frames_of(MODE)[:N_USED]):
        if k == 0:
            tr.init(g, d)
        else:
            tr.track(g, d)
        if with_icp and k > 0:
            last = tr.icp_map(d, stats=True, sums29=True, residuals=True, **ICP)
        poses, status, kf = tr.current_frames()
        rec.append(dict(poses=poses, status=status, kf=kf, stats=tr.stats().copy() if k else None))
    return rec, last, tr


def test_entry_equals_icp_points_and_only_reads():
    import torch
    rows, cols, _ = SHAPES[MODE]
    rec, got, tr = tracked(True)
    bare, _, _ = tracked(False)
    for a, b in zip(rec, bare):  # 2.
        assert same_bits(a["poses"], b["poses"]) and same_bits(a["status"], b["status"]) and same_bits(a["kf"], b["kf"])
        assert (a["stats"] is None and b["stats"] is None) or a["stats"].tobytes() == b["stats"].tobytes()
    # 1. the same pass through the handle-free entry, on copies of the handle's own buffers
    m = tr.map()
    depth = frames_of(MODE)[N_USED - 1][1]
    poses = torch.from_numpy(rec[-1]["poses"]).cuda()
    cam = np.array(V.scaled_intrinsics(rows, cols), np.float32)
    want = V.icp_points(m["xyz"], tr.map_normals(), m["counts"], depth, cam, V.DEPTH_SCALE, poses, stats=True, sums29=True, residuals=True, **ICP)
    torch.cuda.synchronize()
    for k in ("poses", "stats", "sums29", "residuals"):
        assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    # 4.
    st = V.decode_icp_stats(got["stats"])
    refined = got["poses"].cpu().numpy()
    assert np.isin(st["status"], [V.ICP_ITERATIONS, V.ICP_CONVERGED, V.ICP_TOO_FEW, V.ICP_SINGULAR]).all() and np.isfinite(refined).all()
    assert (st["considered"] == np.minimum(m["counts"].cpu().numpy().view(np.uint32), rows * cols * N_USED)).all() and (st["matched"] > 0).all()
    print("status", st["status"].tolist(), "iterations", st["iterations"].tolist(), "matched", st["matched"].tolist(), "rms", st["rms"].tolist())
    print("max |refined - tracked| per sequence", np.abs(refined - rec[-1]["poses"]).max(1).tolist())


def test_refused_without_map_normals():
    _, _, tr = tracked(False, normals=False)
    with pytest.raises(V.VorsError) as e:
        tr.icp_map(frames_of(MODE)[0][1], **ICP)
    assert str(e.value) == "vors_hip error -1: icp_map: the normals of the map are not enabled (vors_trackers_enable_map_normals)"


def test_refused_without_map():
    """A handle without a map, no frame tracked: the library's own sentence, as from icp_map_robust() and icp_map_joint()."""
    rows, cols, _ = SHAPES[MODE]
    tr = V.Trackers(config(MODE, ARITH), N_SEQ, rows, cols)
    with pytest.raises(V.VorsError) as e:
        tr.icp_map(frames_of(MODE)[0][1], **ICP)
    assert str(e.value) == "vors_hip error -1: icp_map: the keyframe map is not enabled (vors_trackers_enable_map)"
