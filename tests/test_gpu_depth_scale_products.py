"""The batch products at level 0 at depth scales 1000 and 30000 (tests/depth_scales.py): vors_batch_reproject_depth, vors_batch_fuse_depth
and vors_batch_point_cloud. GPU only.

The checkers are those of test_gpu_reproject_depth.py, test_gpu_fuse_depth.py and test_gpu_point_cloud.py, with the scale passed through
and nothing else changed: the u16 depth map is to_depth of the device's own z-buffer, the residual plane and the counts against float64,
the merge exact against vors_fuse_depth_pixels on the device's own keys, the clouds the oracle's points back-projected.

Saturation: the scenes end at about 2.18 m, which is 65535 / 30000, so at the tracked models next to nothing saturates. The products are
therefore also run at a model moved along +z, by the first of PUSHES_M at which the host helper alone (to_depth of the float64 depths)
gives 65535 on at least 100 pixels of every pair; the test asserts that the device's depth maps saturate there."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
import test_gpu_fuse_depth as FD
import test_gpu_point_cloud as PC
import test_gpu_reproject_depth as RD
from depth_scales import scale_id
from test_gpu_first_principles import level_intrinsics

F32 = np.float32
PUSHES_M = (0.02, 0.05, 0.1, 0.2, 0.4)
CASES = [((120, 160, 4), V.CANDIDATES_DENSE, "fused", 1000.0, 1.0), ((120, 160, 4), V.CANDIDATES_DENSE, "reference", 30000.0, 3e-7),
         ((120, 160, 4), V.CANDIDATES_COARSE_TO_FINE, "fused", 30000.0, 1.0), ((122, 162, 3), V.CANDIDATES_DENSE, "exact", 1000.0, 3e-7)]
IDS = [f"{c[0][1]}x{c[0][0]}L{c[0][2]}-{('c2f', 'dense', 'dso')[c[1]]}-{c[2]}-{scale_id(c[3], c[4])}" for c in CASES]


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def scene(request):
    shape, mode, arith, scale, variance = request.param
    return FD.with_weights_and_holes(RD.Scene(shape, mode, arith, scale=scale, idepth_variance=variance))


def pushed_models(sc):
    """Each pair's tracked model moved along +z until the host helper alone saturates on at least 100 points of every pair."""
    k5 = level_intrinsics(sc.intr, 0)
    for push in PUSHES_M:
        models = sc.models[:, 0].copy()
        models[:, 2] += F32(push)
        saturated = [int((RD.to_depth_np(sc.scale, (1.0 / RD.z64(sc.b, p, 0, k5, models[p])[1]).astype(F32)) == 65535).sum()) for p in range(RD.N)]
        if min(saturated) >= 100:
            return models, push
    raise AssertionError(f"no push of {PUSHES_M} m saturates 100 points of every pair: {saturated}")


def test_the_scene_is_at_its_scale(scene):
    sc = scene
    kd = sc.kd.cpu().numpy().view(np.uint16)
    metres = kd[kd > 0].astype(np.float64) / sc.scale
    assert 1.5 < metres.min() and metres.max() < 2.7 and (V.decode_stats(sc.stats)["n_points"][:, 0] > 0).all()
    assert (sc.cd_host > 0).any() and np.abs(np.median(sc.cd_host[sc.cd_host > 0]) / sc.scale - np.median(metres)) < 0.2


def test_reprojected_depth_map_is_to_depth_of_the_z_buffer(scene):
    RD.check_pixel_assignment_depth_values_and_depth_map(scene, levels=(0,))


def test_residual_plane_and_counts_against_float64(scene):
    RD.check_residual_plane_and_counts_against_float64(scene)


def test_fused_depth_equals_the_host_merge(scene):
    FD.check_merge_exact_against_the_host_entry(scene)


def test_the_depth_maps_saturate_at_30000(scene):
    import torch
    sc = scene
    if sc.scale != 30000.0:
        assert not (RD.to_depth_np(sc.scale, F32(1.0) / F32(2.8)) == 65535).any()   # nothing within reach of these scenes saturates at 1000
        return
    rows, cols = sc.shape(0)
    models, push = pushed_models(sc)
    d_models = torch.from_numpy(models).cuda()
    m = RD.everything(sc.b, 0, d_models, sc.cd)
    sat = 0
    for p in range(RD.N):
        RD.assert_assignment_and_depth_map(m, p, rows, cols, f"pair {p} pushed {push} m", scale=sc.scale)
        d = m["pred_depth"][p].view(np.uint16)
        assert (d == 65535).any() and ((d > 0) & (d < 65535)).any(), f"pair {p}: no pixel of the reprojected depth map saturates"
        sat += int((d == 65535).sum())
    print(f"pushed {push} m: {sat} saturated pixels")
    filled = FD.fuse_all(sc.b, d_models, sc.holes, tol=max(RD.TOL_M, 2 * push), fill_min_weight=1)
    FD.assert_exact_against_host_entry(filled, sc.holes_host, None, max(RD.TOL_M, 2 * push), 255, 1, what="pushed, holes", scale=sc.scale)
    at = (filled["zkey"] != FD.EMPTY) & (sc.holes_host == 0)
    assert (filled["depth"][at] == m["pred_depth"].view(np.uint16)[at]).all()
    assert (filled["depth"][at] == 65535).any(), "no filled pixel saturates"
    assert (filled["counts"][:, FD.AGREE] > 0).all()


CLOUDS = [((120, 160, 4), V.CANDIDATES_DENSE, "fused", 1000.0, 1.0), ((120, 160, 4), V.CANDIDATES_COARSE_TO_FINE, "reference", 30000.0, 3e-7),
          ((122, 162, 3), V.CANDIDATES_DENSE, "reference", 30000.0, 1.0)]


@pytest.mark.parametrize("shape,mode,arith,scale,variance", CLOUDS,
                         ids=[f"{c[0][1]}x{c[0][0]}L{c[0][2]}-{('c2f', 'dense', 'dso')[c[1]]}-{c[2]}-{scale_id(c[3], c[4])}" for c in CLOUDS])
def test_point_clouds_equal_the_oracle(shape, mode, arith, scale, variance):
    sc = PC.Scene(shape, mode, arith, scale=scale, idepth_variance=variance)
    PC.check_clouds_equal_the_oracle(sc)
    z = 1.0 / sc.oracle()[0][0][1].astype(np.float64)   # the scene sits where it sat: the points of pair 0, level 0, in metres
    assert 1.5 < z.min() and z.max() < 2.7
