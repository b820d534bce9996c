"""Depth reprojection of a prepared batch (vors_batch_reproject_depth): z-buffered forward warp and depth check. GPU only.

  1. pixel assignment, exact: the pixels with a finite d_pred_z are the pixels the points of d_warp_uv (vors_batch_residual_maps, pinned to the
     oracle bit for bit by test_gpu_residual_maps.py) land on by floor(u + 0.5), floor(v + 0.5) and the window test in float32; the first two
     counts are the numbers of finite and of landing (u, v);
  2. depth values against float64: Z' from vors_batch_get_points, the level intrinsics and the model, np.minimum.at over that assignment;
  3. d_pred_depth exact from the device's own d_pred_z (the numpy statement of to_depth of test_to_depth_host.py);
  4. the z-buffer on a constructed scene with two depth layers that overlap after the warp, and the pass fed its own depth map;
  5. the residual plane and the last two counts against float64 on the rendered pairs (with the rendered current depth);
  6. independence of the batch, the run, the subset of outputs, the model stride and the stream; no workspace; legal before any track;
  7. hostile models (NaN, everything behind the camera, a translation of 1e6 m) and the hostile scenes of tests/golden/adversarial;
  8. argument checks on a live handle.

Shapes: those of test_gpu_residual_maps.py, the smallest at which each source path differs — 120x160 / 4 levels in the three candidate modes
(dense: the quad source, two chunks at level 0), 240x320 / 5 levels coarse-to-fine (the list is cut), 122x162 / 3 levels dense (the
one-pixel source, odd halving). The pass does not depend on the handle's arithmetic; each shape runs on one. The DSO scenes are rendered
with the piecewise-constant texture, the only one the DSO selector picks points from (about 1950 per pair at level 0 here).

Tolerance of 2 and 5: the float32 chain to Z' (back-projection, quaternion rotation, translation) has about 15 roundings on magnitudes
<= 3 m, i.e. about 3e-6 m at Z' ~ 2; 1e-5 relative is that bound with a margin of about 7."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from test_gpu_first_principles import level_intrinsics
from test_oracle_first_principles import back_project, iso_to_mat, project
from test_to_depth_host import restated as to_depth_np
from depth_scales import requantise_tensor

N = 4
SCALE = 5000.0
TOL_M = 0.01
ARITHS = {"reference": V.ARITH_REFERENCE, "exact": V.ARITH_EXACT, "fused": V.ARITH_FUSED}
PARAMS = [((120, 160, 4), 0, "reference"), ((120, 160, 4), 1, "fused"), ((120, 160, 4), 2, "exact"), ((240, 320, 5), 0, "fused"),
          ((122, 162, 3), 1, "reference")]
F32 = np.float32
BLOCKY = 1 << 63   # seeds with the top bit set render the piecewise-constant texture: the DSO selector rejects the smooth one entirely


def scene_seed(seed, mode):
    """Every mode gets a scene it has points in (without the texture the DSO lists are empty and every check below would hold trivially)."""
    return seed | (BLOCKY if mode == V.CANDIDATES_DSO else 0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def landing(u, v, rows, cols):
    """The landing rule in float32 -> (mask, pixel index where the mask holds, 0 elsewhere). NaN and huge values fail the compares."""
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        fu, fv = np.floor(u + F32(0.5)), np.floor(v + F32(0.5))
        ok = (fu >= 0) & (fu < F32(cols)) & (fv >= 0) & (fv < F32(rows))
    q = np.where(ok, fv, 0).astype(np.int64) * cols + np.where(ok, fu, 0).astype(np.int64)
    return ok, q


def z64(b, p, lvl, k5, model):
    """xy and the float64 depth P'.z of every point of a level of a pair at a model."""
    xy, iz, _, _ = b.points(p, lvl)
    P = back_project(k5, xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64), 1.0 / iz.astype(np.float64))
    T = iso_to_mat(model)
    return xy, (P @ T[:3, :3].T + T[:3, 3])[:, 2]


def tracked_handle(cfg, kg, kd, cg, rows, cols):
    import torch
    n = kg.shape[0]
    b = V.Batch(cfg, n, rows, cols)
    poses = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    stats = V.stats_tensor(n)
    b.track_pairs(kg, kd, cg, poses, status, stats)
    torch.cuda.synchronize()
    return b, stats


def everything(b, lvl, d_models, cd):
    """Every output of the pass (the residual at level 0 only) + the warp field at the same models, read back once -> numpy arrays."""
    import torch
    out = b.reproject_depth(lvl, d_models, cur_depth=cd if lvl == 0 else None, tol_m=TOL_M, pred_z=True, pred_depth=True, residual=lvl == 0,
                            counts=True)
    warp = b.residual_maps(lvl, d_models, residuals=False, warp=True)["warp"]
    torch.cuda.synchronize()
    m = {k: t.cpu().numpy() for k, t in out.items()}
    m["warp"] = warp.cpu().numpy()
    return m


def assert_assignment_and_depth_map(m, p, rows, cols, what, z_positive=None, scale=SCALE):
    """Cases 1 and 3 for one pair. z_positive: per-pixel bool plane (True where the point's Z' > 0), None = everywhere. scale: the handle's
    depth scale."""
    uv, pz, cnt = m["warp"][p], m["pred_z"][p], m["counts"][p]
    assert pz.shape == (rows, cols) and pz.dtype == np.float32
    usable = ~np.isnan(uv[..., 0])
    ok, q = landing(uv[..., 0], uv[..., 1], rows, cols)
    if z_positive is not None:
        ok &= z_positive
    hit = np.zeros(rows * cols, bool)
    hit[q[ok]] = True
    assert not np.isnan(pz).any() and (pz > 0).all(), what
    assert (np.isfinite(pz).ravel() == hit).all(), what
    assert np.isposinf(pz.ravel()[~hit]).all(), what
    assert int(cnt[0]) == int(usable.sum()) and int(cnt[1]) == int(ok.sum()), (what, cnt, usable.sum(), ok.sum())
    # 3: the depth map from the device's own plane, IEEE division on both sides
    with np.errstate(divide="ignore"):
        want = np.where(np.isposinf(pz), np.uint16(0), to_depth_np(scale, F32(1.0) / pz))
    assert (m["pred_depth"][p].view(np.uint16) == want).all(), what
    return ok, q


class Scene:
    """4 rendered pairs (with the rendered current depth) tracked once; models [N, 2, 7]: each pair's lm_model and one moved by se3_exp(3e-3 u).
    scale, idepth_variance: the handle's; the rendered depth maps (quantised at SCALE) are re-quantised at another scale."""

    def __init__(self, shape, mode, arith, scale=SCALE, idepth_variance=1e-4):
        import torch
        self.rows, self.cols, self.L = shape
        self.mode, self.scale = mode, scale
        self.intr = V.scaled_intrinsics(self.rows, self.cols)
        self.kg, self.kd, self.cg, self.cd, _ = V.synth_render_pairs(scene_seed(0x5EEDE7A3, mode), N, self.rows, self.cols, self.intr, want_cur_depth=True)
        if scale != SCALE:
            self.kd, self.cd = requantise_tensor(self.kd, scale), requantise_tensor(self.cd, scale)
        cfg = V.Config(nb_levels=self.L, intrinsics=V.Intrinsics(self.intr[:2], self.intr[2:4], self.intr[4]), candidates_mode=mode,
                       depth_scale=scale, idepth_variance=idepth_variance, arithmetic=ARITHS[arith])
        self.b, self.stats = tracked_handle(cfg, self.kg, self.kd, self.cg, self.rows, self.cols)
        lm = V.decode_stats(self.stats)["lm_model"].copy()
        rng = np.random.default_rng(11)
        self.models = np.empty((N, 2, 7), np.float32)
        for p in range(N):
            self.models[p, 0] = lm[p]
            self.models[p, 1] = V.iso_mul(lm[p], V.se3_exp((rng.uniform(-1, 1, 6) * 3e-3).astype(np.float32)))
        self.d_models = [torch.from_numpy(np.ascontiguousarray(self.models[:, k])).cuda() for k in range(2)]
        self.cd_host = self.cd.cpu().numpy().view(np.uint16)
        self._out, self._z = {}, {}

    def shape(self, lvl):
        return self.rows >> lvl, self.cols >> lvl

    def out(self, lvl, k):
        if (lvl, k) not in self._out:   # read back once per (handle, level, model)
            self._out[lvl, k] = everything(self.b, lvl, self.d_models[k], self.cd)
        return self._out[lvl, k]

    def z(self, p, lvl, k):
        if (p, lvl, k) not in self._z:  # the float64 reference, computed once and shared
            self._z[p, lvl, k] = z64(self.b, p, lvl, level_intrinsics(self.intr, lvl), self.models[p, k])
        return self._z[p, lvl, k]


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: f"{p[0][1]}x{p[0][0]}L{p[0][2]}-{('c2f', 'dense', 'dso')[p[1]]}-{p[2]}")
def scene(request):
    return Scene(*request.param)


# ------------------------------------------------------------------------------------------------------------ 1, 2, 3
def check_pixel_assignment_depth_values_and_depth_map(sc, levels=None):
    for lvl in (0, sc.L - 1) if levels is None else levels:
        rows, cols = sc.shape(lvl)
        for k in range(2):
            m = sc.out(lvl, k)
            assert m["counts"].shape == (N, 4) and m["pred_depth"].shape == (N, rows, cols)
            for p in range(N):
                what = f"level {lvl} pair {p} model {k}"
                xy, Z = sc.z(p, lvl, k)
                assert len(xy) > 0 and (Z > 1.0).all(), what   # the rendered scenes sit at 1.6 - 2.6 m: every point is in front of the camera
                ok, q = assert_assignment_and_depth_map(m, p, rows, cols, what, scale=sc.scale)
                assert int(m["counts"][p][0]) == len(xy), what
                # 2: nearest float64 depth per pixel over the assignment of 1
                okp, qp = ok[xy[:, 1], xy[:, 0]], q[xy[:, 1], xy[:, 0]]
                want = np.full(rows * cols, np.inf)
                np.minimum.at(want, qp[okp], Z[okp])
                got = m["pred_z"][p].ravel().astype(np.float64)
                fin = np.isfinite(want)
                assert (np.isfinite(got) == fin).all(), what
                err = (np.abs(got[fin] - want[fin]) / want[fin]).max() if fin.any() else 0.0
                print(f"{what}: {len(xy)} points, {int(okp.sum())} land on {int(fin.sum())} pixels, max rel |z - z64| = {err:.3e}")
                assert err <= 1e-5, what


def test_pixel_assignment_depth_values_and_depth_map(scene):
    check_pixel_assignment_depth_values_and_depth_map(scene)


# ------------------------------------------------------------------------------------------------------------ 5
def check_residual_plane_and_counts_against_float64(sc):
    rows, cols = sc.shape(0)
    for k in range(2):
        m = sc.out(0, k)
        assert m["residual"].shape == (N, rows, cols)
        for p in range(N):
            what = f"pair {p} model {k}"
            xy, Z = sc.z(p, 0, k)
            uv = m["warp"][p]
            ok, q = landing(uv[..., 0], uv[..., 1], rows, cols)
            okp, qp = ok[xy[:, 1], xy[:, 0]], q[xy[:, 1], xy[:, 0]]
            d = sc.cd_host[p].ravel()[qp]
            has = okp & (d != 0)
            want = np.full((rows, cols), np.nan)
            want[xy[has, 1], xy[has, 0]] = Z[has] - d[has].astype(np.float64) / sc.scale
            res = m["residual"][p]
            assert (np.isfinite(res) == np.isfinite(want)).all() and np.isnan(res[~np.isfinite(want)]).all(), what
            bound = np.full((rows, cols), np.nan)
            bound[xy[has, 1], xy[has, 0]] = 1e-5 * Z[has]
            f = np.isfinite(want)
            excess = (np.abs(res[f].astype(np.float64) - want[f]) / bound[f]).max() if f.any() else 0.0
            print(f"{what}: {int(f.sum())} residuals, max |res - res64| / (1e-5 Z') = {excess:.3f}")
            assert excess <= 1.0, what
            cnt = m["counts"][p]
            assert int(cnt[2]) == int(f.sum()), what
            assert int(cnt[3]) == int((np.abs(res[f]) <= F32(TOL_M)).sum()), what
            assert 0 < int(cnt[3]) <= int(cnt[2]) <= int(cnt[1]) <= int(cnt[0]), (what, cnt)


def test_residual_plane_and_counts_against_float64(scene):
    check_residual_plane_and_counts_against_float64(scene)


# ------------------------------------------------------------------------------------------------------------ 6
def test_outputs_do_not_depend_on_the_batch_the_run_the_subset_the_stride_or_the_stream(scene):
    import torch
    sc, b = scene, scene.b
    before = b.workspace_bytes()
    for lvl in (0, sc.L - 1):
        cd = sc.cd if lvl == 0 else None
        kw_all = dict(cur_depth=cd, tol_m=TOL_M, pred_z=True, pred_depth=True, residual=lvl == 0, counts=True)
        names = ["pred_z", "pred_depth", "counts"] + (["residual"] if lvl == 0 else [])
        full = sc.out(lvl, 1)
        run1 = b.reproject_depth(lvl, sc.d_models[1], **kw_all)
        twice = run1["pred_z"] * 2.0   # a dependent op on the same stream, no host synchronisation in between
        run2 = b.reproject_depth(lvl, sc.d_models[1], **kw_all)
        subsets = [b.reproject_depth(lvl, sc.d_models[1], cur_depth=cd, tol_m=TOL_M, **kw)
                   for kw in (dict(), dict(pred_z=False, pred_depth=True), dict(pred_z=False, counts=True), dict(counts=True))]
        if lvl == 0:
            subsets.append(b.reproject_depth(lvl, sc.d_models[1], cur_depth=cd, tol_m=TOL_M, pred_z=False, residual=True))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = b.reproject_depth(lvl, sc.d_models[1], **kw_all)
        alone = {}
        for p in (0, 2, 3):
            first = sc.models[:p + 1, 0].copy()
            first[p] = sc.models[p, 1]
            alone[p] = b.reproject_depth(lvl, torch.from_numpy(first).cuda(), **{**kw_all, "cur_depth": cd[:p + 1].contiguous() if lvl == 0 else None})
        at_lm = b.reproject_depth(lvl, sc.stats, **kw_all)   # the stats tensor, struct stride
        torch.cuda.synchronize()
        for name in names:
            want = bits(full[name])
            for run in [run1, run2, other] + subsets:
                if name in run:
                    assert (bits(run[name].cpu().numpy()) == want).all(), (lvl, name)
            for p, t in alone.items():
                assert t[name].shape[0] == p + 1
                assert (bits(t[name].cpu().numpy()[p]) == want[p]).all(), (lvl, name, p)
            assert (bits(at_lm[name].cpu().numpy()) == bits(sc.out(lvl, 0)[name])).all(), (lvl, name)
        assert [sorted(s) for s in subsets[:4]] == [["pred_z"], ["pred_depth"], ["counts"], ["counts", "pred_z"]]
        assert (bits(twice.cpu().numpy()) == bits(full["pred_z"] * F32(2.0))).all(), lvl
    assert b.workspace_bytes() == before   # the pass has no workspace


def test_legal_directly_after_prepare_keyframes(scene):
    import torch
    sc = scene
    cfg = V.Config(nb_levels=sc.L, intrinsics=V.Intrinsics(sc.intr[:2], sc.intr[2:4], sc.intr[4]), candidates_mode=sc.mode, arithmetic=V.ARITH_FUSED)
    b = V.Batch(cfg, N, sc.rows, sc.cols)
    b.prepare_keyframes(sc.kg, sc.kd)
    before = b.workspace_bytes()
    for lvl in (0, sc.L - 1):
        out = b.reproject_depth(lvl, sc.d_models[1], cur_depth=sc.cd if lvl == 0 else None, tol_m=TOL_M, pred_z=True, pred_depth=True,
                                residual=lvl == 0, counts=True)
        torch.cuda.synchronize()
        for name, t in out.items():   # and what it gives is what the tracked handle gives (REFERENCE handles keep their lists in another order)
            assert (bits(t.cpu().numpy()) == bits(sc.out(lvl, 1)[name])).all(), (lvl, name)
    assert b.workspace_bytes() == before


# ------------------------------------------------------------------------------------------------------------ 4
def test_z_buffer_on_two_overlapping_depth_layers():
    import torch
    rows, cols, L, n = 60, 80, 3, 2
    intr = V.scaled_intrinsics(rows, cols)
    rng = np.random.default_rng(5)
    kg = torch.from_numpy(rng.integers(0, 256, (n, rows, cols), dtype=np.uint8)).cuda()
    kd_h = np.full((n, rows, cols), 15000, np.uint16)
    kd_h[:, :, 32:48] = 5000
    kd = torch.from_numpy(kd_h.view(np.int16)).cuda()
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=V.CANDIDATES_DENSE, arithmetic=V.ARITH_FUSED)
    b = V.Batch(cfg, n, rows, cols)
    b.prepare_keyframes(kg, kd)
    model = np.array([0.1, 0, 0, 0, 0, 0, 1], np.float32)
    d_models = torch.from_numpy(np.tile(model, (n, 1))).cuda()
    out = b.reproject_depth(0, d_models, pred_z=True, pred_depth=True, counts=True)
    fed = b.reproject_depth(0, d_models, cur_depth=out["pred_depth"], tol_m=1e-3, pred_z=True, residual=True, counts=True)
    torch.cuda.synchronize()
    # float64 side: every pixel is a point (dense, all depths known)
    k5 = level_intrinsics(intr, 0)
    ys, xs = np.mgrid[0:rows, 0:cols]
    Z = kd_h[0].astype(np.float64) / SCALE
    P = back_project(k5, xs.astype(np.float64), ys.astype(np.float64), Z) + np.array([0.1, 0.0, 0.0])
    u, v = project(k5, P)
    assert (np.abs((u + 0.5) - np.round(u + 0.5)) > 1e-3).all() and (np.abs((v + 0.5) - np.round(v + 0.5)) > 1e-3).all()  # no point near a pixel border: float32 assigns alike
    ok, q = landing(u, v, rows, cols)
    near = kd_h[0] == 5000
    has_near, has_far = np.zeros(rows * cols, bool), np.zeros(rows * cols, bool)
    has_near[q[ok & near]] = True
    has_far[q[ok & ~near]] = True
    both = has_near & has_far
    assert int(both.sum()) >= 100, int(both.sum())
    half_step = 0.5 / SCALE + 2e-5   # half a step of the u16 quantisation + the float32 roundings of Z'
    for p in range(n):
        pz = out["pred_z"][p].cpu().numpy().ravel()
        assert (np.isfinite(pz) == (has_near | has_far)).all()
        assert np.isposinf(pz).any()                                   # the disocclusion
        assert (np.abs(pz[both] - 1.0) <= 1e-5).all()                  # the near layer wins
        assert (np.abs(pz[has_far & ~has_near] - 3.0) <= 3e-5).all()
        cnt, cnt2 = out["counts"][p].cpu().numpy(), fed["counts"][p].cpu().numpy()
        assert cnt.tolist() == [rows * cols, int(ok.sum()), 0, 0]
        assert (bits(fed["pred_z"][p].cpu().numpy()) == bits(out["pred_z"][p].cpu().numpy())).all()
        res = fed["residual"][p].cpu().numpy()
        assert (np.isfinite(res) == ok).all()                          # every landing pixel holds a depth
        assert cnt2[2] == cnt2[1] == int(ok.sum())
        assert (res[ok] >= -half_step).all()
        winner = ok & (near | ~has_near[q].reshape(rows, cols))
        occluded = ok & ~near & has_near[q].reshape(rows, cols)
        assert int(occluded.sum()) >= 100
        assert (np.abs(res[winner]) <= half_step).all()
        assert (res[occluded] > 1.0).all()
        assert int(cnt2[3]) == int(np.sum(np.abs(res[ok]) <= F32(1e-3)))
        assert int(cnt2[3]) == int(winner.sum())


# ------------------------------------------------------------------------------------------------------------ 7
def hip_last_error():
    fn = V.lib().hipGetLastError   # resolved through the library's own dependency on the HIP runtime: the runtime the pass ran on
    fn.restype, fn.argtypes = C.c_int, []
    return fn()


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["c2f", "dense", "dso"])
def test_hostile_models(mode):
    import torch
    rows, cols, L, n = 120, 160, 4, 3
    intr = V.scaled_intrinsics(rows, cols)
    kg, kd, _, cd, _ = V.synth_render_pairs(scene_seed(0x5EEDE7A4, mode), n, rows, cols, intr, want_cur_depth=True)
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, arithmetic=V.ARITH_FUSED)
    b = V.Batch(cfg, n, rows, cols)
    b.prepare_keyframes(kg, kd)
    ident = torch.tensor([[0, 0, 0, 0, 0, 0, 1.0]] * n, dtype=torch.float32, device="cuda")
    hostile = {"nan": [np.nan] * 7, "behind": [0, 0, 0, 0, 1, 0, 0], "far": [1e6, 0, 0, 0, 0, 0, 1]}
    for lvl in (0, L - 1):
        cur = cd if lvl == 0 else None
        n_points = b.reproject_depth(lvl, ident, pred_z=False, counts=True)["counts"].cpu().numpy()[:, 0]
        assert (n_points > 0).all()
        for name, m7 in hostile.items():
            d_models = torch.tensor([m7] * n, dtype=torch.float32, device="cuda")
            out = b.reproject_depth(lvl, d_models, cur_depth=cur, tol_m=1e9, pred_z=True, pred_depth=True, residual=lvl == 0, counts=True)
            torch.cuda.synchronize()
            assert hip_last_error() == 0, (lvl, name)
            assert torch.isposinf(out["pred_z"]).all(), (lvl, name)
            assert (out["pred_depth"] == 0).all(), (lvl, name)
            if lvl == 0:
                assert torch.isnan(out["residual"]).all(), (lvl, name)
            cnt = out["counts"].cpu().numpy()
            assert (cnt[:, 0] == n_points).all() and (cnt[:, 1:] == 0).all(), (lvl, name, cnt)


@pytest.mark.parametrize("name", ["depth_step", "invalid_blobs", "large_motion", "rank_deficient"])
def test_hostile_scenes(name):
    import torch
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "adversarial", name + ".npz"))
    L, mode, rows, cols, intr = int(g["L"]), int(g["mode"]), int(g["rows"]), int(g["cols"]), tuple(float(x) for x in g["intr"])
    kg, cg = (torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("kf_gray", "cur_gray"))
    kd = torch.from_numpy(np.ascontiguousarray(g["kf_depth"]).view(np.int16)).cuda()
    n = kg.shape[0]
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, huber_delta=float(g["huber"]),
                   arithmetic=V.ARITH_FUSED)
    b, stats = tracked_handle(cfg, kg, kd, cg, rows, cols)
    models = V.decode_stats(stats)["lm_model"]
    for lvl in range(L):
        r, c = rows >> lvl, cols >> lvl
        m = everything(b, lvl, stats, kd)   # (the keyframe depth stands in for a current one: the point is that no index leaves a plane)
        assert hip_last_error() == 0
        for p in range(n):
            xy, Z = z64(b, p, lvl, level_intrinsics(intr, lvl), models[p])
            assert (np.abs(Z) > 1e-3).all()   # no point within rounding of the camera plane: float32 and float64 agree on the sign
            zpos = np.zeros((r, c), bool)
            zpos[xy[:, 1], xy[:, 0]] = Z > 0
            assert_assignment_and_depth_map(m, p, r, c, f"{name} level {lvl} pair {p}", z_positive=zpos)
            if lvl == 0:
                assert int(m["counts"][p][2]) == int(np.isfinite(m["residual"][p]).sum()) <= int(m["counts"][p][1])


# ------------------------------------------------------------------------------------------------------------ 8
def test_argument_validation_on_a_live_handle():
    import torch
    rows, cols, L = 120, 160, 4
    intr = V.scaled_intrinsics(rows, cols)
    kg, kd, cg, cd, _ = V.synth_render_pairs(0x5EEDE7A2, 4, rows, cols, intr, want_cur_depth=True)
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), arithmetic=V.ARITH_FUSED)
    b = V.Batch(cfg, 8, rows, cols)
    models = torch.zeros((8, 7), dtype=torch.float32, device="cuda")
    models[:, 6] = 1
    lib, s = V.lib(), b._stream()
    outs = dict(z=torch.zeros((8, rows, cols), dtype=torch.float32, device="cuda"), d=torch.zeros((8, rows, cols), dtype=torch.int16, device="cuda"),
                res=torch.zeros((8, rows, cols), dtype=torch.float32, device="cuda"), cnt=torch.full((8, 4), -7, dtype=torch.int32, device="cuda"))

    def call(n=4, lvl=0, stride=0, mdl=models, cur=cd, tol=0.01, stream=s, **kw):
        o = {**outs, **kw}
        return lib.vors_batch_reproject_depth(b._h, n, lvl, b._dp(mdl), stride, b._dp(cur), tol, b._dp(o["z"]), b._dp(o["d"]), b._dp(o["res"]),
                                              b._dp(o["cnt"]), stream)

    assert call() == -1 and b"prepare_keyframes" in lib.vors_last_error()
    b.prepare_keyframes(kg, kd)
    before = b.workspace_bytes()
    refused = [(dict(lvl=1), "level 0"), (dict(cur=None), "d_depth_residual needs d_cur_depth"), (dict(tol=-1e-3), "tol_m"), (dict(tol=float("nan")), "tol_m"),
               (dict(z=None, d=None, res=None, cnt=None), "every output"), (dict(lvl=L, cur=None, res=None), "level"), (dict(lvl=-1, cur=None, res=None), "level"),
               (dict(n=0), "n_pairs"), (dict(n=5), "n_pairs"), (dict(z=None), "d_pred_depth needs d_pred_z"), (dict(mdl=None), "d_models"),
               (dict(stride=30), "stride"), (dict(stride=24), "stride")]
    for bad, word in refused:
        assert call(**bad) == -1, bad
        assert word.encode() in lib.vors_last_error(), (bad, lib.vors_last_error())
    if torch.cuda.device_count() > 1:   # a stream of another device
        with torch.cuda.device(1):
            foreign = torch.cuda.Stream()
        assert call(stream=C.c_void_p(foreign.cuda_stream)) == -1 and b"stream" in lib.vors_last_error()
    torch.cuda.synchronize()
    assert (outs["cnt"] == -7).all() and (outs["z"] == 0).all()   # the refusals enqueued nothing
    assert call() == 0
    assert call(cur=None, res=None) == 0 and call(z=None, d=None) == 0 and call(lvl=L - 1, cur=None, res=None) == 0
    torch.cuda.synchronize()
    cnt = outs["cnt"].cpu().numpy()
    assert (cnt[:4, 0] > 0).all() and (cnt[4:] == -7).all()      # the handle is usable, and only the 4 pairs asked for were written
    assert b.workspace_bytes() == before
    with pytest.raises(V.VorsError):
        b.reproject_depth(0, models[:4], pred_z=False)
    with pytest.raises(V.VorsError):
        b.reproject_depth(0, torch.zeros((4, 2, 7), dtype=torch.float32, device="cuda"))
    with pytest.raises(V.VorsError):
        b.reproject_depth(0, models[:4], cur_depth=cd[:, :60].contiguous())
