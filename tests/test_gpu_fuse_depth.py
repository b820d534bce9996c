"""Depth fusion of a prepared batch (vors_batch_fuse_depth): keyed z-buffer splat and per-pixel merge. GPU only.

  1. keys against the existing pass: zkey >> 32 has the bits of vors_batch_reproject_depth's d_pred_z, empty exactly where that is +inf; the
     source index is a usable point whose (u, v) of vors_batch_residual_maps lands at the pixel and whose float64 Z' is within 1e-5
     relative of d_pred_z (the bound test_gpu_reproject_depth.py derives);
  2. the tie-break on a constructed scene where every Z' is the same float: the smallest source index wins;
  3. depth, weight and counts exact against the host entry (vors_fuse_depth_pixels, pinned to the rule table by test_fuse_depth_host.py) fed
     the device's own key plane; filled pixels carry the bits of d_pred_depth;
  4. two depth layers that overlap after the warp: fed its own depth map, and fed a constant plane;
  5. weights: zero bytes remove points, weights saturate, fill_min_weight gates the fill;
  6. the recursion: eight noisy measurements of a constant depth fused one after another;
  7. independence of the batch, the run, the subset of outputs, the model stride and the stream; no workspace; legal before any track;
  8. hostile models and the hostile scenes of tests/golden/adversarial;
  9. argument checks on a live handle.

Shapes: those of test_gpu_reproject_depth.py (its Scene is reused: 120x160 / 4 levels in the three candidate modes, 240x320 / 5 levels
coarse-to-fine, 122x162 / 3 levels dense), 60x80 for the constructed scenes."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from test_gpu_first_principles import level_intrinsics
from test_gpu_reproject_depth import N, PARAMS, SCALE, TOL_M, Scene, bits, hip_last_error, landing, scene_seed, tracked_handle
from test_oracle_first_principles import back_project, project

F32 = np.float32
EMPTY = np.uint64(V.ZKEY_EMPTY)
LOW = np.uint64(0xFFFFFFFF)
AGREE, FRONT, BEHIND, MEASURED, FILLED, NOTHING = range(6)
IDENT = [0, 0, 0, 0, 0, 0, 1.0]


def host(out):
    """A fuse_depth result read back: the payloads as what they are (uint64 keys, uint16 depths)."""
    m = {k: t.cpu().numpy() for k, t in out.items()}
    if "zkey" in m:
        m["zkey"] = m["zkey"].view(np.uint64)
    if "depth" in m:
        m["depth"] = m["depth"].view(np.uint16)
    return m


def fuse_all(b, models, cd, tol=TOL_M, **kw):
    import torch
    out = b.fuse_depth(models, cd, tol, depth=True, weight=True, zkey=True, counts=True, **kw)
    torch.cuda.synchronize()
    return host(out)


def assert_exact_against_host_entry(m, cd_host, w_host, tol, max_weight=255, fill=0, what="", scale=SCALE):
    """Case 3 for a whole result: every pair's maps and counters from the device's own keys."""
    n, rows, cols = m["zkey"].shape
    for p in range(n):
        depth, weight, counts = V.fuse_depth_pixels(scale, tol, m["zkey"][p], cd_host[p], None if w_host is None else w_host[p], max_weight, fill)
        assert (m["depth"][p] == depth).all() and (m["weight"][p] == weight).all(), (what, p)
        assert m["counts"][p].tolist() == counts.tolist() and int(m["counts"][p].sum()) == rows * cols, (what, p, m["counts"][p], counts)
        assert ((m["depth"][p] == 0) == (m["weight"][p] == 0)).all(), (what, p)


def config(intr, L, mode, arith=None):
    return V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode,
                    arithmetic=V.ARITH_FUSED if arith is None else arith)


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: f"{p[0][1]}x{p[0][0]}L{p[0][2]}-{('c2f', 'dense', 'dso')[p[1]]}-{p[2]}")
def scene(request):
    return with_weights_and_holes(Scene(*request.param))


def with_weights_and_holes(sc):
    """A Scene + a keyframe weight plane with zeros in it and a measured depth with holes."""
    rng = np.random.default_rng(17)
    import torch
    w = rng.integers(1, 9, (N, sc.rows, sc.cols)).astype(np.uint8)
    w[rng.random(w.shape) < 0.3] = 0
    sc.w_host, sc.w = w, torch.from_numpy(w).cuda()
    holes = sc.cd_host.copy()
    holes[:, sc.rows // 3: sc.rows // 2, sc.cols // 4: sc.cols // 2] = 0
    holes[rng.random(holes.shape) < 0.1] = 0
    sc.holes_host, sc.holes = holes, torch.from_numpy(holes.view(np.int16)).cuda()
    sc._fused = {}
    return sc


def fused(sc, k):
    if k not in sc._fused:   # the plain run at model k, read back once
        sc._fused[k] = fuse_all(sc.b, sc.d_models[k], sc.cd)
    return sc._fused[k]


# ------------------------------------------------------------------------------------------------------------ 1
def test_keys_against_the_reprojection_pass(scene):
    sc = scene
    rows, cols = sc.shape(0)
    for k in range(2):
        m, key = sc.out(0, k), fused(sc, k)["zkey"]
        assert key.shape == (N, rows, cols)
        for p in range(N):
            what = f"pair {p} model {k}"
            pz = m["pred_z"][p]
            empty = key[p] == EMPTY
            assert (empty == np.isposinf(pz)).all() and not empty.all(), what
            assert ((key[p] >> np.uint64(32)).astype(np.uint32)[~empty] == bits(pz)[~empty]).all(), what
            src = (key[p] & LOW).astype(np.int64)[~empty]
            assert (src < rows * cols).all(), what
            uv = m["warp"][p].reshape(rows * cols, 2)[src]
            assert not np.isnan(uv).any(), what                       # a usable point ...
            ok, q = landing(uv[:, 0], uv[:, 1], rows, cols)
            assert ok.all() and (q == np.nonzero(~empty.ravel())[0]).all(), what   # ... that lands at this pixel ...
            xy, Z = sc.z(p, 0, k)
            zplane = np.full(rows * cols, np.nan)
            zplane[xy[:, 1].astype(np.int64) * cols + xy[:, 0]] = Z
            err = np.abs(zplane[src] - pz[~empty].astype(np.float64)) / zplane[src]
            print(f"{what}: {int((~empty).sum())} keys, max rel |z64(src) - pred_z| = {err.max():.3e}")
            assert (err <= 1e-5).all(), what                         # ... and is the nearest one


# ------------------------------------------------------------------------------------------------------------ 2
def test_tie_break_smallest_source_index():
    import torch
    rows, cols, L, n = 60, 80, 3, 2
    intr = V.scaled_intrinsics(rows, cols)
    rng = np.random.default_rng(6)
    kg = torch.from_numpy(rng.integers(0, 256, (n, rows, cols), dtype=np.uint8)).cuda()
    kd = torch.full((n, rows, cols), 5000, dtype=torch.int16, device="cuda")
    b = V.Batch(config(intr, L, V.CANDIDATES_DENSE), n, rows, cols)
    b.prepare_keyframes(kg, kd)
    model = np.array([0, 0, 0.5, 0, 0, 0, 1], np.float32)
    m = fuse_all(b, torch.from_numpy(np.tile(model, (n, 1))).cuda(), kd)
    # float64 side: every pixel is a point at Z' = 1.5; the image shrinks to two thirds around the principal point
    k5 = level_intrinsics(intr, 0)
    ys, xs = np.mgrid[0:rows, 0:cols]
    P = back_project(k5, xs.astype(np.float64), ys.astype(np.float64), np.full((rows, cols), 1.0)) + np.array([0.0, 0.0, 0.5])
    u, v = project(k5, P)
    assert (np.abs((u + 0.5) - np.round(u + 0.5)) > 1e-3).all() and (np.abs((v + 0.5) - np.round(v + 0.5)) > 1e-3).all()  # float32 assigns alike
    ok, q = landing(u, v, rows, cols)
    assert ok.all()
    hits = np.bincount(q.ravel(), minlength=rows * cols)
    assert int((hits >= 2).sum()) >= 100, int((hits >= 2).sum())
    first = np.full(rows * cols, -1, np.int64)
    first[q.ravel()[::-1]] = np.arange(rows * cols)[::-1]     # assigned in descending order: the smallest landing index stays
    for p in range(n):
        key = m["zkey"][p].ravel()
        assert ((key == EMPTY) == (hits == 0)).all()
        land = hits > 0
        assert ((key[land] >> np.uint64(32)) == np.uint64(F32(1.5).view(np.uint32))).all()   # every Z' is the same float
        assert ((key[land] & LOW).astype(np.int64) == first[land]).all()


# ------------------------------------------------------------------------------------------------------------ 3
def test_merge_exact_against_the_host_entry(scene):
    check_merge_exact_against_the_host_entry(scene)


def check_merge_exact_against_the_host_entry(sc):
    for k in range(2):
        plain = fused(sc, k)
        assert_exact_against_host_entry(plain, sc.cd_host, None, TOL_M, what=f"model {k}", scale=sc.scale)
        assert (plain["counts"][:, AGREE] > 0).all()
        filled = fuse_all(sc.b, sc.d_models[k], sc.holes, fill_min_weight=1)
        assert_exact_against_host_entry(filled, sc.holes_host, None, TOL_M, 255, 1, what=f"model {k}, holes", scale=sc.scale)
        assert (filled["zkey"] == plain["zkey"]).all()            # the splat does not read the measurement
        at = (filled["zkey"] != EMPTY) & (sc.holes_host == 0)
        assert (filled["counts"][:, FILLED] == at.sum(axis=(1, 2))).all() and at.any()
        assert (filled["depth"][at] == sc.out(0, k)["pred_depth"].view(np.uint16)[at]).all() and (filled["weight"][at] == 1).all()
        weighted = fuse_all(sc.b, sc.d_models[k], sc.holes, kf_weight=sc.w, max_weight=6, fill_min_weight=4)
        assert_exact_against_host_entry(weighted, sc.holes_host, sc.w_host, TOL_M, 6, 4, what=f"model {k}, holes, weights", scale=sc.scale)
        assert (weighted["counts"][:, [AGREE, FILLED]] > 0).all() and weighted["weight"].max() == 8   # (a filled pixel keeps its weight)


# ------------------------------------------------------------------------------------------------------------ 4
def test_two_overlapping_depth_layers():
    import torch
    rows, cols, L, n = 60, 80, 3, 2
    intr = V.scaled_intrinsics(rows, cols)
    rng = np.random.default_rng(5)
    kg = torch.from_numpy(rng.integers(0, 256, (n, rows, cols), dtype=np.uint8)).cuda()
    kd_h = np.full((n, rows, cols), 15000, np.uint16)
    kd_h[:, :, 32:48] = 5000
    kd = torch.from_numpy(kd_h.view(np.int16)).cuda()
    b = V.Batch(config(intr, L, V.CANDIDATES_DENSE), n, rows, cols)
    b.prepare_keyframes(kg, kd)
    d_models = torch.from_numpy(np.tile(np.array([0.1, 0, 0, 0, 0, 0, 1], np.float32), (n, 1))).cuda()
    own = b.reproject_depth(0, d_models, pred_z=True, pred_depth=True)["pred_depth"]
    fed = fuse_all(b, d_models, own, tol=1e-3)
    plane = torch.full((n, rows, cols), 15000, dtype=torch.int16, device="cuda")
    flat = fuse_all(b, d_models, plane, tol=1e-3)
    # float64 side, as in test_gpu_reproject_depth.py case 4
    k5 = level_intrinsics(intr, 0)
    ys, xs = np.mgrid[0:rows, 0:cols]
    P = back_project(k5, xs.astype(np.float64), ys.astype(np.float64), kd_h[0].astype(np.float64) / SCALE) + np.array([0.1, 0.0, 0.0])
    u, v = project(k5, P)
    ok, q = landing(u, v, rows, cols)
    near = kd_h[0] == 5000
    has_near, has_far = np.zeros(rows * cols, bool), np.zeros(rows * cols, bool)
    has_near[q[ok & near]] = True
    has_far[q[ok & ~near]] = True
    lands = (has_near | has_far).reshape(rows, cols)
    has_near, has_far = has_near.reshape(rows, cols), has_far.reshape(rows, cols)
    assert int((has_near & has_far).sum()) >= 100 and int((~lands).sum()) > 0
    own_h = own.cpu().numpy().view(np.uint16)
    for p in range(n):
        assert ((fed["zkey"][p] != EMPTY) == lands).all()
        assert (kd_h[p].ravel()[(fed["zkey"][p][has_near] & LOW).astype(np.int64)] == 5000).all()   # the near layer wins
        # its own depth map: every landing pixel agrees (half a quantisation step is 1e-4 m), the disocclusion is empty
        assert (fed["weight"][p][lands] == 2).all() and (fed["depth"][p][lands] == own_h[p][lands]).all()
        assert (fed["weight"][p][~lands] == 0).all() and (fed["depth"][p][~lands] == 0).all()
        assert fed["counts"][p].tolist() == [int(lands.sum()), 0, 0, 0, 0, int((~lands).sum())]
        # a constant 3 m plane: the near layer is in front of it, the far-only pixels agree, the disocclusion is measured only
        assert (flat["depth"][p][has_near] == 15000).all() and (flat["weight"][p][has_near] == 1).all()
        far_only = has_far & ~has_near
        assert (flat["weight"][p][far_only] == 2).all() and (np.abs(flat["depth"][p][far_only].astype(int) - 15000) <= 1).all()
        assert (flat["depth"][p][~lands] == 15000).all() and (flat["weight"][p][~lands] == 1).all()
        assert flat["counts"][p].tolist() == [int(far_only.sum()), int(has_near.sum()), 0, int((~lands).sum()), 0, 0]
    assert_exact_against_host_entry(fed, own_h, None, 1e-3, what="own depth map")
    assert_exact_against_host_entry(flat, np.full((n, rows, cols), 15000, np.uint16), None, 1e-3, what="constant plane")


# ------------------------------------------------------------------------------------------------------------ 5
def test_weights_remove_points_saturate_and_gate_the_fill():
    import torch
    rows, cols, L, n = 60, 80, 3, 2
    intr = V.scaled_intrinsics(rows, cols)
    kg, kd, _, _, _ = V.synth_render_pairs(0x5EEDE7A5, n, rows, cols, intr, want_cur_depth=True)
    kd_h = kd.cpu().numpy().view(np.uint16)
    rng = np.random.default_rng(23)
    w_h = rng.integers(1, 6, (n, rows, cols)).astype(np.uint8)
    w_h[rng.random(w_h.shape) < 0.4] = 0
    w = torch.from_numpy(w_h).cuda()
    models = torch.tensor([[0.02, -0.01, 0.01, 0, 0, 0, 1.0]] * n, dtype=torch.float32, device="cuda")
    b = V.Batch(config(intr, L, V.CANDIDATES_DENSE), n, rows, cols)
    b.prepare_keyframes(kg, kd)
    cd = b.reproject_depth(0, models, pred_z=True, pred_depth=True)["pred_depth"]   # the measurement: the unweighted prediction itself
    cd_h = cd.cpu().numpy().view(np.uint16)
    m = fuse_all(b, models, cd, kf_weight=w, max_weight=4, fill_min_weight=0)
    full = fuse_all(b, models, cd)
    # zero bytes remove points: no key names one, and the keys are those of a scene where those depths are unknown
    for p in range(n):
        src = (m["zkey"][p][m["zkey"][p] != EMPTY] & LOW).astype(np.int64)
        assert len(src) > 0 and (w_h[p].ravel()[src] != 0).all()
    assert (m["zkey"] != full["zkey"]).any()
    masked = kd_h.copy()
    masked[w_h == 0] = 0
    kd2 = torch.from_numpy(masked.view(np.int16)).cuda()
    b2 = V.Batch(config(intr, L, V.CANDIDATES_DENSE), n, rows, cols)
    b2.prepare_keyframes(kg, kd2)
    assert (fuse_all(b2, models, cd)["zkey"] == m["zkey"]).all()
    # saturation: an agreeing pixel gets min(wk + 1, max_weight)
    for p in range(n):
        has = m["zkey"][p] != EMPTY
        wk = np.where(has, w_h[p].ravel()[(m["zkey"][p] & LOW).astype(np.int64) * has], 0)
        agree = has & (m["weight"][p] > 1)
        assert agree.sum() > 100 and (m["weight"][p][agree] == np.minimum(wk[agree] + 1, 4)).all() and (wk[agree] + 1 > 4).any()
    assert_exact_against_host_entry(m, cd_h, w_h, TOL_M, 4, 0, what="weights")
    # the fill gate on a frame without any measurement: filled exactly where the winner's weight reaches fill_min_weight
    nothing = torch.zeros_like(cd)
    for fill in (0, 1, 3, 5, 6):
        f = fuse_all(b, models, nothing, kf_weight=w, fill_min_weight=fill)
        assert (f["zkey"] == m["zkey"]).all()
        for p in range(n):
            has = f["zkey"][p] != EMPTY
            wk = np.where(has, w_h[p].ravel()[(f["zkey"][p] & LOW).astype(np.int64) * has], 0)
            want = has & (wk >= fill) & (fill > 0)
            assert ((f["weight"][p] != 0) == want).all() and (f["weight"][p][want] == wk[want]).all(), fill
            assert f["counts"][p].tolist() == [0, 0, 0, 0, int(want.sum()), rows * cols - int(want.sum())], fill
        assert (f["counts"][:, FILLED] > 0).all() == (0 < fill <= 5)


# ------------------------------------------------------------------------------------------------------------ 6
def test_recursion_filters_a_noisy_depth():
    import torch
    rows, cols, L, n, steps, truth, sigma, tol = 60, 80, 3, 2, 8, 10000, 20.0, 0.05
    intr = V.scaled_intrinsics(rows, cols)
    rng = np.random.default_rng(31)
    kg = torch.from_numpy(rng.integers(0, 256, (n, rows, cols), dtype=np.uint8)).cuda()
    meas = np.rint(truth + rng.normal(0, sigma, (steps, n, rows, cols))).astype(np.uint16)
    ident = torch.tensor([IDENT] * n, dtype=torch.float32, device="cuda")
    b = V.Batch(config(intr, L, V.CANDIDATES_DENSE), n, rows, cols)
    depth = torch.from_numpy(meas[0].view(np.int16)).cuda()          # the first measurement is the first keyframe, weight 1
    weight = torch.ones((n, rows, cols), dtype=torch.uint8, device="cuda")
    for i in range(1, steps):
        b.prepare_keyframes(kg, depth)
        m = fuse_all(b, ident, torch.from_numpy(meas[i].view(np.int16)).cuda(), tol=tol, kf_weight=weight)
        assert_exact_against_host_entry(m, meas[i], weight.cpu().numpy(), tol, what=f"step {i}")
        assert (m["counts"] == np.array([rows * cols, 0, 0, 0, 0, 0])).all(), (i, m["counts"])
        assert (m["weight"] == i + 1).all()
        assert ((m["zkey"] & LOW).astype(np.int64) == np.arange(rows * cols).reshape(rows, cols)).all()   # identity: every pixel is its own source
        depth, weight = torch.from_numpy(m["depth"].view(np.int16)).cuda(), torch.from_numpy(m["weight"]).cuda()
    final = depth.cpu().numpy().view(np.uint16).astype(np.float64)
    rms = np.sqrt(np.mean((final - truth) ** 2))
    rms_one = np.sqrt(np.mean((meas[-1].astype(np.float64) - truth) ** 2))
    print(f"rms of one measurement {rms_one:.2f}, of {steps} fused {rms:.2f} depth units (ratio {rms / rms_one:.3f}, 1 / sqrt(8) = 0.354)")
    assert (weight == steps).all() and rms < 0.5 * rms_one


# ------------------------------------------------------------------------------------------------------------ 7
def test_outputs_do_not_depend_on_the_batch_the_run_the_subset_the_stride_or_the_stream(scene):
    import torch
    sc, b = scene, scene.b
    before = b.workspace_bytes()
    names = ["depth", "weight", "zkey", "counts"]
    kw = dict(kf_weight=sc.w, max_weight=6, fill_min_weight=2)
    full = fuse_all(b, sc.d_models[1], sc.holes, **kw)
    run1 = b.fuse_depth(sc.d_models[1], sc.holes, TOL_M, depth=True, weight=True, zkey=True, counts=True, **kw)
    shifted = run1["depth"] + 1   # a dependent op on the same stream, no host synchronisation in between
    run2 = b.fuse_depth(sc.d_models[1], sc.holes, TOL_M, depth=True, weight=True, zkey=True, counts=True, **kw)
    subsets = [b.fuse_depth(sc.d_models[1], sc.holes, TOL_M, **{**dict(depth=False, weight=False), **want, **kw})
               for want in (dict(depth=True), dict(weight=True), dict(zkey=True), dict(counts=True), dict(depth=True, counts=True))]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = b.fuse_depth(sc.d_models[1], sc.holes, TOL_M, depth=True, weight=True, zkey=True, counts=True, **kw)
    alone = {}
    for p in (0, 2, 3):
        first = sc.models[:p + 1, 0].copy()
        first[p] = sc.models[p, 1]
        alone[p] = b.fuse_depth(torch.from_numpy(first).cuda(), sc.holes[:p + 1].contiguous(), TOL_M, depth=True, weight=True, zkey=True, counts=True,
                                **{**kw, "kf_weight": sc.w[:p + 1].contiguous()})
    at_lm = b.fuse_depth(sc.stats, sc.holes, TOL_M, depth=True, weight=True, zkey=True, counts=True, **kw)   # the stats tensor, struct stride
    at_lm_plain = fuse_all(b, sc.d_models[0], sc.holes, **kw)
    torch.cuda.synchronize()
    runs = [host(r) for r in [run1, run2, other] + subsets]
    for name in names:
        for run in runs:
            if name in run:
                assert (run[name] == full[name]).all(), name
        for p, t in alone.items():
            assert t[name].shape[0] == p + 1 and (host(t)[name][p] == full[name][p]).all(), (name, p)
        assert (host(at_lm)[name] == at_lm_plain[name]).all(), name
    assert [sorted(s) for s in subsets] == [["depth"], ["weight"], ["zkey"], ["counts"], ["counts", "depth"]]
    assert (shifted.cpu().numpy().view(np.uint16) == full["depth"] + np.uint16(1)).all()
    assert b.workspace_bytes() == before   # the pass has no workspace


def test_legal_directly_after_prepare_keyframes(scene):
    sc = scene
    b = V.Batch(config(sc.intr, sc.L, sc.mode), N, sc.rows, sc.cols)
    b.prepare_keyframes(sc.kg, sc.kd)
    before = b.workspace_bytes()
    m = fuse_all(b, sc.d_models[1], sc.cd)
    for name, a in m.items():   # and what it gives is what the tracked handle gives
        assert (a == fused(sc, 1)[name]).all(), name
    assert b.workspace_bytes() == before


# ------------------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["c2f", "dense", "dso"])
def test_hostile_models(mode):
    import torch
    rows, cols, L, n = 120, 160, 4, 3
    intr = V.scaled_intrinsics(rows, cols)
    kg, kd, _, cd, _ = V.synth_render_pairs(scene_seed(0x5EEDE7A4, mode), n, rows, cols, intr, want_cur_depth=True)
    cd_h = cd.cpu().numpy().view(np.uint16).copy()
    cd_h[:, 10:20, 10:40] = 0
    cd = torch.from_numpy(cd_h.view(np.int16)).cuda()
    b = V.Batch(config(intr, L, mode), n, rows, cols)
    b.prepare_keyframes(kg, kd)
    sane = fuse_all(b, torch.tensor([IDENT] * n, dtype=torch.float32, device="cuda"), cd, fill_min_weight=1)
    assert (sane["zkey"] != EMPTY).any(axis=(1, 2)).all()
    hostile = {"nan": [np.nan] * 7, "behind": [0, 0, 0, 0, 1, 0, 0], "far": [1e6, 0, 0, 0, 0, 0, 1]}
    for name, m7 in hostile.items():
        m = fuse_all(b, torch.tensor([m7] * n, dtype=torch.float32, device="cuda"), cd, tol=1e9, fill_min_weight=1)
        assert hip_last_error() == 0, name
        assert (m["zkey"] == EMPTY).all(), name
        assert (m["depth"] == cd_h).all() and (m["weight"] == (cd_h != 0)).all(), name
        assert (m["counts"][:, [AGREE, FRONT, BEHIND, FILLED]] == 0).all(), (name, m["counts"])
        assert (m["counts"][:, MEASURED] == (cd_h != 0).sum(axis=(1, 2))).all() and (m["counts"].sum(axis=1) == rows * cols).all(), name


@pytest.mark.parametrize("name", ["depth_step", "invalid_blobs", "large_motion", "rank_deficient"])
def test_hostile_scenes(name):
    import torch
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "adversarial", name + ".npz"))
    L, mode, rows, cols, intr = int(g["L"]), int(g["mode"]), int(g["rows"]), int(g["cols"]), tuple(float(x) for x in g["intr"])
    kg, cg = (torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("kf_gray", "cur_gray"))
    kd_h = np.ascontiguousarray(g["kf_depth"])
    kd = torch.from_numpy(kd_h.view(np.int16)).cuda()
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, huber_delta=float(g["huber"]),
                   arithmetic=V.ARITH_FUSED)
    b, stats = tracked_handle(cfg, kg, kd, cg, rows, cols)
    m = fuse_all(b, stats, kd, fill_min_weight=1)   # (the keyframe depth stands in for a current one: the point is that no index leaves a plane)
    assert hip_last_error() == 0
    assert (m["counts"].sum(axis=1) == rows * cols).all()
    src = (m["zkey"][m["zkey"] != EMPTY] & LOW).astype(np.int64)
    assert (src < rows * cols).all()
    assert_exact_against_host_entry(m, kd_h.view(np.uint16), None, TOL_M, 255, 1, what=name)


# ------------------------------------------------------------------------------------------------------------ 9
def test_argument_validation_on_a_live_handle():
    import torch
    rows, cols, L = 120, 160, 4
    intr = V.scaled_intrinsics(rows, cols)
    kg, kd, cg, cd, _ = V.synth_render_pairs(0x5EEDE7A2, 4, rows, cols, intr, want_cur_depth=True)
    b = V.Batch(config(intr, L, V.CANDIDATES_COARSE_TO_FINE), 8, rows, cols)
    models = torch.zeros((8, 7), dtype=torch.float32, device="cuda")
    models[:, 6] = 1
    lib, s = V.lib(), b._stream()
    key = torch.full((8 * rows * cols + 1,), 5, dtype=torch.int64, device="cuda")
    outs = dict(d=torch.full((8, rows, cols), 7, dtype=torch.int16, device="cuda"), w=torch.full((8, rows, cols), 7, dtype=torch.uint8, device="cuda"),
                cnt=torch.full((8, 6), -7, dtype=torch.int32, device="cuda"))
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(n=4, stride=0, mdl=models, cur=cd, tol=0.01, kw=None, maxw=255, fill=0, zkey=ptr(key), stream=s, **kws):
        o = {**outs, **kws}
        return lib.vors_batch_fuse_depth(b._h, n, ptr(mdl), stride, ptr(cur), tol, ptr(kw), maxw, fill, zkey, ptr(o["d"]), ptr(o["w"]), ptr(o["cnt"]), stream)

    assert call() == -1 and b"prepare_keyframes" in lib.vors_last_error()
    assert lib.vors_batch_fuse_depth(None, 4, ptr(models), 0, ptr(cd), 0.01, None, 255, 0, ptr(key), None, None, None, s) == -1
    b.prepare_keyframes(kg, kd)
    before = b.workspace_bytes()
    refused = [(dict(mdl=None), "d_models"), (dict(cur=None), "d_cur_depth"), (dict(zkey=None), "d_zkey"),
               (dict(zkey=C.c_void_p(key.data_ptr() + 4)), "aligned"), (dict(tol=-1e-3), "tol_m"), (dict(tol=float("nan")), "tol_m"),
               (dict(maxw=0), "max_weight"), (dict(maxw=256), "max_weight"), (dict(fill=-1), "fill_min_weight"), (dict(fill=256), "fill_min_weight"),
               (dict(stride=30), "stride"), (dict(stride=24), "stride"), (dict(n=0), "n_pairs"), (dict(n=5), "n_pairs")]
    for bad, word in refused:
        assert call(**bad) == -1, bad
        assert word.encode() in lib.vors_last_error(), (bad, lib.vors_last_error())
    if torch.cuda.device_count() > 1:   # a stream of another device
        with torch.cuda.device(1):
            foreign = torch.cuda.Stream()
        assert call(stream=C.c_void_p(foreign.cuda_stream)) == -1 and b"stream" in lib.vors_last_error()
    torch.cuda.synchronize()
    assert (key == 5).all() and (outs["d"] == 7).all() and (outs["w"] == 7).all() and (outs["cnt"] == -7).all()   # the refusals enqueued nothing
    assert call(d=None, w=None, cnt=None) == 0   # the key plane alone is legal: the pass is then only the splat
    torch.cuda.synchronize()
    assert (key[:4 * rows * cols] != 5).all() and (key[4 * rows * cols:] == 5).all() and (outs["d"] == 7).all() and (outs["cnt"] == -7).all()
    assert call(zkey=C.c_void_p(key.data_ptr() + 8)) == 0   # 8-byte aligned is enough (the merge then takes its one-pixel path)
    torch.cuda.synchronize()
    cnt = outs["cnt"].cpu().numpy()
    assert (cnt[:4].sum(axis=1) == rows * cols).all() and (cnt[4:] == -7).all()   # the handle is usable, and only the 4 pairs asked for were written
    assert (outs["d"][4:] == 7).all() and (outs["w"][4:] == 7).all() and (key[0] != 5)
    narrow = {k: t.cpu().numpy().copy() for k, t in outs.items()}
    wide = b.fuse_depth(models[:4], cd, 0.01, counts=True)
    torch.cuda.synchronize()
    assert (wide["depth"].cpu().numpy() == narrow["d"][:4]).all() and (wide["weight"].cpu().numpy() == narrow["w"][:4]).all()
    assert (wide["counts"].cpu().numpy() == narrow["cnt"][:4]).all()   # both paths of the merge kernel give the same maps
    assert b.workspace_bytes() == before
    with pytest.raises(V.VorsError):
        b.fuse_depth(models[:4], cd, 0.01, depth=False, weight=False)
    with pytest.raises(V.VorsError):
        b.fuse_depth(torch.zeros((4, 2, 7), dtype=torch.float32, device="cuda"), cd, 0.01)
    with pytest.raises(V.VorsError):
        b.fuse_depth(models[:4], cd[:, :60].contiguous(), 0.01)
    with pytest.raises(V.VorsError):
        b.fuse_depth(models[:4], cd, 0.01, kf_weight=torch.ones((4, rows, cols), dtype=torch.int16, device="cuda"))
