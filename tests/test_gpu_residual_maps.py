"""Residual maps, warp fields and residual histograms of a prepared batch (vors_batch_residual_maps). GPU only.

  1. against the oracle, bit for bit (levels 0 and L - 1): the pixels with a finite warp are oracle.Tracker's points, the residual at each has
     the bits of oracle.lm_eval's (or both are NaN), everything else is NaN — on handles of every arithmetic, with Huber on or off;
  2. self-consistency, exact (every level): finite residual <=> the strict inside test recomputed in float32 from the returned (u, v); the
     histogram is numpy's bincount of the map; its sum is n_inside of vors_batch_eval_pairs (EXACT); sum r^2 against that evaluation's
     energy (Huber off); the scale is the host helper's, bit for bit;
  3. the warp field against the float64 projection of the handle's points;
  4. independence of the batch, the run, the subset of outputs requested and the model stride; valid on the stream;
  5. hostile scenes; 6. argument checks on a live handle.

Shapes (the smallest at which each path can go wrong): 120x160 / 4 levels in the three candidate modes (dense: the quad source at every level,
19200 pixels = two chunks of at most 16384 at level 0; DSO level 0 is cut too); 240x320 / 5 levels coarse-to-fine (15 * 20 * 16 = 4800 slots >
4096: the list is cut); 122x162 / 3 levels dense (widths 162, 81, 40: the quad source is refused at levels 0 and 1, which run the one-pixel
source, odd halving included)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from oracle import oracle as O
from test_gpu_first_principles import level_intrinsics
from test_oracle_first_principles import back_project, iso_to_mat, project

N = 4
ARITHS = {"reference": V.ARITH_REFERENCE, "exact": V.ARITH_EXACT, "fused": V.ARITH_FUSED}
CONFIGS = [((120, 160, 4), m, ("reference", "exact", "fused")) for m in (0, 1, 2)] + [((240, 320, 5), 0, ("reference", "fused")),
                                                                                        ((122, 162, 3), 1, ("reference", "fused"))]
PARAMS = [(s, m, h, a) for s, m, ar in CONFIGS for h in (0.0, 10.0) for a in ar]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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


def all_maps(b, lvl, d_models):
    """Every output of the pass + the EXACT 29 sums at the same models, read back once -> dict of numpy arrays."""
    import torch
    out = b.residual_maps(lvl, d_models, residuals=True, warp=True, hist=True, scale=True)
    sums = b.eval_pairs(lvl, d_models, arithmetic=V.ARITH_EXACT)
    torch.cuda.synchronize()
    m = {k: t.cpu().numpy() for k, t in out.items()}
    m["sums29"] = sums.cpu().numpy()[:, 0]
    return m


class Scene:
    """4 rendered pairs tracked once on a handle of one arithmetic; models [N, 2, 7]: each pair's lm_model and one moved by se3_exp(3e-3 u)."""

    def __init__(self, shape, mode, huber, arith):
        import torch
        self.rows, self.cols, self.L = shape
        self.mode, self.huber, self.arith = mode, huber, ARITHS[arith]
        self.intr = V.scaled_intrinsics(self.rows, self.cols)
        self.kg, self.kd, self.cg, _, _ = V.synth_render_pairs(0x5EEDE7A3, N, self.rows, self.cols, self.intr)
        cfg = V.Config(nb_levels=self.L, intrinsics=V.Intrinsics(self.intr[:2], self.intr[2:4], self.intr[4]), candidates_mode=mode,
                       huber_delta=huber, arithmetic=self.arith)
        self.b, self.stats = tracked_handle(cfg, self.kg, self.kd, self.cg, self.rows, self.cols)
        lm = V.decode_stats(self.stats)["lm_model"].copy()
        rng = np.random.default_rng(11)
        self.models = np.empty((N, 2, 7), np.float32)
        for p in range(N):
            self.models[p, 0] = lm[p]
            self.models[p, 1] = V.iso_mul(lm[p], V.se3_exp((rng.uniform(-1, 1, 6) * 3e-3).astype(np.float32)))
        self.d_models = [torch.from_numpy(np.ascontiguousarray(self.models[:, k])).cuda() for k in range(2)]
        self._maps = {}

    def shape(self, lvl):
        return self.rows >> lvl, self.cols >> lvl

    def maps(self, lvl, k):
        if (lvl, k) not in self._maps:   # read back once per (handle, level, model)
            self._maps[lvl, k] = all_maps(self.b, lvl, self.d_models[k])
        return self._maps[lvl, k]


@pytest.fixture(scope="module", params=PARAMS,
                ids=lambda p: f"{p[0][1]}x{p[0][0]}L{p[0][2]}-{('c2f', 'dense', 'dso')[p[1]]}-{'huber' if p[2] else 'l2'}-{p[3]}")
def scene(request):
    return Scene(*request.param)


# ------------------------------------------------------------------------------------------------------------ 1
def test_planes_equal_the_oracle_bit_for_bit(scene):
    sc = scene
    kg, kd, cg = sc.kg.cpu().numpy(), sc.kd.cpu().numpy().view(np.uint16), sc.cg.cpu().numpy()
    for p in range(N):
        tr = O.Tracker(O.make_config(sc.L, sc.intr, candidates_mode=sc.mode, huber_delta=sc.huber), 0.0, kd[p], 0.0, kg[p])
        cur = O.mean_pyramid(cg[p], sc.L)
        for lvl in (0, sc.L - 1):
            rows, cols = sc.shape(lvl)
            xy, iz, jac = tr.points(lvl)
            _, _, _, k5 = tr.level(lvl)
            is_point = np.zeros((rows, cols), bool)
            is_point[xy[:, 1], xy[:, 0]] = True
            assert is_point.sum() == len(xy)
            for k in range(2):
                m = sc.maps(lvl, k)
                res, uv = m["residuals"][p], m["warp"][p]
                assert res.shape == (rows, cols) and uv.shape == (rows, cols, 2)
                assert (np.isfinite(uv[..., 0]) == is_point).all() and (np.isfinite(uv[..., 1]) == is_point).all(), (lvl, p, k)
                assert np.isnan(uv[~is_point]).all() and np.isnan(res[~is_point]).all(), (lvl, p, k)
                _, no, _, _, ro = O.lm_eval(k5, tr.image(lvl), cur[lvl], xy, iz, jac, sc.models[p, k], huber_delta=sc.huber, want_residuals=True)
                mine = res[xy[:, 1], xy[:, 0]]
                both_nan = np.isnan(mine) & np.isnan(ro)
                assert ((bits(mine) == bits(ro)) | both_nan).all(), (lvl, p, k)
                assert int(np.isfinite(mine).sum()) == no == int(m["hist"][p].sum()), (lvl, p, k)


# ------------------------------------------------------------------------------------------------------------ 2
def assert_self_consistent(m, p, rows, cols, huber, what):
    res, uv, hist = m["residuals"][p], m["warp"][p], m["hist"][p].view(np.uint32)
    u, v = uv[..., 0], uv[..., 1]
    assert u.dtype == np.float32
    with np.errstate(invalid="ignore"):
        fu, fv = np.floor(u), np.floor(v)
        inside = (fu >= 0) & (fu < np.float32(cols - 2)) & (fv >= 0) & (fv < np.float32(rows - 2))   # lm_optimizer.rs:227-231; NaN: False
    finite = np.isfinite(res)
    assert (finite == inside).all(), what
    assert not np.isinf(res).any(), what
    r = res[finite]
    # grey levels are 0 .. 255 and the four bilinear weights sum to 1 up to float32 rounding (a handful of ulp of 255, ~1e-4): a saturated
    # patch against a black template gives 255.00002, which the histogram's min(int(|r|), 255) puts in the last bin
    assert (np.abs(r) < 255.01).all(), what
    assert (hist == np.bincount(np.minimum(np.abs(r).astype(int), 255), minlength=256)).all(), what
    s29 = m["sums29"][p]
    assert int(hist.sum()) == int(s29[1]), what
    if huber == 0:
        e64 = float((r.astype(np.float64) ** 2).sum())
        print(f"{what}: |sum r^2 - e| = {abs(e64 - float(s29[0])):.3e} (bound {2e-4 * e64 + 1e-3:.3e})")
        assert abs(e64 - float(s29[0])) <= 2e-4 * e64 + 1e-3, what
    med, sig, n = V.residual_scale_from_hist(hist)
    assert n == int(hist.sum())
    assert (bits(m["scale"][p]) == bits([med, sig])).all(), (what, m["scale"][p], med, sig)
    assert np.isnan(med) == (n == 0)


def test_maps_histogram_sums_and_scale_are_consistent(scene):
    sc = scene
    for lvl in range(sc.L):
        rows, cols = sc.shape(lvl)
        for k in range(2):
            m = sc.maps(lvl, k)
            assert m["hist"].shape == (N, 256) and m["scale"].shape == (N, 2)
            for p in range(N):
                assert_self_consistent(m, p, rows, cols, sc.huber, f"level {lvl} pair {p} model {k}")


# ------------------------------------------------------------------------------------------------------------ 3
def test_warp_field_against_the_float64_projection(scene):
    sc = scene
    for lvl in range(sc.L):
        k5 = level_intrinsics(sc.intr, lvl)
        for p in range(N):
            xy, iz, _, _ = sc.b.points(p, lvl)
            P = back_project(k5, xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64), 1.0 / iz.astype(np.float64))
            for k in range(2):
                T = iso_to_mat(sc.models[p, k])
                u, v = project(k5, P @ T[:3, :3].T + T[:3, 3])
                uv = sc.maps(lvl, k)["warp"][p][xy[:, 1], xy[:, 0]].astype(np.float64)
                err = max(np.abs(uv[:, 0] - u).max(), np.abs(uv[:, 1] - v).max()) if len(xy) else 0.0
                print(f"level {lvl} pair {p} model {k}: {len(xy)} points, max |uv - uv64| = {err:.3e} px")
                assert err <= 2e-3, (lvl, p, k)
                assert int(np.isfinite(sc.maps(lvl, k)["warp"][p][..., 0]).sum()) == len(xy), (lvl, p, k)


# ------------------------------------------------------------------------------------------------------------ 4
def test_planes_do_not_depend_on_the_batch_the_run_or_the_outputs_requested(scene):
    import torch
    sc, b = scene, scene.b
    for lvl in (0, sc.L - 1):
        full = sc.maps(lvl, 1)
        run1 = b.residual_maps(lvl, sc.d_models[1], residuals=True, warp=True, hist=True, scale=True)
        twice = run1["residuals"] * 2.0   # a dependent op on the same stream, no host synchronisation in between
        total = run1["hist"].sum(dim=1)
        run2 = b.residual_maps(lvl, sc.d_models[1], residuals=True, warp=True, hist=True, scale=True)
        subsets = [b.residual_maps(lvl, sc.d_models[1], **kw) for kw in (dict(), dict(residuals=False, warp=True), dict(residuals=False, hist=True),
                                                                         dict(residuals=False, scale=True), dict(warp=True, scale=True))]
        alone = {}
        for p in (0, 2, 3):
            first = sc.models[:p + 1, 0].copy()
            first[p] = sc.models[p, 1]
            alone[p] = b.residual_maps(lvl, torch.from_numpy(first).cuda(), residuals=True, warp=True, hist=True, scale=True)
        at_lm = b.residual_maps(lvl, sc.stats, residuals=True, warp=True, hist=True, scale=True)   # the stats tensor, struct stride
        torch.cuda.synchronize()
        for name in ("residuals", "warp", "hist", "scale"):
            want = full[name].view(np.uint32)
            for run in [run1, run2] + subsets:
                if name in run:
                    assert (run[name].cpu().numpy().view(np.uint32) == want).all(), (lvl, name)
            for p, t in alone.items():
                assert t[name].shape[0] == p + 1
                assert (t[name].cpu().numpy()[p].view(np.uint32) == want[p]).all(), (lvl, name, p)
            assert (at_lm[name].cpu().numpy().view(np.uint32) == sc.maps(lvl, 0)[name].view(np.uint32)).all(), (lvl, name)
        assert [sorted(s) for s in subsets] == [["residuals"], ["warp"], ["hist"], ["scale"], ["residuals", "scale", "warp"]]
        assert (bits(twice.cpu().numpy()) == bits(full["residuals"] * np.float32(2.0))).all(), lvl
        assert (total.cpu().numpy() == full["hist"].sum(axis=1)).all(), lvl


# ------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("name", ["rank_deficient", "saturated"])
@pytest.mark.parametrize("arith", list(ARITHS))
def test_hostile_scenes(name, arith):
    import torch
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "adversarial", name + ".npz"))
    L, mode, rows, cols, intr = int(g["L"]), int(g["mode"]), int(g["rows"]), int(g["cols"]), tuple(float(x) for x in g["intr"])
    kg, cg = (torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("kf_gray", "cur_gray"))
    kd = torch.from_numpy(np.ascontiguousarray(g["kf_depth"]).view(np.int16)).cuda()
    n, huber = kg.shape[0], float(g["huber"])
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, huber_delta=huber, arithmetic=ARITHS[arith])
    b, stats = tracked_handle(cfg, kg, kd, cg, rows, cols)
    for lvl in range(L):
        m = all_maps(b, lvl, stats)   # VORS_OK, or _check raises
        for p in range(n):
            assert_self_consistent(m, p, rows >> lvl, cols >> lvl, huber, f"{name} level {lvl} pair {p}")
            if name == "rank_deficient":   # at most 5 points with a depth per pair
                assert int(np.isfinite(m["warp"][p][..., 0]).sum()) <= 5, (lvl, p)


# ------------------------------------------------------------------------------------------------------------ 6
def test_argument_validation_on_a_live_handle():
    import torch
    rows, cols, L = 120, 160, 4
    intr = V.scaled_intrinsics(rows, cols)
    kg, kd, cg, _, _ = V.synth_render_pairs(0x5EEDE7A2, 4, rows, cols, intr)
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), arithmetic=V.ARITH_FUSED)
    b = V.Batch(cfg, 8, rows, cols)
    models = torch.zeros((8, 7), dtype=torch.float32, device="cuda")
    models[:, 6] = 1
    res = torch.zeros((8, rows, cols), dtype=torch.float32, device="cuda")
    uv = torch.zeros((8, rows, cols, 2), dtype=torch.float32, device="cuda")
    hist = torch.zeros((8, 256), dtype=torch.int32, device="cuda")
    scale = torch.zeros((8, 2), dtype=torch.float32, device="cuda")
    b.prepare_keyframes(kg, kd)
    with pytest.raises(V.VorsError) as before_track:
        b.residual_maps(0, models[:1])
    assert "track_current" in str(before_track.value)
    poses = torch.zeros((4, 7), dtype=torch.float32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    b.track_current(cg, poses, status)
    before = b.workspace_bytes()
    lib, s = V.lib(), b._stream()
    outs = dict(res=res, uv=uv, hist=hist, scale=scale)

    def call(n=4, lvl=0, stride=0, mdl=models, **kw):
        o = {**outs, **kw}
        return lib.vors_batch_residual_maps(b._h, n, lvl, b._dp(mdl), stride, b._dp(o["res"]), b._dp(o["uv"]), b._dp(o["hist"]), b._dp(o["scale"]), s)

    assert call() == 0
    assert call(res=None, uv=None, scale=None) == 0 and call(res=None, uv=None) == 0 and call(hist=None, scale=None) == 0
    assert b.workspace_bytes() == before   # the pass has no workspace, with or without d_hist
    for bad, word in ((dict(lvl=L), "level"), (dict(lvl=-1), "level"), (dict(n=5), "n_pairs"), (dict(n=0), "n_pairs"), (dict(stride=30), "stride"),
                      (dict(stride=24), "stride"), (dict(mdl=None), "d_models"), (dict(res=None, uv=None, hist=None, scale=None), "every output"),
                      (dict(hist=None), "d_scale needs d_hist")):
        assert call(**bad) == -1, bad
        assert word.encode() in lib.vors_last_error(), (bad, lib.vors_last_error())
    with pytest.raises(V.VorsError):
        b.residual_maps(0, models[:4], residuals=False)
    with pytest.raises(V.VorsError):
        b.residual_maps(0, torch.zeros((4, 2, 7), dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    assert b.workspace_bytes() == before
