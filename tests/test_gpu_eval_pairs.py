"""The batched evaluation at explicit models (vors_batch_eval_pairs) and the pose information built on it (vors_batch_pose_information). GPU only.

  * REFERENCE on a REFERENCE handle: the sums of every (pair, level, model) equal vors_batch_eval_level's bit for bit, and on the finest and
    the coarsest level the oracle's (oracle.lm_eval on oracle.Tracker's points);
  * EXACT and FUSED: n_inside equals eval_level's, the sums lie within the bounds tests/test_gpu_first_principles.py applies between the
    device's tree sums and the float64 definition (2e-4 / 5e-4 / 2e-4 relative, with its border slack), and a level of one workgroup gives
    eval_level's bits;
  * the sums of a (pair, model) do not depend on the batch around it, nor on the run; the output is valid on the stream;
  * energy-only; pose information against the host algebra on the device's own sums; hostile scenes; argument checks.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from oracle import oracle as O
from test_gpu_first_principles import level_intrinsics
from test_oracle_first_principles import back_project, iso_to_mat, project
from test_pose_information_host import cov_bound, mirrored, same_bits

N = 8
SHAPES = [(120, 160, 4), (240, 320, 5)]
ARITHS = {"reference": V.ARITH_REFERENCE, "exact": V.ARITH_EXACT, "fused": V.ARITH_FUSED}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Scene:
    """8 rendered pairs, tracked once per arithmetic on a handle of that arithmetic; models [N, 4, 7]: each pair's lm_model + 3 moved ones."""

    def __init__(self, shape, mode, huber):
        import torch
        self.rows, self.cols, self.L = shape
        self.mode, self.huber = mode, huber
        self.intr = V.scaled_intrinsics(self.rows, self.cols)
        self.kg, self.kd, self.cg, _, _ = V.synth_render_pairs(0x5EEDE7A1, N, self.rows, self.cols, self.intr)
        self.handles = {}
        self.level_data = {}
        torch.cuda.synchronize()

    def handle(self, arith):
        import torch
        if arith not in self.handles:
            cfg = V.Config(nb_levels=self.L, intrinsics=V.Intrinsics(self.intr[:2], self.intr[2:4], self.intr[4]), candidates_mode=self.mode,
                           huber_delta=self.huber, arithmetic=arith)
            b = V.Batch(cfg, N, self.rows, self.cols)
            poses = torch.zeros((N, 7), dtype=torch.float32, device="cuda")
            status = torch.zeros(N, dtype=torch.int32, device="cuda")
            stats = V.stats_tensor(N)
            b.track_pairs(self.kg, self.kd, self.cg, poses, status, stats)
            torch.cuda.synchronize()
            lm = V.decode_stats(stats)["lm_model"].copy()
            rng = np.random.default_rng(11)
            models = np.empty((N, 4, 7), np.float32)
            for p in range(N):
                models[p, 0] = lm[p]
                for k in range(1, 4):
                    models[p, k] = V.iso_mul(lm[p], V.se3_exp((rng.uniform(-1, 1, 6) * 3e-3).astype(np.float32)))
            self.handles[arith] = (b, stats, models, torch.from_numpy(models).cuda())
        return self.handles[arith]

    def one_workgroup(self, lvl):
        """engine.h eval_pairs_chunks: a level of at most 16384 pixels (dense) / 4096 candidate slots is one workgroup."""
        r, c = self.rows >> lvl, self.cols >> lvl
        if self.mode == V.CANDIDATES_DENSE:
            return r * c <= 16384
        if self.mode == V.CANDIDATES_DSO:
            return min(r * c, 65536) <= 4096
        return (self.rows >> (self.L - 1)) * (self.cols >> (self.L - 1)) * (1 << (self.L - 1 - lvl)) <= 4096


@pytest.fixture(scope="module", params=[(s, m, h) for s in SHAPES for m in (0, 1, 2) for h in (0.0, 10.0)],
                ids=lambda p: f"{p[0][1]}x{p[0][0]}L{p[0][2]}-{('c2f', 'dense', 'dso')[p[1]]}-{'huber' if p[2] else 'l2'}")
def scene(request):
    return Scene(*request.param)


def level29(b, pair, lvl, model7, arith):
    m = np.ascontiguousarray(model7, np.float32)
    out = np.zeros(29, np.float32)
    V._check(V.lib().vors_batch_eval_level(b._h, pair, lvl, V._ptr(m), int(arith), V._ptr(out)))
    return out


def synced(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def float64_sums(sc, b, pair, lvl, model):
    """tests/test_gpu_first_principles.py's float64 definition of one evaluation (+ Huber: loss, weights |r| > delta -> delta / |r|) and what
    the points within float32 rounding of the window border may change -> (e, n, g, H), (slack_e, slack_n, slack_g, slack_H), scale_g."""
    k = level_intrinsics(sc.intr, lvl)
    key = (id(b), pair, lvl)
    if key not in sc.level_data:   # read back once per (handle, pair, level), shared by every model and test
        sc.level_data[key] = b.points(pair, lvl) + (b.current_image(pair, lvl),)
    xy, iz, jac, tm, img = sc.level_data[key]
    rows, cols = img.shape
    T = iso_to_mat(model)
    P = back_project(k, xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64), 1.0 / iz.astype(np.float64))
    u, v = project(k, P @ T[:3, :3].T + T[:3, 3])
    fu, fv = np.floor(u), np.floor(v)
    inside = (fu >= 0) & (fu < cols - 2) & (fv >= 0) & (fv < rows - 2)
    border = inside ^ ((np.floor(u - 2e-3) >= 0) & (np.floor(u + 2e-3) < cols - 2) & (np.floor(v - 2e-3) >= 0) & (np.floor(v + 2e-3) < rows - 2))
    iu, iv = np.clip(fu, 0, cols - 2).astype(int), np.clip(fv, 0, rows - 2).astype(int)
    a, c = u - fu, v - fv
    I = img.astype(np.float64)
    val = (1 - a) * (1 - c) * I[iv, iu] + a * (1 - c) * I[iv, iu + 1] + (1 - a) * c * I[iv + 1, iu] + a * c * I[iv + 1, iu + 1]
    r = np.where(inside, val - tm.astype(np.float64), 0.0)
    Jd = jac.astype(np.float64)
    if sc.huber > 0:
        ar = np.abs(r)
        lin = ar > sc.huber
        loss = np.where(lin, sc.huber * (2 * ar - sc.huber), r * r)
        w = np.where(lin, sc.huber / np.maximum(ar, 1e-300), 1.0)
    else:
        loss, w = r * r, np.ones_like(r)
    e_ref, g_ref = loss.sum(), (Jd * (w * r)[:, None]).sum(0)
    H_ref = (Jd[inside] * w[inside, None]).T @ Jd[inside]
    slack_e = (np.abs(val - tm)[border] ** 2).sum()
    slack_g = (np.abs(Jd[border]) * np.abs(val - tm)[border, None]).sum(0).max() if border.any() else 0.0
    slack_H = (np.abs(Jd[border]).max() ** 2) * border.sum() if border.any() else 0.0
    return (e_ref, int(inside.sum()), g_ref, H_ref), (slack_e, int(border.sum()), slack_g, slack_H), np.abs(Jd * (w * r)[:, None]).sum(0).max()


def assert_within_float64_bounds(s29, ref, slack, scale_g, what, energy_only=False):
    (e_ref, n_ref, g_ref, H_ref), (slack_e, slack_n, slack_g, slack_H) = ref, slack
    err_e = abs(float(s29[0]) - e_ref)
    print(f"{what}: |e - e64| = {err_e:.3e} (bound {2e-4 * e_ref + slack_e + 1e-3:.3e})", end="")
    assert abs(int(s29[1]) - n_ref) <= slack_n, what
    assert err_e <= 2e-4 * e_ref + slack_e + 1e-3, what
    if energy_only:
        print()
        return
    H = mirrored(s29).astype(np.float64)
    err_g, err_H = np.abs(s29[2:8] - g_ref).max(), np.abs(H - H_ref).max()
    print(f", |g - g64| = {err_g:.3e} (bound {5e-4 * scale_g + slack_g:.3e}), |H - H64| = {err_H:.3e} (bound {2e-4 * np.abs(H_ref).max() + slack_H:.3e})")
    assert err_g <= 5e-4 * scale_g + slack_g, what
    assert err_H <= 2e-4 * np.abs(H_ref).max() + slack_H, what


# ------------------------------------------------------------------------------------------------------------ 1
def test_reference_sums_equal_eval_level_and_the_oracle_bit_for_bit(scene):
    sc = scene
    b, stats, models, d_models = sc.handle(V.ARITH_REFERENCE)
    kg, kd, cg = sc.kg.cpu().numpy(), sc.kd.cpu().numpy().view(np.uint16), sc.cg.cpu().numpy()
    for lvl in range(sc.L):
        at_lm = synced(b.eval_pairs(lvl, stats, arithmetic=V.ARITH_REFERENCE))   # the stats tensor, struct stride, one model per pair
        at_all = synced(b.eval_pairs(lvl, d_models, arithmetic=V.ARITH_REFERENCE))
        assert at_lm.shape == (N, 1, 29) and at_all.shape == (N, 4, 29)
        for p in range(N):
            assert (bits(at_lm[p, 0]) == bits(at_all[p, 0])).all(), (lvl, p)
            for k in range(4):
                assert (bits(at_all[p, k]) == bits(level29(b, p, lvl, models[p, k], V.ARITH_REFERENCE))).all(), (lvl, p, k)
        if lvl not in (0, sc.L - 1):
            continue
        for p in range(N):
            tr = O.Tracker(O.make_config(sc.L, sc.intr, candidates_mode=sc.mode, huber_delta=sc.huber), 0.0, kd[p], 0.0, kg[p])
            cur = O.mean_pyramid(cg[p], sc.L)
            xy, iz, jac = tr.points(lvl)
            _, _, _, k5 = tr.level(lvl)
            for k in range(4):
                eo, no, go, Ho = O.lm_eval(k5, tr.image(lvl), cur[lvl], xy, iz, jac, models[p, k], huber_delta=sc.huber)
                s = at_all[p, k]
                assert int(s[1]) == no, (lvl, p, k)
                if no > 0:
                    assert same_bits(np.float32(s[0]) / np.float32(s[1]), np.float32(eo)), (lvl, p, k)
                assert same_bits(s[2:8], go) and same_bits(mirrored(s), Ho), (lvl, p, k)


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("arith", ["exact", "fused"])
def test_tree_sums_against_eval_level_and_float64(scene, arith):
    sc, ar = scene, ARITHS[arith]
    b, stats, models, d_models = sc.handle(ar)
    for lvl in range(sc.L):
        out = synced(b.eval_pairs(lvl, d_models, arithmetic=ar))
        for p in range(N):
            for k in range(4):
                lv = level29(b, p, lvl, models[p, k], ar)
                assert out[p, k, 1] == lv[1], (lvl, p, k)
                if sc.one_workgroup(lvl):
                    assert (bits(out[p, k]) == bits(lv)).all(), (lvl, p, k)
        for p in range(N):
            for k in range(4):
                ref, slack, scale_g = float64_sums(sc, b, p, lvl, models[p, k])
                assert_within_float64_bounds(out[p, k], ref, slack, scale_g, f"{arith} level {lvl} pair {p} model {k}")


# ------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("arith", list(ARITHS))
def test_sums_do_not_depend_on_the_batch_or_the_run_and_are_valid_on_the_stream(scene, arith):
    import torch
    sc, ar = scene, ARITHS[arith]
    b, stats, models, d_models = sc.handle(ar)
    rng = np.random.default_rng(5)
    models8 = np.empty((N, 8, 7), np.float32)
    for p in range(N):
        for k in range(8):
            models8[p, k] = V.iso_mul(models[p, 0], V.se3_exp((rng.uniform(-1, 1, 6) * 3e-3).astype(np.float32)))
    d8 = torch.from_numpy(models8).cuda()
    for lvl in (0, sc.L - 1):
        run1 = b.eval_pairs(lvl, d8, arithmetic=ar)
        twice = run1 * 2.0   # a dependent op on the same stream, no host synchronisation in between
        run2 = b.eval_pairs(lvl, d8, arithmetic=ar)
        alone = {}
        for p in (0, 3, 7):
            first = models[:p + 1, 0].copy()
            first[p] = models8[p, 5]
            alone[p] = b.eval_pairs(lvl, torch.from_numpy(first).cuda(), arithmetic=ar)
        torch.cuda.synchronize()
        run1, run2, twice = run1.cpu().numpy(), run2.cpu().numpy(), twice.cpu().numpy()
        assert (bits(run1) == bits(run2)).all(), lvl
        assert (twice == run1 * np.float32(2.0)).all(), lvl
        for p, t in alone.items():
            assert t.shape == (p + 1, 1, 29)
            assert (bits(t.cpu().numpy()[p, 0]) == bits(run1[p, 5])).all(), (lvl, p)


@pytest.mark.parametrize("arith", list(ARITHS))
def test_more_items_than_the_workspace_holds_run_as_slices_with_the_same_bits(scene, arith):
    """The workspace of the pass holds max(max_pairs, 256) items: 8 pairs x 40 models = 320 items run as two slices (256 + 64). Every
    (pair, model) must give the bits it gives as one of 8 items, in the full and the energy-only form."""
    import torch
    sc, ar = scene, ARITHS[arith]
    b, stats, models, d_models = sc.handle(ar)
    K = 40
    assert N * K > max(N, 256)
    rng = np.random.default_rng(23)
    models40 = np.empty((N, K, 7), np.float32)
    for p in range(N):
        for k in range(K):
            models40[p, k] = V.iso_mul(models[p, 0], V.se3_exp((rng.uniform(-1, 1, 6) * 3e-3).astype(np.float32)))
    d40 = torch.from_numpy(models40).cuda()
    for lvl in (0, sc.L - 1):
        for what in ("full", "energy"):
            sliced = b.eval_pairs(lvl, d40, arithmetic=ar, what=what)
            single = [b.eval_pairs(lvl, d40[:, k].contiguous(), arithmetic=ar, what=what) for k in range(K)]
            torch.cuda.synchronize()
            sliced = sliced.cpu().numpy()
            assert sliced.shape == (N, K, 29)
            for k in range(K):
                assert (bits(sliced[:, k]) == bits(single[k].cpu().numpy()[:, 0])).all(), (lvl, what, k)



# ------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("arith", list(ARITHS))
def test_energy_only(scene, arith):
    sc, ar = scene, ARITHS[arith]
    b, stats, models, d_models = sc.handle(ar)
    for lvl in range(sc.L):
        full = synced(b.eval_pairs(lvl, d_models, arithmetic=ar))
        en = synced(b.eval_pairs(lvl, d_models, arithmetic=ar, what="energy"))
        assert (en[:, :, 2:] == 0).all(), lvl
        if ar != V.ARITH_FUSED:
            assert (bits(en[:, :, :2]) == bits(full[:, :, :2])).all(), lvl
        else:
            for p, k in ((p, k) for p in range(N) for k in range(4)):
                ref, slack, scale_g = float64_sums(sc, b, p, lvl, models[p, k])
                assert_within_float64_bounds(en[p, k], ref, slack, scale_g, f"fused energy-only level {lvl} pair {p} model {k}", energy_only=True)


# ------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("arith", list(ARITHS))
def test_pose_information_equals_the_host_algebra_on_the_device_sums(scene, arith):
    sc, ar = scene, ARITHS[arith]
    b, stats, models, d_models = sc.handle(ar)
    info, cov, s2, flags = b.pose_information(0, stats)
    sums = synced(b.eval_pairs(0, stats))
    info, cov, s2, flags = info.cpu().numpy(), cov.cpu().numpy(), s2.cpu().numpy(), flags.cpu().numpy()
    for p in range(N):
        hi, hc, hs, hf = V.pose_information_from_sums(sums[p, 0])
        assert flags[p] == hf and same_bits(info[p], hi)
        if hf:
            assert np.isnan(cov[p]).all() and np.isnan(s2[p])
            continue
        assert same_bits(s2[p], hs)
        H64 = hi.astype(np.float64)
        ref = np.float64(hs) * np.linalg.inv(H64)
        assert (np.abs(cov[p].astype(np.float64) - hc.astype(np.float64)) <= cov_bound(H64, ref)).all(), p


@pytest.mark.parametrize("name", ["rank_deficient", "saturated"])
@pytest.mark.parametrize("arith", list(ARITHS))
def test_pose_information_on_hostile_scenes(name, arith):
    import torch
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "adversarial", name + ".npz"))
    L, mode, rows, cols, intr = int(g["L"]), int(g["mode"]), int(g["rows"]), int(g["cols"]), tuple(float(x) for x in g["intr"])
    kg, cg = (torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("kf_gray", "cur_gray"))
    kd = torch.from_numpy(np.ascontiguousarray(g["kf_depth"]).view(np.int16)).cuda()
    n = kg.shape[0]
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, huber_delta=float(g["huber"]),
                   arithmetic=ARITHS[arith])
    b = V.Batch(cfg, n, rows, cols)
    poses = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    stats = V.stats_tensor(n)
    b.track_pairs(kg, kd, cg, poses, status, stats)
    info, cov, s2, flags = b.pose_information(0, stats)   # VORS_OK, or _check raises
    sums = synced(b.eval_pairs(0, stats))
    info, cov, s2, flags = info.cpu().numpy(), cov.cpu().numpy(), s2.cpu().numpy(), flags.cpu().numpy()
    for p in range(n):
        hi, hc, hs, hf = V.pose_information_from_sums(sums[p, 0])
        assert flags[p] == hf and same_bits(info[p], hi), p
        if flags[p]:
            assert np.isnan(cov[p]).all() and np.isnan(s2[p]), p
        else:
            assert np.isfinite(cov[p]).all() and np.isfinite(s2[p]), p
    if name == "rank_deficient":  # at most 5 points with a depth per pair: every pair is affected
        assert (sums[:, 0, 1] <= 6).all() and (flags & 1).all()
    if arith != "reference":
        return
    # Which pairs are affected, decided without the device and without the library's algebra: the oracle's evaluation of level 0 at the
    # pair's lm_model, the count, and the float64 spectrum of its H. A float64 Cholesky of a 6x6 matrix goes through when the smallest
    # eigenvalue is above ~6 * 2^-52 of the largest and meets a bad pivot when it is below minus that; 1e-12 of the largest leaves four
    # decades to either side, and a matrix in between (numerically singular) may go either way, so nothing is asserted of it.
    lm = V.decode_stats(stats)["lm_model"]
    kg_h, cg_h, kd_h = g["kf_gray"], g["cur_gray"], np.ascontiguousarray(g["kf_depth"]).view(np.uint16)
    decided = 0
    for p in range(n):
        tr = O.Tracker(O.make_config(L, intr, candidates_mode=mode, huber_delta=float(g["huber"])), 0.0, kd_h[p], 0.0, kg_h[p])
        xy, iz, jac = tr.points(0)
        _, _, _, k5 = tr.level(0)
        _, no, _, Ho = O.lm_eval(k5, tr.image(0), O.mean_pyramid(cg_h[p], L)[0], xy, iz, jac, lm[p], huber_delta=float(g["huber"]))
        ev = np.linalg.eigvalsh(np.asarray(Ho, np.float64))
        few = no <= 6
        assert bool(flags[p] & 1) == few, (p, no)
        if ev[0] > 1e-12 * ev[-1]:
            assert not flags[p] & 2, (p, ev)
            decided += 1
        elif ev[0] < -1e-12 * max(ev[-1], 0.0) or ev[-1] <= 0.0:
            assert flags[p] & 2, (p, ev)
            decided += 1
    print(f"{name}: {decided} of {n} pairs decided by the spectrum, flags {flags.tolist()}")


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
    out = torch.zeros((8, 29), dtype=torch.float32, device="cuda")
    before = b.workspace_bytes()
    b.prepare_keyframes(kg, kd)
    with pytest.raises(V.VorsError) as before_track:
        b.eval_pairs(0, models[:1])
    with pytest.raises(V.VorsError) as level_before_track:
        b.eval_level(0, 0, [0, 0, 0, 0, 0, 0, 1], V.ARITH_FUSED)
    assert str(before_track.value) == str(level_before_track.value)
    poses = torch.zeros((4, 7), dtype=torch.float32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    b.track_current(cg, poses, status)
    assert b.workspace_bytes() == before   # a handle that has not evaluated yet has not paid for the pass
    lib, s = V.lib(), b._stream()

    def call(n=4, lvl=0, k=1, stride=0, arith=V.ARITH_FUSED, what=0):
        return lib.vors_batch_eval_pairs(b._h, n, lvl, k, b._dp(models), stride, arith, what, b._dp(out), s)

    assert call() == 0
    after = b.workspace_bytes()
    assert after > before
    assert call(k=2) == 0 and b.workspace_bytes() == after   # no allocation after the first call
    for bad, word in ((dict(lvl=L), "level"), (dict(lvl=-1), "level"), (dict(n=5), "n_pairs"), (dict(n=0), "n_pairs"), (dict(stride=30), "stride"),
                      (dict(stride=24), "stride"), (dict(what=7), "what"), (dict(k=0), "models_per_pair"), (dict(arith=9), "arithmetic")):
        assert call(**bad) == -1, bad
        assert word.encode() in lib.vors_last_error(), (bad, lib.vors_last_error())
    torch.cuda.synchronize()
