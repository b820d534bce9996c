"""Adversarial frame pairs for the parity tests: deterministic edits of the synthetic scene (oracle.synth_*) that drive the tracker into
the corners the plain scene never reaches — depth discontinuities, large invalid regions, occluders, large motion, brightness jumps,
saturated checkerboards — and into the LM loop's rarer outcomes:

  1  a level fails (Cholesky) after the coarser levels converged: `lm_model` has already moved when the keyframe test runs
     (inverse_compositional.rs:195-224);
  2  a level fails after it accepted at least one step: the level's progress is discarded, `lm_model` is the model it started from;
  3  an accepted evaluation with no point inside the image: energy 0 / 0 = NaN is not greater than the kept energy, so the step is
     accepted and `!(d_energy > 1)` ends the level with energy NaN (lm_optimizer.rs:140-192).

The edited arrays go to the oracle and to the device alike, so a scene need not be geometrically consistent: only parity is asserted.
`classify` replays the oracle's LM loop level by level from the oracle's own primitives (lm_eval, lm_step) and reports, per pair, which
of the outcomes it went through; `check_replay` asserts that the replay reproduces oracle.track_pairs bit for bit, so the
classification is the oracle's. CPU only (numpy + the oracle)."""
import numpy as np

from oracle import oracle as O

F32 = np.float32
BLOCKY = 1 << 63


def identity7():
    return np.array([0, 0, 0, 0, 0, 0, 1], np.float32)


# ---------------------------------------------------------------------------------------------- scene families
def _pairs(seed, n, rows, cols, intr, motion_scale=1.0):
    kg = np.empty((n, rows, cols), np.uint8)
    kd = np.empty((n, rows, cols), np.uint16)
    cg = np.empty((n, rows, cols), np.uint8)
    for i in range(n):
        ms = float(motion_scale[i]) if np.ndim(motion_scale) else float(motion_scale)
        kg[i], kd[i], cg[i], _, _ = O.synth_pair(seed + i, rows, cols, intr, motion_scale=ms)
    return kg, kd, cg


def depth_step(seed, n, rows, cols, intr):
    """One rectangle (even pairs) or a half plane (odd pairs) at 0.4-0.6x the depth of the rest, with a sharp edge."""
    rng = np.random.default_rng(seed)
    kg, kd, cg = _pairs(seed, n, rows, cols, intr)
    for i in range(n):
        f = rng.uniform(0.4, 0.6)
        m = np.zeros((rows, cols), bool)
        if i % 2:
            m[:, int(rng.integers(cols // 4, 3 * cols // 4)):] = True
        else:
            h, w = int(rng.integers(rows // 4, rows // 2)), int(rng.integers(cols // 4, cols // 2))
            y, x = int(rng.integers(0, rows - h)), int(rng.integers(0, cols - w))
            m[y:y + h, x:x + w] = True
        d = kd[i].astype(np.float64)
        kd[i] = np.where(m & (kd[i] > 0), np.maximum(1, np.rint(d * f)), d).astype(np.uint16)
    return kg, kd, cg, None


def invalid_blobs(seed, n, rows, cols, intr, fractions=(0.3, 0.6, 0.9)):
    """Random discs of unknown depth until pair i has lost fractions[i % 3] of its pixels."""
    rng = np.random.default_rng(seed)
    kg, kd, cg = _pairs(seed, n, rows, cols, intr)
    yy, xx = np.mgrid[0:rows, 0:cols]
    for i in range(n):
        gone = np.zeros((rows, cols), bool)
        while gone.mean() < fractions[i % len(fractions)]:
            r = rng.uniform(0.05, 0.2) * min(rows, cols)
            cy, cx = rng.uniform(0, rows), rng.uniform(0, cols)
            gone |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        kd[i][gone] = 0
    return kg, kd, cg, None


def occluder(seed, n, rows, cols, intr):
    """A rectangle of 20 % of the image pasted into the current frame only: foreign texture (even pairs) or constant grey (odd)."""
    rng = np.random.default_rng(seed)
    kg, kd, cg = _pairs(seed, n, rows, cols, intr)
    for i in range(n):
        aspect = rng.uniform(0.6, 1.6)
        h = min(rows, int(round(np.sqrt(0.2 * rows * cols / aspect))))
        w = min(cols, int(round(0.2 * rows * cols / h)))
        y, x = int(rng.integers(0, rows - h + 1)), int(rng.integers(0, cols - w + 1))
        if i % 2 == 0:
            foreign, _ = O.synth_frame(seed + 7919 * (i + 1), np.zeros(6), rows, cols, intr)
            cg[i, y:y + h, x:x + w] = foreign[y:y + h, x:x + w]
        else:
            cg[i, y:y + h, x:x + w] = 128
    return kg, kd, cg, None


def large_motion(seed, n, rows, cols, intr):
    """motion_scale 4-8 and, for three pairs in four, an initial pose far off (translations up to 0.5, rotations up to 0.3 rad):
    some candidates warp every point out of view."""
    rng = np.random.default_rng(seed)
    kg, kd, cg = _pairs(seed, n, rows, cols, intr, motion_scale=rng.uniform(4.0, 8.0, n))
    init = np.tile(identity7(), (n, 1))
    for i in range(n):
        if i % 4:
            init[i] = O.gt_model7(np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.3, 0.3, 3)]))
    return kg, kd, cg, init


def brightness_jump(seed, n, rows, cols, intr):
    """A low-contrast texture (a fifth of the synthetic one's) and a current frame 60 grey levels brighter (even pairs) or darker:
    large residuals, small Jacobians, huge first steps. Meant for the dense candidate mode."""
    kg, kd, cg = _pairs(seed, n, rows, cols, intr)
    for i in range(n):
        sign = 1 if i % 2 == 0 else -1
        base = 128 - 60 * sign
        kg[i] = np.clip(np.rint(base + (kg[i].astype(np.float64) - 128.0) * 0.2), 0, 255).astype(np.uint8)
        cg[i] = np.clip(np.rint(base + (cg[i].astype(np.float64) - 128.0) * 0.2) + 60 * sign, 0, 255).astype(np.uint8)
    return kg, kd, cg, None


def saturated(seed, n, rows, cols, intr):
    """0 / 255 checkerboards (cell sizes 1-8, random phase): gradients of +-127, whose squared norm wraps in u16
    (gradient.rs:38-44); the current frame is the same board moved by up to two pixels."""
    rng = np.random.default_rng(seed)
    _, kd, _ = _pairs(seed, n, rows, cols, intr)
    kg = np.empty((n, rows, cols), np.uint8)
    cg = np.empty((n, rows, cols), np.uint8)
    yy, xx = np.mgrid[0:rows + 8, 0:cols + 8]
    for i in range(n):
        cell = int(rng.choice([1, 2, 3, 4, 5, 8]))
        board = (((yy + int(rng.integers(0, cell))) // cell + xx // cell) % 2 * 255).astype(np.uint8)
        dy, dx = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        kg[i] = board[4:4 + rows, 4:4 + cols]
        cg[i] = board[4 + dy:4 + dy + rows, 4 + dx:4 + dx + cols]
    return kg, kd, cg, None


# ---------------------------------------------------------------------------------------------- outcome-targeted constructions
def mid_pyramid_frame(seed, rows, cols, intr, axis=0):
    """A keyframe whose level 0 is singular while the coarser levels are not (outcome 1). axis 0: the texture is constant over bands
    of four rows, and the depth is unknown wherever the oracle's level-0 gy != 0 — every remaining level-0 point has
    J[1] = _z (gu s + gv fv) = 0 (skew 0, warp_jacobian_at), so H[1][1] = 0 and Cholesky fails at level 0 whatever lm_coef is; the
    coarser levels sit on 2x2 means, where gy is generally not 0. axis 1: the same with columns, gx and J[0].
    (The gradients depend on the grey image alone.) -> (gray, depth) of the keyframe."""
    gray, depth = O.synth_frame(seed, np.zeros(6), rows, cols, intr)
    # bands {4k-1 .. 4k+2}: the centred level-0 gradient across them is 0 on rows 4k and 4k+1, while the 2x2 blocks that the coarser
    # levels' gradients are taken on (rows 2i, 2i+1) straddle a band edge every other block
    band = lambda m: np.minimum((np.arange(m) + 1) // 4 * 4, m - 1)
    gray = np.ascontiguousarray(gray[band(rows)] if axis == 0 else gray[:, band(cols)])
    gx, gy, _ = O.Tracker(O.make_config(1, intr), 0.0, depth, 0.0, gray).gradients(0)
    depth = depth.copy()
    depth[(gy if axis == 0 else gx) != 0] = 0
    return gray, depth


def mid_pyramid(seed, n, rows, cols, intr):
    """Outcome 1: the mid_pyramid_frame keyframe against itself moved by 2-7 pixels along its bands (the coarse levels have something
    to converge to). Even pairs: row bands, odd pairs: column bands."""
    rng = np.random.default_rng(seed)
    kg = np.empty((n, rows, cols), np.uint8)
    kd = np.empty((n, rows, cols), np.uint16)
    cg = np.empty((n, rows, cols), np.uint8)
    for i in range(n):
        axis = i % 2
        kg[i], kd[i] = mid_pyramid_frame(seed + i, rows, cols, intr, axis)
        cg[i] = np.roll(kg[i], int(rng.integers(2, 8)) * int(rng.choice([-1, 1])), axis=1 - axis)
    return kg, kd, cg, None


def rank_deficient(seed, n, rows, cols, intr, mode=0, L=3):
    """Outcome 2: a known depth on only 1-5 level-0 candidates, so H has rank <= 5 at every level. Each accepted step divides lm_coef
    by 10; once 1 + lm_coef == 1 in f32 the last pivot can go (lm_optimizer.rs:131-133) — after accepted steps of the same level.
    The current frame is the keyframe moved by a few pixels (large residuals: the level accepts steps before it gets there).
    `mode` / `L`: the candidate mask the points are drawn from (DSO: pass a BLOCKY seed, the selector needs that texture)."""
    rng = np.random.default_rng(seed)
    kg, kd, cg = _pairs(seed, n, rows, cols, intr)
    interior = np.zeros((rows, cols), bool)
    interior[3:rows - 3, 3:cols - 3] = True
    for i in range(n):
        mask = O.Tracker(O.make_config(L, intr, candidates_mode=mode), 0.0, kd[i], 0.0, kg[i]).mask()  # (coarse-to-fine: depends on L)
        cand = np.flatnonzero((mask != 0) & (kd[i] > 0) & interior)
        keep = rng.choice(cand, size=int(rng.integers(1, 6)), replace=False)
        d = np.zeros(rows * cols, np.uint16)
        d[keep] = kd[i].reshape(-1)[keep]
        kd[i] = d.reshape(rows, cols)
        sy, sx = (int(rng.integers(1, 6)) * int(rng.choice([-1, 1])) for _ in range(2))
        cg[i] = np.roll(kg[i], (sy, sx), axis=(0, 1))
    return kg, kd, cg, None


def mid_pyramid_sequences(seed, n_seq, n_frames, rows, cols, intr):
    """Keyframe switches on failed frames: frame 0 of sequence s is a mid_pyramid_frame (row bands for even s, column bands for odd),
    frame k is frame 0 moved along its bands by a running sum of 1-8 pixel steps, grey and depth alike (np.roll), so whichever frame is
    the keyframe has a singular level 0. Every frame then fails at level 0 after the coarser levels moved the model, the keyframe test
    runs on that model, and a large enough move makes the failed frame the keyframe with the kept pose.
    -> gray, depth [n_frames, n_seq, rows, cols] (frame-major, like oracle.track_sequences takes them)."""
    rng = np.random.default_rng(seed)
    gray = np.empty((n_frames, n_seq, rows, cols), np.uint8)
    depth = np.empty((n_frames, n_seq, rows, cols), np.uint16)
    for s in range(n_seq):
        axis = s % 2
        g0, d0 = mid_pyramid_frame(seed + s, rows, cols, intr, axis)
        sign, pos = int(rng.choice([-1, 1])), 0
        for k in range(n_frames):
            gray[k, s] = np.roll(g0, pos, axis=1 - axis)
            depth[k, s] = np.roll(d0, pos, axis=1 - axis)
            pos += sign * int(rng.integers(1, 9))
    return gray, depth


FAMILIES = {"depth_step": depth_step, "invalid_blobs": invalid_blobs, "occluder": occluder, "large_motion": large_motion,
            "brightness_jump": brightness_jump, "saturated": saturated, "mid_pyramid": mid_pyramid, "rank_deficient": rank_deficient}


# ---------------------------------------------------------------------------------------------- the oracle's LM loop, replayed
def _lm_level(k, tmpl, img, xy, iz, jac, model, huber):
    """optimizer::iterative_solve for LMOptimizerState (optimizer.rs:57-70, lm_optimizer.rs:113-192), step by step through the oracle's
    lm_eval / lm_step. -> dict(ok, model, nb_iter, energy, accepted, nan_accepted)."""
    e, _, g, H = O.lm_eval(k, tmpl, img, xy, iz, jac, model, huber_delta=huber)
    e = F32(e)
    lm_coef = F32(0.1)
    nb_iter, accepted, nan_accepted = 0, 0, False
    while True:
        nb_iter += 1
        st, cand, _ = O.lm_step(H, g, model, lm_coef)
        if st != 0:  # "Error at Cholesky decomposition of hessian"
            return dict(ok=False, model=model, nb_iter=nb_iter, energy=e, accepted=accepted, nan_accepted=nan_accepted)
        e2, n2, g2, H2 = O.lm_eval(k, tmpl, img, xy, iz, jac, cand, huber_delta=huber)
        e2 = F32(e2)
        too_many = nb_iter > 20
        if e2 > e:  # Err(energy)
            if too_many:
                break
            lm_coef = F32(lm_coef * F32(10.0))
            continue
        d_energy = F32(e - e2)
        accepted += 1
        nan_accepted |= n2 == 0
        e, g, H, model = e2, g2, H2, cand
        if too_many:
            break
        lm_coef = F32(F32(0.1) * lm_coef)
        if not d_energy > 1.0:
            break
    return dict(ok=True, model=model, nb_iter=nb_iter, energy=e, accepted=accepted, nan_accepted=nan_accepted)


def classify(cfg, kg, kd, cg, init=None):
    """Replay Tracker::track of every pair (inverse_compositional.rs:170-224) level by level. -> dict of per-pair arrays: status,
    models (lm_model after the level loop), nb_iter / energy per level (0 for a failed level and those below it, as the oracle reports
    them), fail_level (-1: none), accepted_in_fail (accepted steps of the failing level), nan_accept (an accepted evaluation with no
    point inside), and the outcome flags o1 / o2 / o3 of the module docstring."""
    n, rows, cols = kg.shape
    L = cfg.nb_levels
    out = {k: np.zeros(n, np.int32) for k in ("status", "fail_level", "accepted_in_fail")}
    out.update(models=np.zeros((n, 7), np.float32), nb_iter=np.zeros((n, L), np.int32), energy=np.zeros((n, L), np.float32),
               nan_accept=np.zeros(n, bool))
    for p in range(n):
        tr = O.Tracker(cfg, 0.0, kd[p], 0.0, kg[p])
        cur = O.mean_pyramid(cg[p], L)
        prev = identity7() if init is None else np.asarray(init[p], np.float32)
        model = O.iso_mul(O.iso_inverse(prev), identity7())
        out["fail_level"][p] = -1
        for lvl in range(L - 1, -1, -1):
            xy, iz, jac = tr.points(lvl)
            _, _, _, k = tr.level(lvl)
            r = _lm_level(k, tr.image(lvl), cur[lvl], xy, iz, jac, model, cfg.huber_delta)
            out["nan_accept"][p] |= r["nan_accepted"]
            if not r["ok"]:
                out["status"][p] = 1
                out["fail_level"][p] = lvl
                out["accepted_in_fail"][p] = r["accepted"]
                break
            model = r["model"]
            out["nb_iter"][p, lvl] = r["nb_iter"]
            out["energy"][p, lvl] = r["energy"]
        out["models"][p] = model
    out["o1"] = (out["fail_level"] >= 0) & (out["fail_level"] < L - 1)
    out["o2"] = (out["fail_level"] >= 0) & (out["accepted_in_fail"] > 0)
    out["o3"] = out["nan_accept"]
    return out


def check_replay(ref, cls):
    """The replay is the oracle: statuses, iteration counts and final models equal oracle.track_pairs' bit for bit."""
    assert (cls["status"] == ref["status"]).all(), "replay: statuses differ from the oracle's"
    assert (cls["nb_iter"] == ref["nb_iter"]).all(), "replay: iteration counts differ from the oracle's"
    assert (cls["models"].view(np.uint32) == ref["models"].view(np.uint32)).all(), "replay: final models differ from the oracle's"


def same_energy(a, b):
    """Per-level energies: a NaN matches a NaN whatever its payload, every other value must match in its bits."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a[~na].view(np.uint32) == b[~nb].view(np.uint32)).all())
