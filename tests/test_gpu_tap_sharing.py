"""The dense FUSED evaluation at models where the pixels of a quad can NOT share their tap loads. GPU only.

In its ENERGY-ONLY evaluations fused_stage_b (G = 4) fetches the bilinear taps of the pixel pairs (0, 1) and (2, 3) of a quad with one
unaligned 32-bit gather per row whenever both pixels are inside, on the same row of the current image and at most two columns apart;
every other pair falls back to the second pixel's own 16-bit gathers. The bench scenes (motion of a few centimetres) almost never leave
the shared form, so this file drives the evaluation with models that do, in every way:

  * rotations about the optical axis of 0.05 and 0.3 rad: the pairs of most quads cross a row;
  * forward / backward translations that scale the image by ~0.6, ~1.6 and ~2.2: column distances 0, 1, 2 and MORE than 2 on one row;
  * shifts that push quads over the right / bottom (and left / top) limits of the strict window: one pixel of a pair outside;
  * the LAST pair of the batch at the LAST level and at level 0: the reads nearest to the end of the allocations;
  * a 324 x 244 image: level 0 runs the quads, level 1 (162 wide, not a multiple of 4) the one-pixel source.

Two entries, both pinned to what the PARENT of this change computed on an MI355X (tests/golden/tap_sharing/sums.npz, written by
tools/make_tap_sharing_golden.py together with the models) — the loaded bytes are the same bytes, so EQUALITY OF BITS:

  * test_tracking_from_hostile_initial_models: vors_batch_track_pairs started from those models (prev_poses7). Every LM iteration
    evaluates its candidate ENERGY-ONLY — in lm_split_eval_kernel's rounds at the levels of >= 64 Ki pixels, in lm_track_kernel below —
    so this is where the shared fetch and its fall-back run at hostile models. Poses, statuses and the raw per-pair statistics
    (energies, models, iteration and evaluation counts per level).
  * test_fused_sums_...: vors_batch_eval_level, one FULL evaluation per case: the 29 sums, and the same cases against the EXACT arithmetic
    with the bound tests/test_gpu_parity.py puts on sums (SUM_RTOL relative to the largest entry of e, n, g, H), so the fixture cannot
    hide an error that was there when it was recorded. (Measured on the parent: every case within 1.6e-5. The scale-1.6 model at level 2
    of the 320 x 240 shape — 1728 points, not among the cases — gave 2.31e-5 for g on the parent and is why levels 0 and 1 are used.)
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from test_gpu_parity import SUM_RTOL, rel_close

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "tap_sharing", "sums.npz")

# the synthetic scene is a plane ~2 m in front of the camera: t_z = +1.33 m scales the image by ~0.6, -0.75 m by ~1.6, -1.1 m by ~2.2;
# twists are (v, w) as vors_se3_exp takes them, applied on top of the pair's true motion
TWISTS = {
    "truth": (0, 0, 0, 0, 0, 0),
    "roll_0.05": (0, 0, 0, 0, 0, 0.05),
    "roll_0.3": (0, 0, 0, 0, 0, 0.3),
    "scale_0.6": (0, 0, 1.33, 0, 0, 0),
    "scale_1.6": (0, 0, -0.75, 0, 0, 0),
    "scale_2.2": (0, 0, -1.1, 0, 0, 0),
    "shift_right_down": (0.013, 0.011, 0, 0, 0, 0),
    "shift_left_up": (-0.019, -0.006, 0, 0, 0, 0),
}
# shape name -> (rows, cols, levels, pairs, seed). "quads": every level is a multiple of 4 wide over a finer level a multiple of 8 wide;
# "mixed": level 0 is, level 1 (162 wide) is not; "rounds": the headline shape, whose levels 0 and 1 run in evaluation rounds
SHAPES = {"quads": (240, 320, 5, 3, 0x5EED7A00), "mixed": (244, 324, 3, 2, 0x5EED7A01), "rounds": (480, 640, 6, 8, 0x5EED7A02),
          "quads8": (240, 320, 5, 8, 0x5EED7A03)}
HOSTILE = ("roll_0.05", "roll_0.3", "scale_0.6", "scale_1.6", "scale_2.2", "shift_right_down", "shift_left_up")
CASES = ([("quads", 0, lvl, tw) for lvl in (0, 1) for tw in HOSTILE]
         + [("quads", 2, 4, tw) for tw in ("truth", "roll_0.05", "shift_right_down")] + [("quads", 2, 0, "shift_right_down")]
         + [("mixed", 1, lvl, tw) for lvl in (0, 1) for tw in ("roll_0.05", "shift_right_down")])
TRACKED = ("rounds", "quads8")  # pair p starts from HOSTILE[p] (the eighth pair from the truth)


def case_id(case):
    shape, pair, lvl, tw = case
    return f"{shape}-pair{pair}-level{lvl}-{tw}"


def render(shape):
    rows, cols, L, n, seed = SHAPES[shape]
    intr = V.scaled_intrinsics(rows, cols)
    kg, kd, cg, _, gt = V.synth_render_pairs(seed, n, rows, cols, intr)
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=V.CANDIDATES_DENSE,
                   arithmetic=V.ARITH_FUSED)
    return V.Batch(cfg, n, rows, cols), (kg, kd, cg), gt.cpu().numpy()


def track(b, frames, prev=None):
    """vors_batch_track_pairs -> poses [n, 7], status [n], the raw bytes of the n vors_pair_stats."""
    import torch
    n = frames[0].shape[0]
    poses = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    stats = V.stats_tensor(n)
    b.track_pairs(*frames, poses, status, stats, prev_poses7=None if prev is None else torch.from_numpy(prev).cuda())
    torch.cuda.synchronize()
    return poses.cpu().numpy(), status.cpu().numpy(), stats.cpu().numpy()


class Handles:
    """One dense FUSED handle per shape with its pairs tracked (vors_batch_eval_level needs both pyramids), and the true motions."""

    def __init__(self):
        self.h = {}

    def get(self, shape):
        if shape not in self.h:
            b, frames, gt = render(shape)
            track(b, frames)
            self.h[shape] = (b, gt, frames)
        return self.h[shape]


@pytest.fixture(scope="module")
def handles():
    h = Handles()
    yield h
    h.h.clear()


def hostile_model(gt_pair, tw):
    return V.iso_mul(gt_pair, V.se3_exp(np.array(TWISTS[tw], np.float32)))


def model_of(handles, case):
    shape, pair, _, tw = case
    return hostile_model(handles.get(shape)[1][pair], tw)


def sums29(handles, case, model, arith):
    """The 29 sums (sum r^2, n_inside, g[6], H upper triangle[21]) as one float32 vector."""
    shape, pair, lvl, _ = case
    e, n, g, H = handles.get(shape)[0].eval_level(pair, lvl, model, arith)
    return np.concatenate([np.array([e, n], np.float32), g, H[np.triu_indices(6)]]).astype(np.float32)


def hostile_priors(gt):
    """prev_poses7 of a batch: the tracker's initial guess is the inverse of the pose it is given (inverse_compositional.rs:177)."""
    tws = HOSTILE + ("truth",)
    return np.stack([V.iso_inverse(hostile_model(gt[p], tws[p % len(tws)])) for p in range(len(gt))]).astype(np.float32)


@pytest.mark.parametrize("shape", TRACKED)
def test_tracking_from_hostile_initial_models(shape):
    gold = np.load(GOLDEN)
    b, frames, gt = render(shape)
    prev = gold["prev__" + shape]
    assert np.abs(prev - hostile_priors(gt)).max() < 1e-6, "the fixture's initial models are not this shape's"
    poses, status, stats = track(b, frames, prev)
    L = SHAPES[shape][2]
    st = np.frombuffer(stats.tobytes(), V.PAIR_STATS_DTYPE)
    print(f"[{shape}] status {status.tolist()} iterations per level {st['nb_iter'][:, :L].tolist()}")
    assert (st["nb_iter"][:, :L].sum(axis=1) >= L).all(), "every pair must iterate (its candidates are the energy-only evaluations)"
    assert (status == gold["status__" + shape]).all()
    assert (poses.view(np.uint32) == gold["poses__" + shape].view(np.uint32)).all(), "poses differ from the recorded bits"
    assert (stats == gold["stats__" + shape]).all(), "per-pair statistics differ from the recorded bytes"


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_fused_sums_are_the_recorded_bits_and_within_the_parity_bound_of_exact(handles, case):
    gold = np.load(GOLDEN)
    model = gold["model__" + case_id(case)]
    assert np.abs(model - model_of(handles, case)).max() < 1e-6, "the fixture's model is not this case's model"
    fused = sums29(handles, case, model, V.ARITH_FUSED)
    exact = sums29(handles, case, model, V.ARITH_EXACT)
    want = gold["sums__" + case_id(case)]
    scale = lambda a: max(float(np.abs(a).max()), 1e-30)
    print(f"[{case_id(case)}] n_inside fused {int(fused[1])} exact {int(exact[1])}; fused vs exact / largest entry: "
          f"e {abs(float(fused[0]) - float(exact[0])) / scale(exact[0:1]):.2e} g {np.abs(fused[2:8] - exact[2:8]).max() / scale(exact[2:8]):.2e} "
          f"H {np.abs(fused[8:] - exact[8:]).max() / scale(exact[8:]):.2e}; words differing from the fixture: "
          f"{int((fused.view(np.uint32) != want.view(np.uint32)).sum())} of 29")
    assert fused[1] > 100, "the case must keep points inside"
    assert (fused.view(np.uint32) == want.view(np.uint32)).all(), f"FUSED sums differ from the recorded ones: {fused} vs {want}"
    assert rel_close(fused[1], exact[1], SUM_RTOL) and rel_close(fused[0], exact[0], SUM_RTOL)
    assert rel_close(fused[2:8], exact[2:8], SUM_RTOL)
    assert rel_close(fused[8:], exact[8:], SUM_RTOL)
