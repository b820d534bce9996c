#!/usr/bin/env python3
"""Time vors_batch_eval_pairs / vors_batch_pose_information at level 0 (640x480, 6 levels; 4096 pairs, dense 1024) and write
profiles/eval_pairs_summary.md. HIP events around one call after warm-up, median of 20. Two yardsticks from the same process:
(a) the loop of vors_batch_eval_level over 64 pairs (two synchronisations and two allocations per pair), extrapolated to the batch;
(b) the LM stage of one track of the same batch divided by the mean evaluations per pair (sum over levels of nb_iter + 1) — every level,
where the new call evaluates the finest alone. Also: how the covariance is calibrated against the renderer's ground truth (FUSED).
usage: python tools/eval_pairs_bench.py [--out profiles/eval_pairs_summary.md] [--pairs N]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "visual-odometry-rs_amd"), ROOT]
import torch  # noqa: E402
import vors_amd as V  # noqa: E402

ROWS, COLS, L = 480, 640, 6


class Timing(float):
    """The median, with the spread of the repetitions in its text."""

    def __new__(cls, med, lo, hi):
        t = super().__new__(cls, med)
        t.lo, t.hi = lo, hi
        return t

    def __format__(self, spec):
        return f"{float(self):{spec}} ({self.lo:{spec}}-{self.hi:{spec}})"


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return Timing(float(np.median(ms)), float(np.min(ms)), float(np.max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_pairs_summary.md"))
    ap.add_argument("--pairs", type=int, default=0)
    a = ap.parse_args()
    intr = V.scaled_intrinsics(ROWS, COLS)
    lines = ["# vors_batch_eval_pairs / vors_batch_pose_information, level 0, 640x480, 6 levels, one MI355X", "",
             "HIP events around one call, median (fastest-slowest) of 20 after 3 warm-up calls. (a) = loop of `vors_batch_eval_level` over 64 pairs (host wall clock)",
             "extrapolated to the batch; (b) = LM stage of one track / mean evaluations per pair (all levels).", "",
             "| candidates | arithmetic | pairs | FULL K=1 ms | ENERGY K=1 ms | FULL K=8 ms | ENERGY K=8 ms | pose_information ms | (a) ms | (b) ms per batch-evaluation |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    calib = []
    for mode, mname in ((V.CANDIDATES_COARSE_TO_FINE, "coarse-to-fine"), (V.CANDIDATES_DSO, "DSO"), (V.CANDIDATES_DENSE, "dense")):
        n = a.pairs or (1024 if mode == V.CANDIDATES_DENSE else 4096)
        kg, kd, cg, _, gt = V.synth_render_pairs(0x5EEDB000, n, ROWS, COLS, intr)
        for arith, aname in ((V.ARITH_REFERENCE, "REFERENCE"), (V.ARITH_FUSED, "FUSED")):
            cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, arithmetic=arith)
            b = V.Batch(cfg, n, ROWS, COLS)
            b.enable_kernel_timing(4)
            poses = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
            status = torch.zeros(n, dtype=torch.int32, device="cuda")
            stats = V.stats_tensor(n)
            for _ in range(2):
                b.track_pairs(kg, kd, cg, poses, status, stats)
            torch.cuda.synchronize()
            st = V.decode_stats(stats)
            evals = float((st["nb_iter"][:, :L] + (st["nb_iter"][:, :L] > 0)).sum(1).mean())
            lm_ms = b.last_kernel_ms()["lm_ms"]
            lm = torch.from_numpy(st["lm_model"].copy()).cuda()
            m8 = lm[:, None, :].repeat(1, 8, 1).contiguous()
            out1 = torch.empty((n, 1, 29), dtype=torch.float32, device="cuda")
            out8 = torch.empty((n, 8, 29), dtype=torch.float32, device="cuda")
            t = [timed(lambda: b.eval_pairs(0, m, what=w, out=o))
                 for m, o in ((lm, out1), (m8, out8)) for w in ("full", "energy")]
            t_pi = timed(lambda: b.pose_information(0, stats))
            models = st["lm_model"]
            t0 = time.perf_counter()
            for p in range(64):
                b.eval_level(p, 0, models[p], arith)
            t_a = (time.perf_counter() - t0) * 1e3 / 64 * n
            lines.append(f"| {mname} | {aname} | {n} | {t[0]:.3f} | {t[1]:.3f} | {t[2]:.3f} | {t[3]:.3f} | {t_pi:.3f} | {t_a:.0f} | {lm_ms / evals:.3f} "
                         f"({lm_ms:.2f} ms / {evals:.1f}) |")
            assert t[0] < t_a, "the batched call must beat the loop of vors_batch_eval_level"
            if arith == V.ARITH_FUSED:  # calibration: xi = log(gt^-1 * estimate) against cov
                info, cov, s2, flags = (x.cpu().numpy() for x in b.pose_information(0, stats))
                g, status_h = gt.cpu().numpy(), status.cpu().numpy()
                q = []
                for p in range(n):
                    if flags[p] or status_h[p] != 0:
                        continue
                    xi = V.se3_log(V.iso_mul(V.iso_inverse(g[p]), models[p])).astype(np.float64)
                    q.append(xi @ np.linalg.solve(cov[p].astype(np.float64), xi) / 6.0)
                calib.append(f"| {mname} | {len(q)} | {np.median(q):.3g} | {np.percentile(q, 90):.3g} |")
    lines += ["", "(b) is the track's own cost of one evaluation of the whole batch averaged over ALL levels (most of a track's evaluations run on the",
              "coarse levels, which are far cheaper than level 0), so a level-0 evaluation is expected to cost more than (b); it is reported, not gated.", "",
              "## Calibration of the covariance (FUSED, level 0, against the renderer's ground truth)", "",
              "Normalised error `xi^T cov^-1 xi / 6`, `xi = log(gt^-1 * estimate)`: 1 = calibrated, >> 1 = the covariance is over-confident.", "",
              "| candidates | pairs | median | 90th percentile |", "|---|---|---|---|"] + calib
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
