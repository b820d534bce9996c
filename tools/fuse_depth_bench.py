#!/usr/bin/env python3
"""Time vors_batch_fuse_depth (level 0, 640x480, 6 levels, 256 pairs; dense and coarse-to-fine) and write profiles/fuse_depth_summary.md.

Three forms of the pass — the splat alone (d_zkey), splat + merge (d_fused_depth, d_fused_weight), splat + merge + counts — into
preallocated planes, beside two yardsticks on the same handle:
  (a) vors_batch_reproject_depth with d_pred_z + d_pred_depth: the 32-bit z-buffer and its elementwise second kernel;
  (b) the stream fill of the key plane (hipMemsetD32Async over pairs x 640 x 480 x 2 dwords), which the pass issues before its kernel,
      and (b32) the fill of one float plane per pair, which (a) issues.
HIP events around one call; a block = the median of 20 calls after 3 warm-up calls; the blocks of all legs alternate for `--blocks`
rounds, so the figure of a leg is the median of its block medians and its run-to-run spread their range.
The expectation on record (not enforced): the splat costs about the 32-bit pass's own splat plus the doubled fill; what it costs beyond
that is the price of one 64-bit global atomic minimum per landing point instead of a 32-bit one.

  python tools/fuse_depth_bench.py [--pairs N] [--blocks K] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, L, PAIRS = 480, 640, 6, 256
SPLAT, MERGE, COUNTS = "splat alone (d_zkey)", "splat + merge", "splat + merge + counts"
WEIGHTED = "splat + merge + counts, with a weight plane"
YARD_Z, YARD_A = "reproject_depth, d_pred_z alone", "reproject_depth, d_pred_z + d_pred_depth"
YARD_B, YARD_B32 = "stream fill of the key plane", "stream fill of one float plane per pair"


def block(torch, fn, reps=20, warm=3):
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
    return float(np.median(ms))


def measure(a):
    sys.path[:0] = [os.path.join(ROOT, "visual-odometry-rs_amd"), ROOT]
    import torch
    import vors_amd as V
    intr = V.scaled_intrinsics(ROWS, COLS)
    n = a.pairs
    kg, kd, cg, cd, _ = V.synth_render_pairs(0x5EEDB000, n, ROWS, COLS, intr, want_cur_depth=True)
    lib = V.lib()
    fill = lib.hipMemsetD32Async   # the runtime call the pass itself makes, resolved through the library's dependency on the HIP runtime
    fill.argtypes, fill.restype = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p], C.c_int
    shape = (n, ROWS, COLS)
    key = torch.empty(shape, dtype=torch.int64, device="cuda")
    depth = torch.empty(shape, dtype=torch.int16, device="cuda")
    weight = torch.empty(shape, dtype=torch.uint8, device="cuda")
    counts = torch.empty((n, 6), dtype=torch.int32, device="cuda")
    ones = torch.ones(shape, dtype=torch.uint8, device="cuda")
    pz = torch.empty(shape, dtype=torch.float32, device="cuda")
    result = {}
    for mode, mname in ((V.CANDIDATES_DENSE, "dense"), (V.CANDIDATES_COARSE_TO_FINE, "coarse-to-fine")):
        cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, arithmetic=V.ARITH_FUSED)
        b = V.Batch(cfg, n, ROWS, COLS)
        poses = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
        status = torch.zeros(n, dtype=torch.int32, device="cuda")
        stats = V.stats_tensor(n)
        b.track_pairs(kg, kd, cg, poses, status, stats)
        torch.cuda.synchronize()
        st = V.decode_stats(stats)
        lm = torch.from_numpy(st["lm_model"].copy()).cuda()
        stream = lambda: torch.cuda.current_stream().cuda_stream

        def fuse(d=None, w=None, c=None, kw=None):
            p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
            st_ = lib.vors_batch_fuse_depth(b._h, n, p(lm), 0, p(cd), 0.01, p(kw), 255, 1, p(key), p(d), p(w), p(c), C.c_void_p(stream()))
            assert st_ == 0, lib.vors_last_error()

        legs = {
            YARD_B32: lambda: fill(pz.data_ptr(), 0x7f800000, pz.numel(), stream()),
            YARD_B: lambda: fill(key.data_ptr(), -1, 2 * key.numel(), stream()),
            YARD_Z: lambda: b.reproject_depth(0, lm, pred_z=True),
            YARD_A: lambda: b.reproject_depth(0, lm, pred_z=True, pred_depth=True),
            SPLAT: lambda: fuse(),
            MERGE: lambda: fuse(depth, weight),
            COUNTS: lambda: fuse(depth, weight, counts),
            WEIGHTED: lambda: fuse(depth, weight, counts, ones),
        }
        meds = {k: [] for k in legs}
        for r in range(a.blocks):   # alternate the legs: the spread of a leg's block medians is its run-to-run spread in this process
            for k, fn in legs.items():
                meds[k].append(block(torch, fn))
            print(f"{mname}: round {r + 1}/{a.blocks} " + ", ".join(f"{k}: {v[-1]:.3f}" for k, v in meds.items()), file=sys.stderr, flush=True)
        result[mname] = {k: dict(ms=float(np.median(v)), lo=float(np.min(v)), hi=float(np.max(v))) for k, v in meds.items()}
        fuse(depth, weight, counts)
        rc = b.reproject_depth(0, lm, pred_z=False, counts=True)["counts"]
        torch.cuda.synchronize()
        result[mname]["counts"] = counts.cpu().numpy().astype(np.float64).mean(axis=0).tolist()
        result[mname]["points"] = rc.cpu().numpy().astype(np.float64).mean(axis=0).tolist()
        del b
    return result


def fmt(t):
    return f"{t['ms']:.3f} ({t['lo']:.3f}-{t['hi']:.3f})"


def summary(a, res):
    n = a.pairs
    lines = [f"# vors_batch_fuse_depth, level 0, {COLS}x{ROWS}, {L} levels, {n} pairs, one MI355X", "",
             f"HIP events around one call. A block = median of 20 calls after 3 warm-up calls; the blocks of all legs alternate for {a.blocks} rounds:",
             "a figure is the median of a leg's block medians, (lowest-highest) their range = the run-to-run spread inside this process. ms.",
             "The handle is FUSED (the pass does not depend on the handle's arithmetic); models = each pair's lm_model; the current depth is the",
             "rendered one; tol_m = 0.01, max_weight = 255, fill_min_weight = 1; every plane is preallocated.", ""]
    for mname, r in res.items():
        c, pt = r["counts"], r["points"]
        lines += [f"## {mname} (per pair: {pt[0]:.0f} usable points, {pt[1]:.0f} land; pixels: {c[0]:.0f} agree, {c[1]:.0f} + {c[2]:.0f} conflict, "
                  f"{c[3]:.0f} measured only, {c[4]:.0f} filled, {c[5]:.0f} empty)", "", "| leg | ms |", "|---|---|"]
        for k in (SPLAT, MERGE, COUNTS, WEIGHTED, YARD_Z, YARD_A):
            lines.append(f"| {'yardstick (a): ' if k == YARD_A else ''}{k} | {fmt(r[k])} |")
        lines.append(f"| yardstick (b): {YARD_B} ({n * ROWS * COLS * 8 / 1e6:.1f} MB) | {fmt(r[YARD_B])} |")
        lines.append(f"| {YARD_B32} ({n * ROWS * COLS * 4 / 1e6:.1f} MB) | {fmt(r[YARD_B32])} |")
        t = r[SPLAT]["ms"]
        budget = r[YARD_Z]["ms"] - r[YARD_B32]["ms"] + r[YARD_B]["ms"]
        m = pt[1] * n
        lines += ["", f"The splat vs the 32-bit splat with the doubled fill: {t:.3f} vs {r[YARD_Z]['ms']:.3f} - {r[YARD_B32]['ms']:.3f} + {r[YARD_B]['ms']:.3f} "
                  f"= {budget:.3f} ms, ratio **{t / budget:.2f}**; beyond the budget: {t - budget:+.3f} ms for {m / 1e6:.2f} M 64-bit minima"
                  + (f" ({m / (t - budget) / 1e6:.0f} G minima/s if all of it is theirs)." if t > budget else "."),
                  f"The merge: {r[MERGE]['ms'] - t:+.3f} ms over the splat for {n * ROWS * COLS * 14 / 1e6:.0f} MB of plane traffic (8 + 2 B read, 2 + 1 B "
                  f"written per pixel, 1 B more gathered with a weight plane); the counts: {r[COUNTS]['ms'] - r[MERGE]['ms']:+.3f} ms; the second kernel of "
                  f"yardstick (a): {r[YARD_A]['ms'] - r[YARD_Z]['ms']:+.3f} ms.", ""]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_depth_summary.md"))
    ap.add_argument("--pairs", type=int, default=PAIRS)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    text = summary(a, measure(a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
