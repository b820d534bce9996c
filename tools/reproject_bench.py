#!/usr/bin/env python3
"""Time vors_batch_reproject_depth at level 0 (640x480, 6 levels, 256 pairs; dense and coarse-to-fine) and write
profiles/reproject_depth_summary.md.

Three configurations of the pass — d_pred_z alone, d_pred_z + d_pred_depth, all four outputs with a current depth — beside two yardsticks:
  (a) vors_batch_residual_maps with the warp field alone on the same handle: the same loads and per-point arithmetic with plain stores
      for a sink (`--yardstick-only` runs this leg alone, e.g. on the parent commit's library through VORS_HIP_LIB: the entry exists there);
  (b) the stream fill of one float plane per pair (hipMemsetD32Async of pairs x 640 x 480 dwords), which the pass issues before its kernel.
HIP events around one call; a block = the median of 20 calls after 3 warm-up calls; the blocks of all legs alternate for `--blocks`
rounds, so the figure of a leg is the median of its block medians and its run-to-run spread their range.
The expectation on record (not enforced): "d_pred_z alone" costs about (a) + (b); what it costs beyond that is the price of one 32-bit
global atomic minimum per landing point.

  python tools/reproject_bench.py [--parent-json FILE]     the measurement -> profiles/reproject_depth_summary.md
  python tools/reproject_bench.py --yardstick-only [--json FILE]     leg (a) alone -> one JSON line
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, L, PAIRS = 480, 640, 6, 256
CONFIGS = (("d_pred_z alone", dict(pred_z=True), False), ("d_pred_z + d_pred_depth", dict(pred_z=True, pred_depth=True), False),
           ("all four outputs, with a current depth", dict(pred_z=True, pred_depth=True, residual=True, counts=True), True))
YARD_A, YARD_B = "residual_maps, warp field alone", "stream fill of one float plane per pair"


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
    fill = V.lib().hipMemsetD32Async   # the runtime call the pass itself makes, resolved through the library's dependency on the HIP runtime
    fill.argtypes, fill.restype = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p], C.c_int
    plane = torch.empty((n, ROWS, COLS), dtype=torch.float32, device="cuda")
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
        legs = {YARD_A: lambda: b.residual_maps(0, lm, residuals=False, warp=True)}
        if not a.yardstick_only:
            legs[YARD_B] = lambda: fill(plane.data_ptr(), 0x7f800000, plane.numel(), torch.cuda.current_stream().cuda_stream)
            for cname, kw, with_depth in CONFIGS:
                legs[cname] = (lambda kw=kw, with_depth=with_depth: b.reproject_depth(0, lm, cur_depth=cd if with_depth else None, tol_m=0.01,
                                                                                        **{"pred_z": False, **kw}))
        meds = {k: [] for k in legs}
        for r in range(a.blocks):   # alternate the legs: the spread of a leg's block medians is its run-to-run spread in this process
            for k, fn in legs.items():
                meds[k].append(block(torch, fn))
            print(f"{mname}: round {r + 1}/{a.blocks} " + ", ".join(f"{k}: {v[-1]:.3f}" for k, v in meds.items()), file=sys.stderr, flush=True)
        result[mname] = {k: dict(ms=float(np.median(v)), lo=float(np.min(v)), hi=float(np.max(v))) for k, v in meds.items()}
        result[mname]["n_points"] = float(st["n_points"][:, 0].mean())
        if not a.yardstick_only:
            cnt = b.reproject_depth(0, lm, cur_depth=cd, tol_m=0.01, pred_z=False, counts=True)["counts"].cpu().numpy().astype(np.float64)
            result[mname]["counts"] = cnt.mean(axis=0).tolist()
        del b
    return result


def fmt(t):
    return f"{t['ms']:.3f} ({t['lo']:.3f}-{t['hi']:.3f})"


def summary(a, res, parent):
    n = a.pairs
    lines = [f"# vors_batch_reproject_depth, level 0, {COLS}x{ROWS}, {L} levels, {n} pairs, one MI355X", "",
             f"HIP events around one call. A block = median of 20 calls after 3 warm-up calls; the blocks of all legs alternate for {a.blocks} rounds:",
             "a figure is the median of a leg's block medians, (lowest-highest) their range = the run-to-run spread inside this process. ms.",
             "The handle is FUSED (the pass does not depend on the handle's arithmetic); models = each pair's lm_model; the current depth is the",
             "rendered one.", ""]
    for mname, r in res.items():
        ya, yb = r[YARD_A], r[YARD_B]
        c = r["counts"]
        lines += [f"## {mname} (per pair at level 0: {c[0]:.0f} usable points, {c[1]:.0f} land, {c[2]:.0f} on a measured depth, {c[3]:.0f} within 1 cm)", "",
                  "| leg | ms |", "|---|---|"]
        for cname, _, _ in CONFIGS:
            lines.append(f"| {cname} | {fmt(r[cname])} |")
        lines.append(f"| yardstick (a): `vors_batch_residual_maps`, warp field alone | {fmt(ya)} |")
        if parent and mname in parent:
            lines.append(f"| yardstick (a) on the PARENT commit's library (`--yardstick-only`, a process of its own) | {fmt(parent[mname][YARD_A])} |")
        lines.append(f"| yardstick (b): stream fill of one float plane per pair ({n * ROWS * COLS * 4 / 1e6:.1f} MB) | {fmt(yb)} |")
        t = r["d_pred_z alone"]
        budget = ya["ms"] + yb["ms"]
        lines += ["", f"\"d_pred_z alone\" vs (a) + (b): {t['ms']:.3f} vs {ya['ms']:.3f} + {yb['ms']:.3f} = {budget:.3f} ms, ratio **{t['ms'] / budget:.2f}**; "
                  f"beyond the budget: {t['ms'] - budget:+.3f} ms for {c[1] * n / 1e6:.2f} M atomic minima"
                  + (f" ({c[1] * n / max(t['ms'] - budget, 1e-9) / 1e6:.0f} G minima/s if all of it is theirs)." if t["ms"] > budget else "."), ""]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_depth_summary.md"))
    ap.add_argument("--pairs", type=int, default=PAIRS)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--yardstick-only", action="store_true")
    ap.add_argument("--json", default=None, help="where to write the figures as one JSON line")
    ap.add_argument("--parent-json", default=None, help="figures of a --yardstick-only run on the parent commit's library")
    a = ap.parse_args()
    res = measure(a)
    if a.json:
        open(a.json, "w").write(json.dumps(res) + "\n")
    if a.yardstick_only:
        print(json.dumps(res))
        return
    parent = json.load(open(a.parent_json)) if a.parent_json else None
    text = summary(a, res, parent)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
