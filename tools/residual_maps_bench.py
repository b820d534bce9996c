#!/usr/bin/env python3
"""Time vors_batch_residual_maps at level 0 (640x480, 6 levels, 256 pairs; dense and coarse-to-fine) and write
profiles/residual_maps_summary.md.

Three configurations of the pass — residuals only, all four outputs, histogram only — beside two yardsticks on the same handle:
  (a) vors_batch_eval_pairs, EXACT, VORS_EVAL_ENERGY, one model per pair: the same per-point arithmetic with two sums for a sink;
  (b) a device-to-device copy (hipMemcpyAsync; torch's copy_ of a contiguous tensor) of exactly the bytes the configuration writes:
      the floor for its stores.
HIP events around one call; a block = the median of 20 calls after 3 warm-up calls; the blocks of all configurations alternate for
`--blocks` rounds, so the figure of a configuration is the median of its block medians and its run-to-run spread their range.
The expectation on record: "residuals only" costs no more than (a) + (b), to within the spread.

  python tools/residual_maps_bench.py                      the whole measurement + one rocprofv3 --kernel-trace --stats run of the same
                                                           script (a child process of its own) -> profiles/residual_maps_summary.md
  python tools/residual_maps_bench.py --yardstick-only [--package DIR] [--json FILE]
                                                           leg (a) alone, on the vors_amd package under DIR (another build of the
                                                           library, e.g. the parent commit's: the entry exists there) -> one JSON line
  ... --parent-json FILE                                   put the figures of such a run beside this build's in the summary
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, L, PAIRS = 480, 640, 6, 256
CONFIGS = (("residuals only", dict(residuals=True)), ("all four outputs", dict(residuals=True, warp=True, hist=True, scale=True)),
           ("histogram only", dict(residuals=False, hist=True)))


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


def bytes_written(kw, n):
    plane = ROWS * COLS
    return n * (4 * plane * bool(kw.get("residuals")) + 8 * plane * bool(kw.get("warp")) + 1024 * bool(kw.get("hist") or kw.get("scale"))
                + 8 * bool(kw.get("scale")))


def measure(a):
    sys.path[:0] = [a.package or os.path.join(ROOT, "visual-odometry-rs_amd"), ROOT]
    import torch
    import vors_amd as V
    intr = V.scaled_intrinsics(ROWS, COLS)
    n = a.pairs
    kg, kd, cg, _, _ = V.synth_render_pairs(0x5EEDB000, n, ROWS, COLS, intr)
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
        out29 = torch.empty((n, 1, 29), dtype=torch.float32, device="cuda")
        legs = {"eval_pairs EXACT ENERGY": lambda: b.eval_pairs(0, lm, arithmetic=V.ARITH_EXACT, what="energy", out=out29)}
        if not a.yardstick_only:
            for cname, kw in CONFIGS:
                legs[cname] = (lambda kw=kw: b.residual_maps(0, lm, **{"residuals": False, **kw}))
                words = bytes_written(kw, n) // 4
                src, dst = torch.zeros(words, dtype=torch.float32, device="cuda"), torch.empty(words, dtype=torch.float32, device="cuda")
                legs["copy of the bytes of: " + cname] = (lambda src=src, dst=dst: dst.copy_(src))
        meds = {k: [] for k in legs}
        for _ in range(a.blocks):   # alternate the legs: the spread of a leg's block medians is its run-to-run spread in this process
            for k, fn in legs.items():
                meds[k].append(block(torch, fn))
        result[mname] = {k: dict(ms=float(np.median(v)), lo=float(np.min(v)), hi=float(np.max(v))) for k, v in meds.items()}
        result[mname]["n_points"] = float(st["n_points"][:, 0].mean())
        del b
    return result


def kernel_trace(a):
    """One rocprofv3 --kernel-trace --stats run of this script's measurement (a fresh child process) -> rows (kernel, calls, total ms, mean us)."""
    exe = shutil.which("rocprofv3")
    if not exe:
        return None, "rocprofv3 is not on PATH"
    out = tempfile.mkdtemp(prefix="rmaps_trace_", dir=a.trace_dir)
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--measure-only",
           "--blocks", "1", "--pairs", str(a.pairs)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        return None, f"rocprofv3 exited with {r.returncode}: {r.stderr[-400:]}"
    rows = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            try:
                rows.append((row["Name"], int(row["Calls"]), float(row["TotalDurationNs"]) / 1e6, float(row["AverageNs"]) / 1e3))
            except (KeyError, ValueError):
                return None, f"unexpected columns in {os.path.basename(f)}: {list(row)}"
    if not rows:
        return None, f"no kernel_stats.csv under the profiler's output ({[os.path.relpath(f, out) for f in glob.glob(os.path.join(out, '**', '*'), recursive=True)][:8]})"
    if not a.trace_dir:
        shutil.rmtree(out, ignore_errors=True)
    return sorted(rows, key=lambda x: -x[2]), None


def fmt(t):
    return f"{t['ms']:.3f} ({t['lo']:.3f}-{t['hi']:.3f})"


def summary(a, res, parent, trace, trace_err):
    n = a.pairs
    lines = [f"# vors_batch_residual_maps, level 0, {COLS}x{ROWS}, {L} levels, {n} pairs, one MI355X", "",
             f"HIP events around one call. A block = median of 20 calls after 3 warm-up calls; the blocks of all legs alternate for {a.blocks} rounds:",
             "a figure is the median of a leg's block medians, (lowest-highest) their range = the run-to-run spread inside this process. ms.",
             "The handle is FUSED (the pass does not depend on the handle's arithmetic); models = each pair's lm_model.", ""]
    for mname, r in res.items():
        e = r["eval_pairs EXACT ENERGY"]
        lines += [f"## {mname} ({r['n_points']:.0f} usable points per pair at level 0)", "",
                  "| leg | bytes written | ms | copy of those bytes, ms | GB/s of the stores |", "|---|---|---|---|---|"]
        for cname, kw in CONFIGS:
            t, c, bw = r[cname], r["copy of the bytes of: " + cname], bytes_written(kw, n)
            lines.append(f"| {cname} | {bw / 1e6:.1f} MB | {fmt(t)} | {fmt(c)} | {bw / t['ms'] / 1e6:.0f} |")
        lines.append(f"| yardstick (a): `vors_batch_eval_pairs` EXACT, ENERGY | {n * 116 / 1e6:.2f} MB | {fmt(e)} | | |")
        if parent and mname in parent:
            lines.append(f"| yardstick (a) on the PARENT commit's library (the tool's `--yardstick-only` leg, a process of its own) | | {fmt(parent[mname]['eval_pairs EXACT ENERGY'])} | | |")
        t, c = r["residuals only"], r["copy of the bytes of: residuals only"]
        budget = e["ms"] + c["ms"]
        spread = (t["hi"] - t["lo"]) + (e["hi"] - e["lo"]) + (c["hi"] - c["lo"])
        verdict = "MET" if t["ms"] <= budget + spread else f"NOT MET: {t['ms'] - budget:.3f} ms ({(t['ms'] / budget - 1) * 100:.0f} %) above"
        lines += ["", f"Expectation \"residuals only <= (a) + copy floor\": {t['ms']:.3f} vs {e['ms']:.3f} + {c['ms']:.3f} = {budget:.3f} ms, margin (sum of the three "
                  f"spreads) {spread:.3f} ms: **{verdict}**.",
                  f"Histogram: \"histogram only\" costs {r['histogram only']['ms'] / e['ms']:.2f} x yardstick (a); \"all four\" costs "
                  f"{r['all four outputs']['ms'] - r['residuals only']['ms']:.3f} ms more than \"residuals only\" for "
                  f"{(bytes_written(CONFIGS[1][1], n) - bytes_written(CONFIGS[0][1], n)) / 1e6:.1f} MB more.", ""]
    lines += ["## Kernel trace (`rocprofv3 --kernel-trace --stats`, one round of the same legs in a process of its own; tracing slows the host, not the kernels)", ""]
    if trace:
        lines += ["| kernel | calls | total ms | mean us |", "|---|---|---|---|"]
        lines += [f"| `{k[:150]}` | {c} | {tot:.2f} | {mean:.1f} |" for k, c, tot, mean in trace[:14]]
    else:
        lines.append(f"not collected: {trace_err}")
    lines += ["", "## Histogram form", "",
              "Kept: one 256-bin sub-histogram per wavefront in LDS (4 x 1 KiB per workgroup, `atomicAdd` on LDS), summed by one thread per bin and flushed with one global",
              "integer `atomicAdd` per non-empty bin and workgroup into an array zeroed on the stream. The figures above are its evidence: what the histogram adds is the",
              "difference between \"histogram only\" and yardstick (a), which runs the same loads and arithmetic with two sums for a sink. No other form was measured.", ""]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_maps_summary.md"))
    ap.add_argument("--pairs", type=int, default=PAIRS)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--yardstick-only", action="store_true")
    ap.add_argument("--measure-only", action="store_true", help="run the legs and print the figures (what the profiler traces)")
    ap.add_argument("--package", default=None, help="directory that holds the vors_amd package to measure (default: this tree's)")
    ap.add_argument("--json", default=None, help="with --yardstick-only: where to write the figures")
    ap.add_argument("--parent-json", default=None, help="figures of a --yardstick-only run on the parent commit's library")
    ap.add_argument("--trace-dir", default=None, help="keep the profiler's output under this directory")
    a = ap.parse_args()
    res = measure(a)
    if a.yardstick_only or a.measure_only:
        print(json.dumps(res))
        if a.json:
            open(a.json, "w").write(json.dumps(res) + "\n")
        return
    parent = json.load(open(a.parent_json)) if a.parent_json else None
    trace, err = kernel_trace(a)
    text = summary(a, res, parent, trace, err)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
