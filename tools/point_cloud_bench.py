#!/usr/bin/env python3
"""Time vors_batch_point_cloud at level 0 (640x480, 6 levels, 256 pairs; dense and coarse-to-fine) and write
profiles/point_cloud_summary.md.

Three configurations of the pass — counts only, xyz + pixel, everything with a half-ones mask — beside two yardsticks on the same handle in
the same run:
  (a) vors_batch_residual_maps with the warp field alone: the same source loads and per-point work with plain stores for a sink;
  (b) a device-to-device copy (torch's copy_ of a contiguous tensor) of exactly the bytes the configuration writes: the floor for its stores.
HIP events around one call; a block = the median of 20 calls after 3 warm-up calls; the blocks of all legs alternate for `--blocks` rounds,
so the figure of a leg is the median of its block medians and its run-to-run spread their range.
The expectation on record (not a gate): "xyz + pixel" costs about (a) + the counting sweep ("counts only", a second read of the keyframe
side) + (b).

  python tools/point_cloud_bench.py             the measurement -> profiles/point_cloud_summary.md
  ... --trace                                   also one rocprofv3 --kernel-trace --stats run of the same legs (a child process of its own)
  ... --measure-only                            run the legs and print the figures as one JSON line (what the profiler traces)
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
CONFIGS = (("counts only", dict(xyz=False, pixel=False, gray=False), False), ("xyz + pixel", dict(xyz=True, pixel=True, gray=False), False),
           ("everything, half-ones mask", dict(xyz=True, pixel=True, gray=True), True))
WARP = "residual_maps, warp field alone"


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
    kg, kd, cg, _, _ = V.synth_render_pairs(0x5EEDB000, n, ROWS, COLS, intr)
    plane = ROWS * COLS
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    keep = (torch.rand((n, ROWS, COLS), device="cuda", generator=gen) < 0.5).to(torch.uint8)
    result = {}
    for mode, mname in ((V.CANDIDATES_DENSE, "dense"), (V.CANDIDATES_COARSE_TO_FINE, "coarse-to-fine")):
        cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, arithmetic=V.ARITH_FUSED)
        b = V.Batch(cfg, n, ROWS, COLS)
        poses = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
        status = torch.zeros(n, dtype=torch.int32, device="cuda")
        stats = V.stats_tensor(n)
        b.track_pairs(kg, kd, cg, poses, status, stats)   # the warp-field yardstick needs a tracked handle; the pass itself does not
        torch.cuda.synchronize()
        lm = torch.from_numpy(V.decode_stats(stats)["lm_model"].copy()).cuda()
        bufs = dict(xyz=torch.empty((n, plane, 3), dtype=torch.float32, device="cuda"), pixel=torch.empty((n, plane), dtype=torch.int32, device="cuda"),
                    gray=torch.empty((n, plane), dtype=torch.uint8, device="cuda"), counts=torch.empty(n, dtype=torch.int32, device="cuda"))
        legs = {WARP: lambda: b.residual_maps(0, lm, residuals=False, warp=True)}
        written = {}
        for cname, kw, masked in CONFIGS:
            args = {k: (bufs[k] if v else False) for k, v in kw.items()}
            fn = (lambda args=args, masked=masked: b.point_cloud(0, poses=lm, keep=keep if masked else None, counts=bufs["counts"], **args))
            fn()
            torch.cuda.synchronize()
            pts = int(bufs["counts"].sum().item())   # the pass writes its points, not the capacity
            written[cname] = pts * (12 * kw["xyz"] + 4 * kw["pixel"] + 1 * kw["gray"]) + 4 * n
            legs[cname] = fn
            words = max(written[cname] // 4, 1)
            src, dst = torch.zeros(words, dtype=torch.float32, device="cuda"), torch.empty(words, dtype=torch.float32, device="cuda")
            legs["copy of the bytes of: " + cname] = (lambda src=src, dst=dst: dst.copy_(src))
        meds = {k: [] for k in legs}
        for _ in range(a.blocks):   # alternate the legs: the spread of a leg's block medians is its run-to-run spread in this process
            for k, fn in legs.items():
                meds[k].append(block(torch, fn))
        result[mname] = {k: dict(ms=float(np.median(v)), lo=float(np.min(v)), hi=float(np.max(v))) for k, v in meds.items()}
        result[mname]["bytes"] = written
        b.point_cloud(0, xyz=False, pixel=False, counts=bufs["counts"])
        result[mname]["n_points"] = float(bufs["counts"].float().mean().item())
        del b
    return result


def kernel_trace(a):
    """One rocprofv3 --kernel-trace --stats run of this script's measurement (a fresh child process) -> rows (kernel, calls, total ms, mean us)."""
    exe = shutil.which("rocprofv3")
    if not exe:
        return None, "rocprofv3 is not on PATH"
    out = tempfile.mkdtemp(prefix="pcloud_trace_", dir=a.trace_dir)
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
        return None, "no kernel_stats.csv under the profiler's output"
    if not a.trace_dir:
        shutil.rmtree(out, ignore_errors=True)
    return sorted(rows, key=lambda x: -x[2]), None


def fmt(t):
    return f"{t['ms']:.3f} ({t['lo']:.3f}-{t['hi']:.3f})"


def summary(a, res, trace, trace_err):
    n = a.pairs
    lines = [f"# vors_batch_point_cloud, level 0, {COLS}x{ROWS}, {L} levels, {n} pairs, one MI355X", "",
             f"HIP events around one call. A block = median of 20 calls after 3 warm-up calls; the blocks of all legs alternate for {a.blocks} rounds:",
             "a figure is the median of a leg's block medians, (lowest-highest) their range = the run-to-run spread inside this process. ms.",
             "The handle is FUSED (the pass does not depend on the handle's arithmetic); poses = each pair's lm_model; capacity = the level's pixels.", ""]
    for mname, r in res.items():
        w = r[WARP]
        lines += [f"## {mname} ({r['n_points']:.0f} usable points per pair at level 0)", "",
                  "| leg | bytes written | ms | copy of those bytes, ms |", "|---|---|---|---|"]
        for cname, _, _ in CONFIGS:
            t, c = r[cname], r["copy of the bytes of: " + cname]
            lines.append(f"| {cname} | {r['bytes'][cname] / 1e6:.2f} MB | {fmt(t)} | {fmt(c)} |")
        lines.append(f"| yardstick (a): `vors_batch_residual_maps`, warp field alone | {n * ROWS * COLS * 8 / 1e6:.1f} MB | {fmt(w)} | |")
        t, cnt, c = r["xyz + pixel"], r["counts only"], r["copy of the bytes of: xyz + pixel"]
        budget = w["ms"] + cnt["ms"] + c["ms"]
        ratio = t["ms"] / budget
        lines += ["", f"Expectation on record (not a gate) \"xyz + pixel ~ (a) + counts only + copy floor\": {t['ms']:.3f} vs {w['ms']:.3f} + {cnt['ms']:.3f} + "
                  f"{c['ms']:.3f} = {budget:.3f} ms: {ratio:.2f} x the sum" + (" — **MORE THAN TWICE the sum**, see the kernel trace." if ratio > 2 else "."), ""]
    lines += ["## Kernel trace (`rocprofv3 --kernel-trace --stats`, one round of the same legs in a process of its own)", ""]
    if trace:
        lines += ["| kernel | calls | total ms | mean us |", "|---|---|---|---|"]
        lines += [f"| `{k[:150]}` | {c} | {tot:.2f} | {mean:.1f} |" for k, c, tot, mean in trace[:12]]
    else:
        lines.append(f"not collected: {trace_err}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_cloud_summary.md"))
    ap.add_argument("--pairs", type=int, default=PAIRS)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--measure-only", action="store_true", help="run the legs and print the figures (what the profiler traces)")
    ap.add_argument("--trace", action="store_true", help="also collect a kernel trace with rocprofv3")
    ap.add_argument("--trace-dir", default=None, help="keep the profiler's output under this directory")
    a = ap.parse_args()
    res = measure(a)
    if a.measure_only:
        print(json.dumps(res))
        return
    trace, err = kernel_trace(a) if a.trace else (None, "--trace was not given")
    text = summary(a, res, trace, err)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
