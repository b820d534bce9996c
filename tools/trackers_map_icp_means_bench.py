#!/usr/bin/env python3
"""Time the lock-step trackers with the joint map ICP correction on a voxel-filtered map, the averaged model off and on
(vors_trackers_enable_map_icp_means); append the figures to profiles/trackers_map_icp_means_summary.md.

The set-up of tools/map_icp_bench.py: 64 sequences x 39 frames of 640x480, six levels, coarse-to-fine candidates, FUSED
arithmetic, a level-0 map with normals at (2, 0.05), its joint stage (JOINT) — and the voxel filter of
tools/trackers_map_voxel_stats_bench.py (0.02 m, 2^20 entries). Three legs: the joint correction, the same with the voxels' statistics
(means off: the parent's behaviour and the yardstick of the third), and with the averaged model at --means. MOVING: every sequence
moves, so sequences promote; ms per run of the 38 track calls and the stage's totals. STILL: every frame is frame 0 again, so no
sequence ever promotes: the difference per track call is the price of the launches the stage enqueues unconditionally. HIP events
around the track calls of a run; the runs of the three handles alternate for --blocks rounds after a warm-up; the figure of a leg is
the median of its runs, the range beside it. No threshold is fixed.

  python tools/trackers_map_icp_means_bench.py [--sequences N] [--frames F] [--blocks K] [--means MIN_COUNT,MIN_SPAN] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from map_icp_bench import COLS, JOINT, ROWS  # noqa: E402

LEGS = ("joint", "joint + statistics (means off)", "joint + statistics + means")
VOXEL_M, SLOTS = 0.02, 1 << 20


def measure(a):
    sys.path[:0] = [os.path.join(ROOT, "visual-odometry-rs_amd"), ROOT]
    import torch
    import vors_amd as V
    intr = np.asarray(V.scaled_intrinsics(ROWS, COLS), np.float32)
    n = a.sequences
    seeds = [3000 + s for s in range(n)]
    step = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001])
    moving = [V.synth_render_frames(seeds, [k] * n, [step * (0.5 + 4.0 * s / n) * k for s in range(n)], ROWS, COLS, intr, invalid_percent=2)
              for k in range(a.frames)]
    still = [moving[0]] * a.frames
    cfg = V.Config(nb_levels=6, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=V.CANDIDATES_COARSE_TO_FINE,
                   arithmetic=V.ARITH_FUSED)
    out = {}
    for block in range(a.blocks + 1):   # (block 0 warms up and is not counted)
        for scene, frames in (("moving", moving), ("still", still)):
            for leg in LEGS:
                tr = V.Trackers(cfg, n, ROWS, COLS)
                tr.enable_map(0, 1 << 20, 64)
                tr.enable_map_voxels(VOXEL_M, SLOTS)
                if leg != "joint":
                    tr.enable_map_voxel_stats()
                tr.enable_map_normals(2, 0.05)
                tr.enable_map_icp_joint(**JOINT)
                if leg.endswith("means"):
                    tr.enable_map_icp_means(*a.means)
                tr.init(*frames[0])
                tr.track(*frames[1])   # warm-up of the launch path
                tr.init(*frames[0])
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for k in range(1, a.frames):
                    tr.track(*frames[k])
                e1.record()
                e1.synchronize()
                if block:
                    r = out.setdefault((scene, leg), dict(ms=[]))
                    r["ms"].append(e0.elapsed_time(e1))
                    r["promotions"] = int((tr.map()["n_segments"].cpu().numpy() - 1).sum())
                    r["totals"] = tr.map_icp()["totals"].cpu().numpy().sum(axis=0).tolist()
                    r["bytes"] = tr.workspace_bytes()
                del tr
    return out, torch.cuda.get_device_name(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--frames", type=int, default=39)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--means", default="2,1", help="MIN_COUNT,MIN_SPAN of the third leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trackers_map_icp_means_summary.md"))
    a = ap.parse_args()
    a.means = tuple(int(x) for x in a.means.split(","))
    out, device = measure(a)
    calls = a.frames - 1
    lines = ["", "## Cost of the averaged model", "",
             f"`python tools/trackers_map_icp_means_bench.py --sequences {a.sequences} --frames {a.frames} --blocks {a.blocks} --means "
             f"{a.means[0]},{a.means[1]}` on {device}: {a.sequences} sequences of {COLS}x{ROWS}, six levels, coarse-to-fine FUSED, a level-0 map of "
             f"2^20 ranks with {VOXEL_M} m voxels in {SLOTS} entries and normals at (2, 0.05); joint stage {JOINT}; medians of {a.blocks} alternating "
             f"runs of {calls} track calls after one warm-up round (range in brackets). The yardstick of the third leg is the second of the same "
             "session.", "",
             "| scene | leg | ms per run | range, ms | frames/s | ms per track call | promotions | attempted, accepted | workspace, MiB |",
             "|---|---|---|---|---|---|---|---|---|"]
    med = lambda scene, leg: float(np.median(out[(scene, leg)]["ms"]))
    for scene in ("moving", "still"):
        for leg in LEGS:
            r, m = out[(scene, leg)], med(scene, leg)
            lines.append(f"| {scene} | {leg} | {m:.3f} | {min(r['ms']):.3f} .. {max(r['ms']):.3f} | {a.sequences * calls / m * 1e3:.0f} | {m / calls:.4f} | "
                         f"{r['promotions']} | {r['totals']} | {r['bytes'] / 2 ** 20:.1f} |")
    lines += ["", f"Means on against means off, ms per track call: still scene (nothing promotes: the memset and the launch every call enqueues) "
              f"{(med('still', LEGS[2]) - med('still', LEGS[1])) / calls:+.4f}; moving scene {(med('moving', LEGS[2]) - med('moving', LEGS[1])) / calls:+.4f} "
              f"(ratio of the runs {med('moving', LEGS[2]) / med('moving', LEGS[1]):.4f}; the corrections accepted differ, and with them the maps)."]
    text = "\n".join(lines) + "\n"
    with open(a.out, "a") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
