#!/usr/bin/env python3
"""Time the lock-step trackers with the depth filter off and on and write profiles/trackers_depth_filter_summary.md.

640x480, 6 levels, 64 sequences x 39 tracked frames (40 rendered), FUSED arithmetic, the three candidate modes. A block = one whole
sequence run (init + 39 tracks) on a fresh handle, timed with HIP events around the 39 tracks; the blocks of the two legs (filter off,
filter on) alternate for `--blocks` rounds after one warm-up run of each, so the figure of a leg is the median of its blocks and its
run-to-run spread their range. No cost target: the yardstick of the filter is the filter-off figure of the same run. The expectation on
record (not enforced): the depth-fusion pass over the promoted share of the sequences, plus the masked fill and the staging copies.

  python tools/trackers_depth_filter_bench.py [--sequences N] [--frames F] [--blocks K] [--tol-m T] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, L = 480, 640, 6
BLOCKY = 1 << 63


def render(V, torch, n_seq, n_frames, blocky):
    intr = V.scaled_intrinsics(ROWS, COLS)
    base = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001])
    rng = np.random.default_rng(7)
    speed = 0.35 + 1.3 * rng.random(n_seq)   # some sequences switch keyframes every few frames, some hardly ever
    sign = rng.choice([-1.0, 1.0], size=(n_seq, 6))
    frames = [V.synth_render_frames([(BLOCKY if blocky else 0) | (1000 + s) for s in range(n_seq)], [k] * n_seq,
                                    [base * sign[s] * speed[s] * k for s in range(n_seq)], ROWS, COLS, intr) for k in range(n_frames)]
    torch.cuda.synchronize()
    return frames


def one_run(V, torch, cfg, frames, n_seq, depth_filter):
    """-> (ms of the tracked frames, sequences whose keyframe is no longer the init frame)"""
    tr = V.Trackers(cfg, n_seq, ROWS, COLS)
    if depth_filter is not None:
        tr.enable_depth_filter(*depth_filter)
    tr.init(*frames[0])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for g, d in frames[1:]:
        tr.track(g, d)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), int((tr.current_frames()[2] > 0).sum())


def measure(a):
    sys.path[:0] = [os.path.join(ROOT, "visual-odometry-rs_amd"), ROOT]
    import torch
    import vors_amd as V
    intr = V.scaled_intrinsics(ROWS, COLS)
    result = {}
    for mode, mname in ((V.CANDIDATES_COARSE_TO_FINE, "coarse-to-fine"), (V.CANDIDATES_DENSE, "dense"), (V.CANDIDATES_DSO, "DSO")):
        frames = render(V, torch, a.sequences, a.frames, mode == V.CANDIDATES_DSO)
        cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, arithmetic=V.ARITH_FUSED)
        legs = {"filter off": None, "filter on": (a.tol_m, 255, 0)}
        ms = {k: [] for k in legs}
        moved = {}
        for k, f in legs.items():
            one_run(V, torch, cfg, frames, a.sequences, f)   # warm-up
        for _ in range(a.blocks):
            for k, f in legs.items():
                t, moved[k] = one_run(V, torch, cfg, frames, a.sequences, f)
                ms[k].append(t)
        result[mname] = {k: (float(np.median(v)), float(min(v)), float(max(v)), moved[k]) for k, v in ms.items()}
        del frames
        torch.cuda.empty_cache()
    return result, torch.cuda.get_device_name(0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sequences", type=int, default=64)
    p.add_argument("--frames", type=int, default=40, help="rendered frames per sequence (the first one initialises)")
    p.add_argument("--blocks", type=int, default=5)
    p.add_argument("--tol-m", type=float, default=0.02)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "trackers_depth_filter_summary.md"))
    a = p.parse_args()
    result, device = measure(a)
    tracked = a.sequences * (a.frames - 1)
    lines = ["# Sequence trackers: frames per second with the depth filter off and on", "",
             f"`tools/trackers_depth_filter_bench.py` on {device}: {COLS}x{ROWS}, {L} levels, {a.sequences} sequences x {a.frames - 1} tracked frames, "
             f"FUSED arithmetic, tol_m = {a.tol_m}; HIP events around the tracked frames of a run, {a.blocks} alternating blocks per leg, "
             "median (min .. max).", "",
             "| candidates | leg | ms per run | frames per second | sequences that promoted at least once |", "|---|---|---|---|---|"]
    for mname, legs in result.items():
        for k, (med, lo, hi, moved) in legs.items():
            lines.append(f"| {mname} | {k} | {med:.2f} ({lo:.2f} .. {hi:.2f}) | {tracked / med * 1e3:.0f} ({tracked / hi * 1e3:.0f} .. {tracked / lo * 1e3:.0f}) | {moved} of {a.sequences} |")
        off, on = legs["filter off"][0], legs["filter on"][0]
        lines.append(f"| {mname} | on / off | {on / off:.3f} | | |")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
