#!/usr/bin/env python3
"""Time the sensor front end — vors_undistort_frames and vors_register_depth — at 640x480 for 64 and 1024 planes, beside one
vors_trackers_track call of 64 sequences measured in the same session; write profiles/frontend_summary.md.

Undistortion: grey and depth of every plane through a TUM-like Brown-Conrady camera into an ideal camera of the same size, against its
byte model of 6 B per output pixel (1 + 2 B gathered, 1 + 2 B written). Registration: a depth camera 5 cm beside a colour camera of the same
size, footprint 1, depth out; its model is 2 B read per source pixel, one 8-byte atomic per landed pixel (taken from the pass's own
counters) and the resolve's 8 + 2 B per colour pixel. The stream fill of the key planes (8 B per colour pixel) is part of the call and of
its time, not of the model; it is also timed alone (the registration of planes that hold no depth, no output but the keys).
HIP events around one call; a block = the median of `--reps` calls after 3 warm-up calls; the blocks of all legs alternate for `--blocks`
rounds, so the figure of a leg is the median of its block medians and its run-to-run spread their range. No threshold is fixed.

  python tools/frontend_bench.py [--blocks K] [--reps R] [--frames F] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS = 480, 640
SIZES = (64, 1024)
CAM = np.array([318.6, 255.3, 517.3, 516.5, 0.0], np.float32)
DIST = np.array([0.26, -0.95, -0.005, 0.003, 1.16], np.float32)
POSE = np.array([0.05, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], np.float32)


def block(torch, fn, reps, warm=3):
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
    plane = ROWS * COLS
    seeds = [2000 + s for s in range(SIZES[0])]
    gray64, depth64 = V.synth_render_frames(seeds, [0] * SIZES[0], [np.zeros(6)] * SIZES[0], ROWS, COLS, CAM, invalid_percent=2)
    legs = {}
    for n in SIZES:
        gray, depth = gray64.repeat(n // SIZES[0], 1, 1), depth64.repeat(n // SIZES[0], 1, 1)
        shape = (n, ROWS, COLS)
        og, od = torch.empty(shape, dtype=torch.uint8, device="cuda"), torch.empty(shape, dtype=torch.int16, device="cuda")
        zkey = torch.empty(shape, dtype=torch.int64, device="cuda")
        legs[f"undistort, grey + depth, n = {n}"] = (
            lambda gray=gray, depth=depth, og=og, od=od: V.undistort_frames(gray, depth, CAM, DIST, CAM, ROWS, COLS, gray_out=og, depth_out=od), n * plane * 6)
        landed = int(V.register_depth(depth, CAM, V.DEPTH_SCALE, CAM, ROWS, COLS, V.DEPTH_SCALE, pose7=POSE, depth_out=od, counts=True,
                                      zkey=zkey)["counts"][:, 2].sum())
        legs[f"register, footprint 1, n = {n}"] = (
            lambda depth=depth, od=od, zkey=zkey: V.register_depth(depth, CAM, V.DEPTH_SCALE, CAM, ROWS, COLS, V.DEPTH_SCALE, pose7=POSE, depth_out=od, zkey=zkey),
            n * plane * 2 + landed * 8 + n * plane * 10)
        empty = torch.zeros_like(depth)
        legs[f"register: key-plane fill + a splat of empty planes, n = {n}"] = (
            lambda empty=empty, zkey=zkey: V.register_depth(empty, CAM, V.DEPTH_SCALE, CAM, ROWS, COLS, V.DEPTH_SCALE, depth_out=False, zkey=zkey),
            n * plane * (2 + 8))
    # the yardstick: one vors_trackers_track call of 64 sequences over the same kind of frames
    n = SIZES[0]
    step = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001])
    frames = [V.synth_render_frames(seeds, [k] * n, [step * k] * n, ROWS, COLS, CAM, invalid_percent=2) for k in range(a.frames)]
    cfg = V.Config(nb_levels=5, intrinsics=V.Intrinsics(CAM[:2], CAM[2:4], CAM[4]), arithmetic=V.ARITH_FUSED)
    tr = V.Trackers(cfg, n, ROWS, COLS)
    tr.init(*frames[0])
    state = {"k": 0}

    def track():
        state["k"] = state["k"] % (a.frames - 1) + 1
        tr.track(*frames[state["k"]])

    legs[f"yardstick: vors_trackers_track, n = {n}"] = (track, 0)
    meds = {name: [] for name in legs}
    for _ in range(a.blocks):
        for name, (fn, _) in legs.items():
            meds[name].append(block(torch, fn, a.reps))
    return [(name, float(np.median(meds[name])), min(meds[name]), max(meds[name]), legs[name][1]) for name in legs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend_summary.md"))
    a = ap.parse_args()
    rows = measure(a)
    track_ms = rows[-1][1]
    lines = ["## Measured on one MI355X", "",
             f"`python tools/frontend_bench.py --blocks {a.blocks} --reps {a.reps} --frames {a.frames}`: planes of {COLS}x{ROWS}; medians of {a.blocks} "
             f"alternating blocks of {a.reps} calls (range of the block medians in brackets); HIP events around one call.", "",
             "| leg | ms per call | range, ms | bytes of the model | GB/s of the model | x one track call of 64 sequences |", "|---|---|---|---|---|---|"]
    for name, med, lo, hi, nbytes in rows:
        rate = f"{nbytes / med / 1e6:.0f}" if nbytes else "-"
        lines.append(f"| {name} | {med:.4f} | {lo:.4f} .. {hi:.4f} | {nbytes or '-'} | {rate} | {med / track_ms:.2f} |")
    text = "\n".join(lines) + "\n"
    # (the summary's first part — definitions, the coordinate bound, the listing's figures — is kept; this section is replaced)
    head = open(a.out).read().split(lines[0])[0] if os.path.exists(a.out) else ""
    with open(a.out, "w") as f:
        f.write(head + text)
    print(text)


if __name__ == "__main__":
    main()
