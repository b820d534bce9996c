#!/usr/bin/env python3
"""Time vors_depth_normals / vors_points_normals (64 planes, 640x480) and the keyframe stage with the map's normals on and off; write
profiles/normals_summary.md.

Plane form: steps 1 and 4, normals only (no counters), against its byte model of 14 B per pixel (2 B read, 12 B written). Beside it, in the
same run, the nearest existing plane pass: vors_render_points on an empty list, which is the stream fill of the key plane plus
render_resolve_kernel (8 B read, 3 B written per pixel) — and the fill alone, so that the resolve's share can be read off.
List form: lists of 23 500 and 465 600 points per sequence (the two list lengths of profiles/render_map_summary.md that are maps without a
voxel filter), pixels drawn uniformly, step 1.
Keyframe stage: stage-1 times (vors_trackers_kernel_times) of 64 dense sequences at 640x480 over --frames frames with a keyframe map
at level 0, normals on and off.
HIP events around one call; a block = the median of 20 calls after 3 warm-up calls; the blocks of all legs alternate for `--blocks` rounds,
so the figure of a leg is the median of its block medians and its run-to-run spread their range. No threshold is fixed.

  python tools/normals_bench.py [--sequences N] [--blocks K] [--frames F] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, SEQS = 480, 640, 64
SIZES = (23_500, 465_600)


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
    intr = np.asarray(V.scaled_intrinsics(ROWS, COLS), np.float32)
    n = a.sequences
    seeds = [2000 + s for s in range(n)]
    gray, depth = V.synth_render_frames(seeds, [0] * n, [np.zeros(6)] * n, ROWS, COLS, intr, invalid_percent=2)
    out_plane = torch.empty((n, ROWS, COLS, 3), dtype=torch.float32, device="cuda")
    legs = {}
    for step in (1, 4):
        legs[f"plane form, step {step}"] = (lambda step=step: V.depth_normals(depth, intr, V.DEPTH_SCALE, step, 0.05, normals=out_plane), n * ROWS * COLS * 14)
    # yardstick: fill + render_resolve_kernel on an empty list, and the fill alone
    zkey = torch.empty((n, ROWS, COLS), dtype=torch.int64, device="cuda")
    rd, rg = torch.empty((n, ROWS, COLS), dtype=torch.int16, device="cuda"), torch.empty((n, ROWS, COLS), dtype=torch.uint8, device="cuda")
    xyz1, g1, c0 = torch.zeros((n, 1, 3), device="cuda"), torch.zeros((n, 1), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    legs["yardstick: key-plane fill + render_resolve_kernel"] = (
        lambda: V.render_points(xyz1, g1, c0, intr, ROWS, COLS, V.DEPTH_SCALE, depth=rd, gray=rg, zkey=zkey), n * ROWS * COLS * (8 + 8 + 3))
    legs["yardstick: key-plane fill alone"] = (
        lambda: V.render_points(xyz1, g1, c0, intr, ROWS, COLS, V.DEPTH_SCALE, depth=False, gray=False, zkey=zkey), n * ROWS * COLS * 8)
    rng = np.random.default_rng(0)
    for size in SIZES:
        pixel = torch.from_numpy((rng.integers(0, COLS, (n, size)) | (rng.integers(0, ROWS, (n, size)) << 16)).astype(np.int32)).cuda()
        counts = torch.full((n,), size, dtype=torch.int32, device="cuda")
        out_list = torch.empty((n, size, 3), dtype=torch.float32, device="cuda")
        legs[f"list form, {size} points per list"] = (
            lambda pixel=pixel, counts=counts, out_list=out_list: V.points_normals(depth, pixel, counts, intr, V.DEPTH_SCALE, 1, 0.05, normals=out_list),
            n * size * (4 + 10 + 12))
    meds = {name: [] for name in legs}
    for _ in range(a.blocks):
        for name, (fn, _) in legs.items():
            meds[name].append(block(torch, fn))
    rows = [(name, float(np.median(meds[name])), min(meds[name]), max(meds[name]), legs[name][1]) for name in legs]

    # keyframe stage of the lock-step trackers, normals on and off, alternating handles over the same frames
    step = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001]) * 4.0
    frames = [V.synth_render_frames(seeds, [k] * n, [step * k] * n, ROWS, COLS, intr, invalid_percent=2) for k in range(a.frames)]
    cfg = V.Config(nb_levels=5, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=V.CANDIDATES_DENSE, arithmetic=V.ARITH_FUSED)
    stage = {"normals off": [], "normals on": []}
    for _ in range(a.blocks):
        for name in stage:
            tr = V.Trackers(cfg, n, ROWS, COLS)
            tr.enable_map(0, ROWS * COLS * 2, 16)
            if name == "normals on":
                tr.enable_map_normals(1, 0.05)
            tr.enable_kernel_timing(64)
            tr.init(*frames[0])
            for k in range(1, a.frames):
                tr.track(*frames[k])
            torch.cuda.synchronize()
            t = tr.kernel_times("keyframe")
            stage[name].append(float(np.sum(t)))
            del tr
    return rows, stage


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=SEQS)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_summary.md"))
    a = ap.parse_args()
    rows, stage = measure(a)
    lines = ["# Surface normals: vors_depth_normals / vors_points_normals and the keyframe map's normals", "",
             f"`python tools/normals_bench.py --sequences {a.sequences} --blocks {a.blocks} --frames {a.frames}` on one MI355X: {a.sequences} planes of "
             f"{COLS}x{ROWS}; medians of {a.blocks} alternating blocks of 20 calls (range of the block medians in brackets).", "",
             "| leg | ms | range, ms | bytes of the model | GB/s of the model |", "|---|---|---|---|---|"]
    for name, med, lo, hi, nbytes in rows:
        lines.append(f"| {name} | {med:.4f} | {lo:.4f} .. {hi:.4f} | {nbytes} | {nbytes / med / 1e6:.0f} |")
    lines += ["", f"Keyframe stage (stage 1, summed over the {a.frames - 1} track calls of {a.sequences} dense sequences with a level-0 map):", "",
              "| handle | ms | range, ms |", "|---|---|---|"]
    for name, v in stage.items():
        lines.append(f"| {name} | {np.median(v):.3f} | {min(v):.3f} .. {max(v):.3f} |")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
