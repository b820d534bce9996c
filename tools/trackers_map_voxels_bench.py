#!/usr/bin/env python3
"""Time the lock-step trackers with the keyframe map on, its voxel filter off and on, and write profiles/trackers_map_voxels_summary.md.

The set-up of tools/trackers_map_bench.py (its frames, shapes and map arguments): 640x480, 6 levels, 64 sequences x 39 tracked frames,
FUSED arithmetic, the three candidate modes, the map at level 0 in the sparse modes and level 1 in dense mode. Both legs run the SAME
handles' configuration with the map on; the second also calls enable_map_voxels(voxel_m, table_slots). A block = one whole sequence run
on a fresh handle, timed with HIP events around the tracked frames (init, which clears the table, is outside); the blocks of the two legs
alternate for `--blocks` rounds after one warm-up run of each: median with range. The yardstick of the filter is the voxels-off figure of
the same run; no threshold is fixed.

  python tools/trackers_map_voxels_bench.py [--sequences N] [--frames F] [--blocks K] [--voxel M] [--slots S] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trackers_map_bench import COLS, L, ROWS, render  # noqa: E402


def one_run(V, torch, cfg, frames, n_seq, map_args, voxels):
    """-> (ms of the tracked frames, keyframes emitted, points kept, occupied entries of the fullest table, sequences overflowed)"""
    tr = V.Trackers(cfg, n_seq, ROWS, COLS)
    tr.enable_map(*map_args)
    if voxels is not None:
        tr.enable_map_voxels(*voxels)
    tr.init(*frames[0])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for g, d in frames[1:]:
        tr.track(g, d)
    e1.record()
    e1.synchronize()
    m = tr.map(copy=False)   # (views: the lists are gigabytes)
    counts = m["counts"].cpu().numpy().view(np.uint32).astype(np.int64)
    occupied = overflowed = 0
    if voxels is not None:
        v = tr.map_voxels()
        occupied, overflowed = int(v["occupied"].cpu().numpy().view(np.uint32).max()), int((v["overflow"].cpu().numpy() != 0).sum())
    return e0.elapsed_time(e1), int(m["n_segments"].cpu().numpy().view(np.uint32).sum()), int(counts.sum()), occupied, overflowed


def measure(a):
    sys.path[:0] = [os.path.join(ROOT, "visual-odometry-rs_amd"), ROOT]
    import torch
    import vors_amd as V
    intr = V.scaled_intrinsics(ROWS, COLS)
    result = {}
    for mode, mname, level in ((V.CANDIDATES_COARSE_TO_FINE, "coarse-to-fine", 0), (V.CANDIDATES_DENSE, "dense", 1), (V.CANDIDATES_DSO, "DSO", 0)):
        frames = render(V, torch, a.sequences, a.frames, mode == V.CANDIDATES_DSO)
        cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, arithmetic=V.ARITH_FUSED)
        per_kf = (ROWS >> level) * (COLS >> level) if mode == V.CANDIDATES_DENSE else 65536 if mode == V.CANDIDATES_DSO else 16384
        map_args = (level, per_kf * a.frames, a.frames, 0)
        legs = {"voxels off": None, "voxels on": (a.voxel, a.slots)}
        ms = {k: [] for k in legs}
        info = {}
        for k, v in legs.items():
            one_run(V, torch, cfg, frames, a.sequences, map_args, v)   # warm-up
        for _ in range(a.blocks):
            for k, v in legs.items():
                t, *info[k] = one_run(V, torch, cfg, frames, a.sequences, map_args, v)
                ms[k].append(t)
        result[mname] = dict(level=level, legs={k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}, info=info)
        del frames
        torch.cuda.empty_cache()
    return result, torch.cuda.get_device_name(0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sequences", type=int, default=64)
    p.add_argument("--frames", type=int, default=40, help="rendered frames per sequence (the first one initialises)")
    p.add_argument("--blocks", type=int, default=5)
    p.add_argument("--voxel", type=float, default=0.02, help="voxel edge in metres")
    p.add_argument("--slots", type=int, default=1 << 20, help="table entries per sequence (16 bytes each)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "trackers_map_voxels_summary.md"))
    a = p.parse_args()
    result, device = measure(a)
    tracked = a.sequences * (a.frames - 1)
    lines = ["# Sequence trackers with the keyframe map: frames per second with the voxel filter off and on", "",
             f"`tools/trackers_map_voxels_bench.py` on {device}: {COLS}x{ROWS}, {L} levels, {a.sequences} sequences x {a.frames - 1} tracked frames, "
             f"FUSED arithmetic, map on in both legs (min_weight 0), voxel edge {a.voxel} m, {a.slots} table entries per sequence "
             f"({16 * a.slots * a.sequences / 2 ** 20:.0f} MiB in all); HIP events around the tracked frames of a run, {a.blocks} alternating blocks "
             "per leg, median (min .. max).", "",
             "| candidates | map level | leg | ms per run | frames per second | keyframes emitted | points kept | fullest table | sequences overflowed |",
             "|---|---|---|---|---|---|---|---|---|"]
    for mname, r in result.items():
        for k, (med, lo, hi) in r["legs"].items():
            kf, pts, occ, over = r["info"][k]
            tail = f"{occ} | {over}" if k == "voxels on" else " | "
            lines.append(f"| {mname} | {r['level']} | {k} | {med:.2f} ({lo:.2f} .. {hi:.2f}) | {tracked / med * 1e3:.0f} ({tracked / hi * 1e3:.0f} .. "
                         f"{tracked / lo * 1e3:.0f}) | {kf} | {pts} | {tail} |")
        off, on = r["legs"]["voxels off"][0], r["legs"]["voxels on"][0]
        lines.append(f"| {mname} | {r['level']} | on / off | {on / off:.3f} | | | | | |")
        lines.append(f"| {mname} | {r['level']} | on - off | {on - off:.2f} | | | | | |")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
