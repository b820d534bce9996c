#!/usr/bin/env python3
"""Time the lock-step trackers with the keyframe map and its voxel filter on, the voxels' statistics off and on, and the resolve of the
statistics; write profiles/trackers_map_voxel_stats_summary.md.

The set-up of tools/trackers_map_voxels_bench.py (its frames, shapes, map arguments, voxel edge and table): 640x480, 6 levels, 64
sequences x 39 tracked frames, FUSED arithmetic, the three candidate modes, the map at level 0 in the sparse modes and level 1 in dense
mode, 0.02 m voxels in 2^20 entries. Both legs run with the map and the voxel filter on; the second also calls enable_map_voxel_stats().
A block = one whole sequence run on a fresh handle, timed with HIP events around the tracked frames (init, which clears the table and
the statistics, is outside); the blocks of the two legs alternate for `--blocks` rounds after one warm-up run of each: median with range.
The yardstick of the statistics is the voxels-on figure of the same run; no threshold is fixed. The resolve (map_voxel_means into
preallocated outputs) is timed on the last statistics handle: `--blocks` calls after a warm-up one, each between two HIP events.

  python tools/trackers_map_voxel_stats_bench.py [--sequences N] [--frames F] [--blocks K] [--voxel M] [--slots S] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trackers_map_bench import COLS, L, ROWS, render  # noqa: E402


def one_run(V, torch, cfg, frames, n_seq, map_args, voxels, stats, resolve_calls=0):
    """-> (ms of the tracked frames, points kept, observations counted, sequences overflowed, ms of each resolve call)"""
    tr = V.Trackers(cfg, n_seq, ROWS, COLS)
    tr.enable_map(*map_args)
    tr.enable_map_voxels(*voxels)
    if stats:
        tr.enable_map_voxel_stats()
    tr.init(*frames[0])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for g, d in frames[1:]:
        tr.track(g, d)
    e1.record()
    e1.synchronize()
    counts = tr.map(copy=False)["counts"].cpu().numpy().view(np.uint32).astype(np.int64)
    overflowed = int((tr.map_voxels()["overflow"].cpu().numpy() != 0).sum())
    observations, resolve = 0, []
    if stats:
        obs = tr.map_voxel_stats(copy=False)["obs"]
        observations = int(obs[..., 0].to(torch.int64).sum().item())
        if resolve_calls:
            cap = map_args[1]
            xyz = torch.empty((n_seq, cap, 3), dtype=torch.float32, device="cuda")
            gray = torch.empty((n_seq, cap), dtype=torch.uint8, device="cuda")
            kept = torch.empty(n_seq, dtype=torch.int32, device="cuda")
            for k in range(resolve_calls + 1):   # (the first one warms up)
                r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                r0.record()
                tr.map_voxel_means(2, 1, xyz_mean=xyz, gray_mean=gray, kept=kept)
                r1.record()
                r1.synchronize()
                if k:
                    resolve.append(r0.elapsed_time(r1))
    return e0.elapsed_time(e1), int(counts.sum()), observations, overflowed, resolve


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
        legs = {"voxels on": False, "voxels + statistics on": True}
        ms = {k: [] for k in legs}
        info, resolve = {}, []
        for k, st in legs.items():
            one_run(V, torch, cfg, frames, a.sequences, map_args, (a.voxel, a.slots), st)   # warm-up
        for b in range(a.blocks):
            for k, st in legs.items():
                t, *info[k], r = one_run(V, torch, cfg, frames, a.sequences, map_args, (a.voxel, a.slots), st,
                                         a.blocks if st and b == a.blocks - 1 else 0)
                ms[k].append(t)
                resolve = r or resolve
        result[mname] = dict(level=level, legs={k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}, info=info,
                             resolve=(float(np.median(resolve)), float(min(resolve)), float(max(resolve))), capacity=map_args[1])
        del frames
        torch.cuda.empty_cache()
    return result, torch.cuda.get_device_name(0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sequences", type=int, default=64)
    p.add_argument("--frames", type=int, default=40, help="rendered frames per sequence (the first one initialises)")
    p.add_argument("--blocks", type=int, default=5)
    p.add_argument("--voxel", type=float, default=0.02, help="voxel edge in metres")
    p.add_argument("--slots", type=int, default=1 << 20, help="table entries per sequence")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "trackers_map_voxel_stats_summary.md"))
    a = p.parse_args()
    result, device = measure(a)
    tracked = a.sequences * (a.frames - 1)
    lines = ["# Sequence trackers with the voxel-filtered keyframe map: the voxels' statistics off and on, and their resolve", "",
             f"`tools/trackers_map_voxel_stats_bench.py` on {device}: {COLS}x{ROWS}, {L} levels, {a.sequences} sequences x {a.frames - 1} tracked "
             f"frames, FUSED arithmetic, map and voxel filter on in both legs (min_weight 0, voxel edge {a.voxel} m, {a.slots} table entries per "
             f"sequence); HIP events around the tracked frames of a run, {a.blocks} alternating blocks per leg, median (min .. max). The resolve is "
             f"map_voxel_means(min_count 2, min_span 1) with all three outputs, {a.blocks} calls on the last handle.", "",
             "| candidates | map level | leg | ms per run | frames per second | points kept | observations counted | sequences overflowed |",
             "|---|---|---|---|---|---|---|---|"]
    for mname, r in result.items():
        for k, (med, lo, hi) in r["legs"].items():
            pts, observations, over = r["info"][k]
            lines.append(f"| {mname} | {r['level']} | {k} | {med:.2f} ({lo:.2f} .. {hi:.2f}) | {tracked / med * 1e3:.0f} ({tracked / hi * 1e3:.0f} .. "
                         f"{tracked / lo * 1e3:.0f}) | {pts} | {observations if 'statistics' in k else ''} | {over} |")
        off, on = r["legs"]["voxels on"][0], r["legs"]["voxels + statistics on"][0]
        lines.append(f"| {mname} | {r['level']} | statistics on / off | {on / off:.3f} | | | | |")
        lines.append(f"| {mname} | {r['level']} | statistics on - off | {on - off:.2f} | | | | |")
        med, lo, hi = r["resolve"]
        lines.append(f"| {mname} | {r['level']} | resolve, per call ({a.sequences} x {r['capacity']} ranks of capacity) | {med:.3f} ({lo:.3f} .. {hi:.3f}) "
                     "| | | | |")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
