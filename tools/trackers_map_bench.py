#!/usr/bin/env python3
"""Time the lock-step trackers with the keyframe map off and on and write profiles/trackers_map_summary.md.

640x480, 6 levels, 64 sequences x 39 tracked frames (40 rendered), FUSED arithmetic, the three candidate modes; the map takes level 0 in
the sparse modes and level 1 in dense mode (a quarter of the pixels: 17 bytes per point and keyframe add up). A block = one whole sequence
run (init + 39 tracks) on a fresh handle, timed with HIP events around the 39 tracks; the blocks of the two legs (map off, map on) alternate
for `--blocks` rounds after one warm-up run of each, so the figure of a leg is the median of its blocks and its run-to-run spread their
range. No cost target: the yardstick of the map is the map-off figure of the same run. Beside it, the same level through
vors_batch_point_cloud on a separate batch handle prepared on the first frame, in calls of n_sequences pairs, over as many keyframes as the
mapped run emitted: what the caller of a plain Batch pays for the same clouds (without the round trips that tell it when to ask).

  python tools/trackers_map_bench.py [--sequences N] [--frames F] [--blocks K] [--out FILE]
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


def one_run(V, torch, cfg, frames, n_seq, map_args):
    """-> (ms of the tracked frames, keyframes emitted over all sequences incl. the init frames, points kept, points beyond the capacity)"""
    tr = V.Trackers(cfg, n_seq, ROWS, COLS)
    if map_args is not None:
        tr.enable_map(*map_args)
    tr.init(*frames[0])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for g, d in frames[1:]:
        tr.track(g, d)
    e1.record()
    e1.synchronize()
    if map_args is None:
        return e0.elapsed_time(e1), 0, 0, 0
    m = tr.map(copy=False)   # (views: the lists are gigabytes)
    counts = m["counts"].cpu().numpy().view(np.uint32).astype(np.int64)
    return e0.elapsed_time(e1), int(m["n_segments"].cpu().numpy().view(np.uint32).sum()), int(counts.sum()), int(np.maximum(counts - map_args[1], 0).sum())


def batch_clouds(V, torch, cfg, frames, n_seq, level, keyframes):
    """ms of ceil(keyframes / n_seq) vors_batch_point_cloud calls of n_seq pairs each (xyz + pixel + gray + counts into fixed outputs)."""
    b = V.Batch(cfg, n_seq, ROWS, COLS)
    b.prepare_keyframes(*frames[0])
    cap = (ROWS >> level) * (COLS >> level)
    poses = torch.zeros((n_seq, 7), dtype=torch.float32, device="cuda")
    poses[:, 6] = 1.0
    out = dict(xyz=torch.empty((n_seq, cap, 3), dtype=torch.float32, device="cuda"), pixel=torch.empty((n_seq, cap), dtype=torch.int32, device="cuda"),
               gray=torch.empty((n_seq, cap), dtype=torch.uint8, device="cuda"), counts=torch.empty(n_seq, dtype=torch.int32, device="cuda"))
    calls = max((keyframes + n_seq - 1) // n_seq, 1)
    b.point_cloud(level, poses=poses, capacity=cap, **out)   # (the first call creates the count workspace)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        b.point_cloud(level, poses=poses, capacity=cap, **out)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), calls


def measure(a):
    sys.path[:0] = [os.path.join(ROOT, "visual-odometry-rs_amd"), ROOT]
    import torch
    import vors_amd as V
    intr = V.scaled_intrinsics(ROWS, COLS)
    result = {}
    for mode, mname, level in ((V.CANDIDATES_COARSE_TO_FINE, "coarse-to-fine", 0), (V.CANDIDATES_DENSE, "dense", 1), (V.CANDIDATES_DSO, "DSO", 0)):
        frames = render(V, torch, a.sequences, a.frames, mode == V.CANDIDATES_DSO)
        cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, arithmetic=V.ARITH_FUSED)
        # room for a keyframe at every frame: dense = every pixel of the level, lists = their capacity at level 0 (65536 bounds both)
        per_kf = (ROWS >> level) * (COLS >> level) if mode == V.CANDIDATES_DENSE else 65536 if mode == V.CANDIDATES_DSO else 16384
        legs = {"map off": None, "map on": (level, per_kf * a.frames, a.frames, 0)}
        ms = {k: [] for k in legs}
        info = {}
        for k, f in legs.items():
            one_run(V, torch, cfg, frames, a.sequences, f)   # warm-up
        for _ in range(a.blocks):
            for k, f in legs.items():
                t, *info[k] = one_run(V, torch, cfg, frames, a.sequences, f)
                ms[k].append(t)
        keyframes, points, dropped = info["map on"]
        beside = []
        for _ in range(a.blocks + 1):
            t, calls = batch_clouds(V, torch, cfg, frames, a.sequences, level, keyframes)
            beside.append(t)
        beside = beside[1:]   # (the first is the warm-up)
        result[mname] = dict(level=level, legs={k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}, keyframes=keyframes,
                             points=points, dropped=dropped, beside=(float(np.median(beside)), float(min(beside)), float(max(beside))), calls=calls)
        del frames
        torch.cuda.empty_cache()
    return result, torch.cuda.get_device_name(0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sequences", type=int, default=64)
    p.add_argument("--frames", type=int, default=40, help="rendered frames per sequence (the first one initialises)")
    p.add_argument("--blocks", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "trackers_map_summary.md"))
    a = p.parse_args()
    result, device = measure(a)
    tracked = a.sequences * (a.frames - 1)
    lines = ["# Sequence trackers: frames per second with the keyframe map off and on", "",
             f"`tools/trackers_map_bench.py` on {device}: {COLS}x{ROWS}, {L} levels, {a.sequences} sequences x {a.frames - 1} tracked frames, "
             f"FUSED arithmetic, min_weight 0; HIP events around the tracked frames of a run, {a.blocks} alternating blocks per leg, "
             "median (min .. max). `batch clouds`: the same level through `vors_batch_point_cloud` on a separate batch handle, in calls of "
             f"{a.sequences} pairs, over as many keyframes as the mapped run emitted (rounded up to whole calls).", "",
             "| candidates | map level | leg | ms per run | frames per second | keyframes emitted | points kept (dropped) |", "|---|---|---|---|---|---|---|"]
    for mname, r in result.items():
        for k, (med, lo, hi) in r["legs"].items():
            kf = f"{r['keyframes']}" if k == "map on" else ""
            pts = f"{r['points']} ({r['dropped']})" if k == "map on" else ""
            lines.append(f"| {mname} | {r['level']} | {k} | {med:.2f} ({lo:.2f} .. {hi:.2f}) | {tracked / med * 1e3:.0f} ({tracked / hi * 1e3:.0f} .. {tracked / lo * 1e3:.0f}) | {kf} | {pts} |")
        off, on = r["legs"]["map off"][0], r["legs"]["map on"][0]
        lines.append(f"| {mname} | {r['level']} | on / off | {on / off:.3f} | | | |")
        lines.append(f"| {mname} | {r['level']} | on - off | {on - off:.2f} | | | |")
        med, lo, hi = r["beside"]
        lines.append(f"| {mname} | {r['level']} | batch clouds, {r['calls']} calls | {med:.2f} ({lo:.2f} .. {hi:.2f}) | | {r['calls'] * a.sequences} | |")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
