#!/usr/bin/env python3
"""Time the lock-step trackers with the map ICP correction at keyframe promotion off and on (vors_trackers_enable_map_icp); append the
figures to profiles/trackers_map_icp_summary.md.

64 sequences x 39 frames of 640x480, six levels, coarse-to-fine candidates, FUSED arithmetic, a level-0 map with normals at (2, 0.05).
MOVING: every sequence moves, so sequences promote; frames/s of the 38 track calls with the stage off and on, and the stage's totals.
STILL: every frame is frame 0 again, so no sequence ever promotes: the difference per track call is the price of the launches the stage
enqueues unconditionally. HIP events around the track calls of a run; runs of both handles alternate for --blocks rounds; the figure of
a leg is the median of its runs, the range beside it. No threshold is fixed.

  python tools/map_icp_bench.py [--sequences N] [--frames F] [--blocks K] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS = 480, 640
ICP = dict(dist_m=0.05, iters=6, min_cos=0.9, huber_m=0.002)


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
    for _ in range(a.blocks):
        for scene, frames in (("moving", moving), ("still", still)):
            for stage in ("off", "on"):
                tr = V.Trackers(cfg, n, ROWS, COLS)
                tr.enable_map(0, 1 << 20, 64)
                tr.enable_map_normals(2, 0.05)
                if stage == "on":
                    tr.enable_map_icp(**ICP)
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
                leg = out.setdefault((scene, stage), dict(ms=[], totals=None, promotions=None))
                leg["ms"].append(e0.elapsed_time(e1))
                leg["promotions"] = int((tr.map()["n_segments"].cpu().numpy() - 1).sum())
                if stage == "on":
                    leg["totals"] = tr.map_icp()["totals"].cpu().numpy().sum(axis=0).tolist()
                del tr
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--frames", type=int, default=39)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trackers_map_icp_summary.md"))
    a = ap.parse_args()
    out = measure(a)
    calls = a.frames - 1
    lines = ["", "## Cost of the stage", "",
             f"`python tools/map_icp_bench.py --sequences {a.sequences} --frames {a.frames} --blocks {a.blocks}` on one MI355X: {a.sequences} sequences of "
             f"{COLS}x{ROWS}, six levels, coarse-to-fine FUSED, a level-0 map with normals; {ICP}; medians of {a.blocks} alternating runs of "
             f"{calls} track calls (range in brackets).", "",
             "| scene | stage | ms per run | range, ms | frames/s | ms per track call | promotions | attempted, accepted |", "|---|---|---|---|---|---|---|---|"]
    for (scene, stage), leg in out.items():
        med = float(np.median(leg["ms"]))
        lines.append(f"| {scene} | {stage} | {med:.3f} | {min(leg['ms']):.3f} .. {max(leg['ms']):.3f} | {a.sequences * calls / med * 1e3:.0f} | {med / calls:.4f} | "
                     f"{leg['promotions']} | {leg['totals'] if leg['totals'] is not None else '-'} |")
    d = (np.median(out[("still", "on")]["ms"]) - np.median(out[("still", "off")]["ms"])) / calls
    lines += ["", f"Price of the unconditional launches (still scene, nothing promotes): {d:.4f} ms per track call."]
    text = "\n".join(lines) + "\n"
    with open(a.out, "a") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
