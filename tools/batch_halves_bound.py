"""Development aid (GPU): the ceiling of running ONE dense track_pairs call as two overlapped halves, measured before any such code exists.

One step of n pairs on one stream (vors_batch_track_pairs, what bench.py times as `value`; and the same step through a vors_pipeline ring
of 1, the ring's handle kind) against the SAME n pairs as two steps of n / 2 through a vors_pipeline ring of 2, inputs resident:

    joined      submit half A, submit half B, drain into the caller's stream; the next pair of halves is ordered after that drain. This is
                what a call that forks at entry and joins before it returns can reach: half B's pyramids and keyframe stage under half A's
                LM stage, each half's tails filled by the other half, nothing carried over from one call to the next.
    continuous  the free-running feed of bench.py's Ring (drain only at the end): half A of pair k + 1 also runs under half B of pair k.
                A looser ceiling that no single call can reach for a caller who uses the results between calls.

`--runs` alternating runs of each form; per form the runs, their median and their spread (max - min); and the stop rule of the issue:
the pair of halves counts as faster only if it beats the whole step by more than twice the spread of the whole step's own runs.

    python tools/batch_halves_bound.py [--pairs 4096] [--rows 480 --cols 640 --levels 6 --huber 0] [--arith fused] [--steps 40] [--runs 3]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "visual-odometry-rs_amd"))
import numpy as np
import torch
import vors_amd as V

p = argparse.ArgumentParser()
p.add_argument("--pairs", type=int, default=4096)
p.add_argument("--rows", type=int, default=480)
p.add_argument("--cols", type=int, default=640)
p.add_argument("--levels", type=int, default=6)
p.add_argument("--huber", type=float, default=0.0)
p.add_argument("--arith", choices=["fused", "reference"], default="fused")
p.add_argument("--steps", type=int, default=40)
p.add_argument("--warmup", type=int, default=3)
p.add_argument("--runs", type=int, default=3)
a = p.parse_args()

n, h = a.pairs, a.pairs // 2
assert n == 2 * h, "--pairs must be even"
intr = V.scaled_intrinsics(a.rows, a.cols)
cfg = V.Config(nb_levels=a.levels, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=V.CANDIDATES_DENSE,
               huber_delta=a.huber, arithmetic={"fused": V.ARITH_FUSED, "reference": V.ARITH_REFERENCE}[a.arith])
kg, kd, cg, _, _ = V.synth_render_pairs(0x5EED0000, n, a.rows, a.cols, intr)     # bench.py's seed: the same pairs
poses = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
status = torch.zeros(n, dtype=torch.int32, device="cuda")
halves = [slice(0, h), slice(h, n)]

whole = V.Batch(cfg, n, a.rows, a.cols)
ring1 = V.Pipeline(cfg, n, a.rows, a.cols, depth=1)
ring2 = V.Pipeline(cfg, h, a.rows, a.cols, depth=2)


def step_whole():
    whole.track_pairs(kg, kd, cg, poses, status)


def step_ring1():
    ring1.submit(kg, kd, cg, poses, status)
    ring1.drain()


def submit_halves():
    for s in halves:
        ring2.submit(kg[s], kd[s], cg[s], poses[s], status[s])


def step_joined():
    submit_halves()
    ring2.drain()


def timed(step, finish=None):
    """-> ms per step over a.steps steps, after a.warmup untimed ones; the clock stops behind a device synchronise."""
    for _ in range(a.warmup):
        step()
    if finish:
        finish()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    if finish:
        finish()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / a.steps * 1e3


forms = [("whole step, one stream (vors_batch_track_pairs)", step_whole, None),
         ("whole step, ring of 1", step_ring1, None),
         ("two halves, ring of 2, joined per pair of halves", step_joined, None),
         ("two halves, ring of 2, continuous feed", submit_halves, ring2.drain)]
ms = {name: [] for name, _, _ in forms}
for r in range(a.runs):
    for name, step, finish in forms:
        ms[name].append(timed(step, finish))
        print(f"run {r}: {name}: {ms[name][-1]:.4f} ms", flush=True)

# the halves compute what the whole step computes? (pairs are independent; the ring's handles have max_pairs = n / 2, so scheduling
# decisions taken from max_pairs may differ between the two: FUSED bits need not agree, poses must within the parity bar)
step_whole()
torch.cuda.synchronize()
ref_p, ref_s = poses.clone(), status.clone()
poses.zero_()
step_joined()
torch.cuda.synchronize()
print(f"halves vs whole: status equal {bool((status == ref_s).all())}, poses bit-identical {bool((poses.view(torch.int32) == ref_p.view(torch.int32)).all())}, "
      f"max |pose diff| {float((poses - ref_p).abs().max()):.3g}")

print(f"\ndense {a.arith}, {n} pairs {a.cols}x{a.rows}, {a.levels} levels, huber {a.huber:g}; {a.steps} steps per run, {a.runs} alternating runs; "
      f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}")
print("| form | runs, ms per step of all the pairs | median | spread |")
print("|---|---|---|---|")
for name, _, _ in forms:
    v = ms[name]
    print(f"| {name} | {' / '.join(f'{x:.3f}' for x in v)} | {np.median(v):.3f} | {max(v) - min(v):.3f} |")
w = ms[forms[0][0]]
bar = 2.0 * (max(w) - min(w))
for name in (forms[2][0], forms[3][0]):
    gain = float(np.median(w) - np.median(ms[name]))
    print(f"stop rule, {name}: median gain {gain:+.3f} ms against 2 x spread of the whole step = {bar:.3f} ms -> {'PASSES' if gain > bar else 'FAILS'}"
          f" (slowest halves run {max(ms[name]):.3f} vs fastest whole run {min(w):.3f})")
