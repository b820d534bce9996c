"""Development aid (CPU, reads rocprofv3 CSVs): where the second slice of a two-halves step runs, and the LM stage's VALU instructions.

    python tools/batch_halves_trace.py KERNEL_TRACE_CSV [COUNTER_COLLECTION_CSV] --pyramids-per-step 2|4

KERNEL_TRACE_CSV is the per-dispatch trace of `rocprofv3 --kernel-trace --stats -- python bench.py ...` (tools/profile.sh pass 1),
COUNTER_COLLECTION_CSV the SQ pass of a run of its own (pass 4). A bench step launches pyramid_fused_kernel twice on the plain path
(keyframe, current) and four times as two halves, which is how the steps are told apart: --pyramids-per-step.

For the LAST complete step of the trace: every dispatch up to the end of the last pre-LM kernel, with its queue; per queue that runs
pre-LM kernels, the pre-LM interval and the interval of the LM-stage kernels of that queue; and whether the pre-LM kernels of the
queue that starts second lie inside the LM interval of the queue that starts first. Then SQ_INSTS_VALU of the LM-stage kernels per step.
"""
import argparse
import csv
from collections import defaultdict

LM_STAGE = ("lm_track_kernel", "lm_split_eval_kernel", "lm_split_step_kernel", "lm_split_merge", "lm_ref_track_kernel", "lm_ref_track_coop_kernel")
PRE_LM = ("pyramid_fused_kernel", "halve_mean_kernel", "dense_idepth")

p = argparse.ArgumentParser()
p.add_argument("trace")
p.add_argument("counters", nargs="?")
p.add_argument("--pyramids-per-step", type=int, required=True)
a = p.parse_args()


def short(name):
    return name.split("(")[0].replace("void ", "").replace("vors::", "")[:48]


def is_in(name, group):
    return any(k in name for k in group)


disp = []
for r in csv.DictReader(open(a.trace)):
    disp.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "-"), r["Kernel_Name"]))
disp.sort()
pyr = [i for i, d in enumerate(disp) if "pyramid_fused_kernel" in d[3]]
n_steps = len(pyr) // a.pyramids_per_step
assert n_steps >= 2, "the trace holds fewer than two steps"
k = n_steps - 2 if len(pyr) % a.pyramids_per_step == 0 else n_steps - 1   # the last step that is followed by another one (or by a partial one)
first, nxt = pyr[k * a.pyramids_per_step], pyr[(k + 1) * a.pyramids_per_step]
step = disp[first:nxt]
t0 = step[0][0]
us = lambda t: (t - t0) / 1e3
print(f"steps in the trace: {n_steps}; step {k}: {len(step)} dispatches, {us(max(e for _, e, _, _ in step)):.1f} us from its first start to its last end")
last_pre = max(i for i, d in enumerate(step) if is_in(d[3], PRE_LM))
print("\n| start us | end us | queue | kernel |\n|---|---|---|---|")
for s, e, q, n in step[:last_pre + 1]:
    print(f"| {us(s):.1f} | {us(e):.1f} | {q} | {short(n)} |")
by_q = defaultdict(lambda: {"pre": [], "lm": []})
for s, e, q, n in step:
    if is_in(n, PRE_LM):
        by_q[q]["pre"].append((s, e))
    elif is_in(n, LM_STAGE):
        by_q[q]["lm"].append((s, e))
pre_queues = sorted((q for q in by_q if by_q[q]["pre"]), key=lambda q: min(s for s, _ in by_q[q]["pre"]))
print()
for q in pre_queues:
    pre, lm = by_q[q]["pre"], by_q[q]["lm"]
    print(f"queue {q}: pre-LM kernels {us(min(s for s, _ in pre)):.1f} .. {us(max(e for _, e in pre)):.1f} us"
          + (f", LM-stage kernels {us(min(s for s, _ in lm)):.1f} .. {us(max(e for _, e in lm)):.1f} us" if lm else ""))
if len(pre_queues) >= 2 and by_q[pre_queues[0]]["lm"]:
    qa, qb = pre_queues[0], pre_queues[1]
    lm0, lm1 = min(s for s, _ in by_q[qa]["lm"]), max(e for _, e in by_q[qa]["lm"])
    inside = [(s, e) for s, e in by_q[qb]["pre"] if s >= lm0 and e <= lm1]
    after = [(s, e) for s, e in by_q[qb]["pre"] if e > lm0]
    print(f"second slice (queue {qb}): {len(inside)} of its {len(by_q[qb]['pre'])} pre-LM dispatches lie wholly inside the first slice's LM interval "
          f"(queue {qa}, {us(lm0):.1f} .. {us(lm1):.1f} us); {len(after)} end after it starts")
elif len(pre_queues) == 1:
    print("one queue runs every pre-LM kernel: the plain path")

if a.counters:
    valu, n_pyr = 0.0, 0
    for r in csv.DictReader(open(a.counters)):
        if r.get("Counter_Name") != "SQ_INSTS_VALU":
            continue
        if is_in(r["Kernel_Name"], LM_STAGE):
            valu += float(r["Counter_Value"])
        if "pyramid_fused_kernel" in r["Kernel_Name"]:
            n_pyr += 1
    steps = n_pyr / a.pyramids_per_step
    print(f"\nSQ_INSTS_VALU of the LM-stage kernels: {valu / steps:.6g} per step over {steps:g} steps")
