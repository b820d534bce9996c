"""Times of the loop-closure entries on the device (include/vors_hip.h 2h) -> profiles/loop_closure_summary.md.

    python tools/loop_closure_bench.py [--reps 5] [--small]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/loop_closure_bench.py --reps 5   (kernel times, a run of its own)

Signatures: 4096 planes of 640 x 480 at 16 x 12, against the bytes read (n rows cols) and 8 TB/s. Candidates: counts 4096 and 16384,
D = 192 and 768, k = 4, with and without poses, against count^2 / 2 * D i8 multiply-adds and the i8 matrix rate. One warm-up call, then
the best of --reps calls, events around each call."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-odometry-rs_amd"))
import vors_amd as V  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
I8_MACS_PER_S = 2.5e15  # i8 MFMA: twice the BF16 rate per clock (~2.5 PFLOP/s dense), ~5 Pop/s, as multiply-adds


def best_ms(call, reps):
    import torch
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return min(times)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a tenth of the sizes, to try the tool")
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(1)
    n, rows, cols, tr, tc = (4096 if not args.small else 256), 480, 640, 12, 16
    gray = torch.randint(0, 256, (n, rows, cols), dtype=torch.uint8, device="cuda", generator=gen)
    sig = torch.empty((n, tr * tc), dtype=torch.int8, device="cuda")
    meta = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    ms = best_ms(lambda: V.loop_signatures(gray, tr, tc, sig=sig, meta=meta), args.reps)
    nbytes = n * rows * cols
    print(f"signatures: {n} planes {cols}x{rows} at {tc}x{tr}: {ms:.3f} ms, {nbytes / ms / 1e6:.0f} GB/s = {100 * nbytes / (ms * 1e-3) / HBM_BYTES_PER_S:.1f} % of 8 TB/s")
    del gray
    for count in ((4096, 16384) if not args.small else (512, 2048)):
        for d in (192, 768):
            s = torch.randint(-128, 128, (1, count, d), dtype=torch.int8, device="cuda", generator=gen)
            s64 = s.to(torch.int64)
            m = torch.stack([s64.sum(-1), (s64 * s64).sum(-1)], dim=-1).to(torch.int32).contiguous()
            counts_in = torch.tensor([count], dtype=torch.int32, device="cuda")
            poses = torch.zeros((1, count, 7), dtype=torch.float32, device="cuda")
            poses[0, :, 0] = torch.arange(count, device="cuda") * 0.05
            poses[0, :, 6] = 1.0
            cand = torch.zeros((1, count, 4, 2), dtype=torch.int32, device="cuda")
            cc = torch.zeros((1, count), dtype=torch.int32, device="cuda")
            for with_poses in (False, True):
                call = lambda: V.loop_candidates(s, m, counts_in, 10, 4, 0.1, poses=poses if with_poses else None, max_dist_m=20.0 if with_poses else 0.0,  # noqa: E731
                                                 min_qdot=0.5 if with_poses else 0.0, cand=cand, cand_counts=cc)
                ms = best_ms(call, args.reps)
                macs = count * count / 2 * d
                tally = call()["counts"].cpu().numpy()[0]
                print(f"candidates: count {count}, D {d}, k 4, min_score 0.1, poses {'yes' if with_poses else 'no '}: {ms:.3f} ms, "
                      f"{macs / ms / 1e9:.1f} T i8 MAC/s = {100 * macs / (ms * 1e-3) / I8_MACS_PER_S:.2f} % of the matrix rate, "
                      f"{count * count / 2 / ms / 1e6:.1f} G pairs/s; counts {tally.tolist()}")


if __name__ == "__main__":
    main()
