"""Times of the corrected map's passes on the device (include/vors_hip.h 2i) -> profiles/repose_summary.md.

    python tools/repose_bench.py [--reps 5] [--small] [--write]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/repose_bench.py --reps 5   (kernel times, a run of its own)

Re-pose: one list of 2^24 points in 4096 segments, and 64 lists of 65 536 points in 16 segments each, with and without normals, every
segment moved — against a device-to-device copy of the same bytes (24 B per point, 48 with normals: read + write) timed in the same
session, and against 8 TB/s. Filter: one list of 2^22 points with about 50 % duplicates, table 2^23. One warm-up call, then the best of
--reps calls, events around each call (so a figure includes the launches of the call: the clear of the counters, the point pass, the
record pass)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-odometry-rs_amd"))
import vors_amd as V  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


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


def unit_poses(gen, shape):
    import torch
    q = torch.randn(shape + (4,), device="cuda", generator=gen)
    q = q / q.norm(dim=-1, keepdim=True)
    return torch.cat([torch.rand(shape + (3,), device="cuda", generator=gen) * 2 - 1, q], dim=-1).contiguous()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a sixteenth of the sizes, to try the tool")
    ap.add_argument("--write", action="store_true", help="write profiles/repose_summary.md")
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(1)
    shrink = 16 if args.small else 1
    lines = []
    for n, cap, nkf in ((1, (1 << 24) // shrink, 4096), (64, 65536 // shrink, 16)):
        xyz = torch.rand((n, cap, 3), device="cuda", generator=gen) * 8 - 4
        nrm = torch.randn((n, cap, 3), device="cuda", generator=gen)
        seg = np.zeros((n, nkf), V.MAP_SEGMENT_DTYPE)
        seg["count"], seg["first"] = cap // nkf, (np.arange(nkf) * (cap // nkf))[None]
        seg["pose7"] = unit_poses(gen, (n, nkf)).cpu().numpy()
        seg_t = torch.from_numpy(seg.view(np.uint8).reshape(n, nkf, 40)).cuda()
        counts = torch.full((n,), cap, dtype=torch.int32, device="cuda")
        n_seg = torch.full((n,), nkf, dtype=torch.int32, device="cuda")
        poses = unit_poses(gen, (n, nkf))
        xo, no, so = torch.empty_like(xyz), torch.empty_like(nrm), torch.empty_like(seg_t)
        co = torch.empty((n, V.REPOSE_COUNTS), dtype=torch.int32, device="cuda")
        for normals in (False, True):
            call = lambda: V.repose_points(xyz, counts, seg_t, n_seg, poses, n_seg, normals=nrm if normals else None, xyz_out=xo,  # noqa: E731
                                           normals_out=no if normals else False, segments_out=so, counts=co)
            copy = (lambda: (xo.copy_(xyz), no.copy_(nrm))) if normals else (lambda: xo.copy_(xyz))
            ms, ms_copy = best_ms(call, args.reps), best_ms(copy, args.reps)
            nbytes = n * cap * (48 if normals else 24)
            moved = int(co[:, 0].sum())
            lines.append(f"| re-pose, {n} x {cap} points, {nkf} segments per list, {'points and normals' if normals else 'points'} | {ms:.3f} | "
                         f"{ms_copy:.3f} | {ms / ms_copy:.2f} | {100 * nbytes / (ms * 1e-3) / HBM_BYTES_PER_S:.1f} % | {moved} moved |")
            print(lines[-1])
        del xyz, nrm, xo, no
    cap = (1 << 22) // shrink
    cells = torch.randint(0, cap // 2, (cap,), device="cuda", generator=gen)  # about half of the entries repeat a voxel
    xyz = (torch.stack([cells % 256, (cells // 256) % 256, cells // 65536], dim=-1).float() + 0.5).mul(0.05).view(1, cap, 3).contiguous()
    counts = torch.full((1,), cap, dtype=torch.int32, device="cuda")
    slots = 1 << 23
    ws = torch.empty(V.voxel_filter_workspace_bytes(1, cap, slots), dtype=torch.uint8, device="cuda")
    index, xo = torch.empty((1, cap), dtype=torch.int32, device="cuda"), torch.empty_like(xyz)
    out = {}
    def call():
        out.update(V.voxel_filter_points(xyz, counts, 0.05, slots, workspace=ws, index=index, xyz_out=xo))
    ms = best_ms(call, args.reps)
    kept = int(out["counts"][0])
    lines.append(f"| filter, 1 x {cap} points, table 2^23, xyz gathered | {ms:.3f} | - | - | - | {kept} kept ({100 * (cap - kept) / cap:.0f} % duplicates) |")
    print(lines[-1])
    if args.write:
        head = ("| case | call, ms | copy of the same bytes, ms | ratio | of 8 TB/s | |\n|---|---|---|---|---|---|\n")
        with open(os.path.join(ROOT, "profiles", "repose_summary.md"), "w") as f:
            f.write("# The corrected map: measured times (tools/repose_bench.py)\n\n" + head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
