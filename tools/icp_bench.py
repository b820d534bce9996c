#!/usr/bin/env python3
"""Time vors_icp_points (64 lists against 64 depth planes of 640x480) and write the device part of profiles/icp_summary.md.

Lists of 23 500 and 465 600 points per list (the two list lengths of profiles/normals_summary.md): pixels of the depth frame drawn
uniformly, back-projected in the camera frame, their normals from vors_points_normals; the start pose is 5 mm and 0.2 degrees off, and
step_eps = 0 keeps every list iterating, so that a pass at `iters` runs iters + 1 evaluation launches and iters + 1 solve launches.
Legs, per list length: the pass at iters = 0 (the start of the state, one evaluation, one solve: the pure evaluator), the pass at iters = 8,
and from the two one round = (t8 - t0) / 8, an evaluation launch plus a solve launch. Beside them, in the same run, the nearest existing
pass: vors_render_points at footprint 1 over the same lists (it reads the same 12-byte rows and scatters one key per point where the
ICP gathers one depth), splat alone (zkey only).
Byte model of an evaluation: 12 + 12 B per point read, a 2 B gather; the partials are 112 B per 1024 points.
HIP events around one call; a block = the median of 20 calls after 3 warm-up calls; the blocks of all legs alternate for `--blocks` rounds,
so the figure of a leg is the median of its block medians and its run-to-run spread their range. No threshold is fixed.

--robust times the robust pass instead (vors_icp_points_robust) and writes profiles/icp_robust_summary.md: per list length
the pass at iters 0 and at iters 8 in four forms — the plain pass, robust neutral (no frame normals, no Huber), robust with the normal
gate, robust with the gate and Huber — all in the same run, their blocks alternating. The frame normals are vors_depth_normals' of the
frames. Byte model of an evaluation: 26 B per point, 38 B with the 12 B gather of the frame normal.

--joint times the joint pass (vors_icp_points_joint) beside the robust one and writes profiles/icp_joint_summary.md: per list
length the pass at iters 0 and at iters 8 as robust with the gate and Huber, as joint with the same and the photometric rows, and as joint
with the photo Huber weight too. The list's grey is the frame's at the point's pixel. Byte model of an evaluation: the robust pass's 38 B
per point, and 1 B of list grey and 4 gathered tap bytes: 43 B.

  python tools/icp_bench.py [--robust | --joint] [--lists N] [--blocks K] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from normals_bench import COLS, ROWS, SEQS, SIZES, block  # noqa: E402


def measure(a):
    sys.path[:0] = [os.path.join(ROOT, "visual-odometry-rs_amd"), ROOT]
    import torch
    import vors_amd as V
    intr = np.asarray(V.scaled_intrinsics(ROWS, COLS), np.float32)
    cu, cv, fu, fv, _ = [float(v) for v in intr]
    n = a.lists
    frame_gray, depth = V.synth_render_frames([2000 + s for s in range(n)], [0] * n, [np.zeros(6)] * n, ROWS, COLS, intr, invalid_percent=2)
    start = np.zeros(7, np.float32)
    V.lib().vors_se3_exp(V._ptr(np.array([0.003, -0.003, 0.003, 0.002, -0.002, 0.002], np.float32)), V._ptr(start))
    poses = torch.from_numpy(np.tile(start, (n, 1))).cuda()
    zkey = torch.empty((n, ROWS, COLS), dtype=torch.int64, device="cuda")
    rng = np.random.default_rng(0)
    legs, matched = {}, {}
    for size in SIZES:
        px, py = rng.integers(0, COLS, (n, size)), rng.integers(0, ROWS, (n, size))
        pixel = torch.from_numpy((px | (py << 16)).astype(np.int32)).cuda()
        counts = torch.full((n,), size, dtype=torch.int32, device="cuda")
        z = torch.gather(depth.view(n, -1).to(torch.int32) & 0xffff, 1, torch.from_numpy(py * COLS + px).cuda()).to(torch.float32) / V.DEPTH_SCALE
        xyz = torch.stack([(torch.from_numpy(px).cuda() - cu) * z / fu, (torch.from_numpy(py).cuda() - cv) * z / fv, z], -1).to(torch.float32).contiguous()
        nrm = V.points_normals(depth, pixel, counts, intr, V.DEPTH_SCALE, 1, 0.05)["normals"]
        gray = torch.zeros((n, size), dtype=torch.uint8, device="cuda")
        ws = torch.empty(V.icp_workspace_bytes(n, size), dtype=torch.uint8, device="cuda")
        stats = torch.zeros((n, 24), dtype=torch.uint8, device="cuda")

        def icp(iters, xyz=xyz, nrm=nrm, counts=counts, ws=ws, stats=stats):
            return V.icp_points(xyz, nrm, counts, depth, intr, V.DEPTH_SCALE, poses, 0.05, step_eps=0.0, iters=iters, workspace=ws, stats=stats)

        if a.robust or a.joint:
            frame_normals = V.depth_normals(depth, intr, V.DEPTH_SCALE, 1, 0.05)["normals"]
            forms = {"plain": None, "robust neutral": dict(), "robust, normal gate": dict(frame_normals=frame_normals, min_cos=0.8),
                     "robust, normal gate + Huber": dict(frame_normals=frame_normals, min_cos=0.8, huber_m=0.005)}
            if a.joint:
                list_gray = torch.gather(frame_gray.view(n, -1), 1, torch.from_numpy(py * COLS + px).cuda()).contiguous()
                both = forms["robust, normal gate + Huber"]
                forms = {"robust, normal gate + Huber": both, "joint, normal gate + Huber + photometric rows": dict(both, photo_scale_m=0.0005),
                         "joint, the same + photo Huber": dict(both, photo_scale_m=0.0005, photo_huber_grey=10.0)}
            for form, kw in forms.items():
                def run(iters, kw=kw, xyz=xyz, nrm=nrm, counts=counts, ws=ws, stats=stats, list_gray=list_gray if a.joint else None):
                    if kw is None:
                        return icp(iters, xyz, nrm, counts, ws, stats)
                    if "photo_scale_m" in kw:
                        return V.icp_points_joint(xyz, nrm, list_gray, counts, depth, frame_gray, intr, V.DEPTH_SCALE, poses, 0.05, step_eps=0.0,
                                                  iters=iters, workspace=ws, stats=stats, **kw)
                    return V.icp_points_robust(xyz, nrm, counts, depth, intr, V.DEPTH_SCALE, poses, 0.05, step_eps=0.0, iters=iters, workspace=ws,
                                               stats=stats, **kw)
                run(8)
                torch.cuda.synchronize()
                st = V.decode_icp_stats(stats)
                matched[size, form] = (int(st["matched"].min()), int(st["matched"].max()), sorted(set(st["iterations"].tolist())),
                                       sorted(set(st["status"].tolist())))
                model = n * size * ((38 if kw and "frame_normals" in kw else 26) + (5 if kw and "photo_scale_m" in kw else 0)) \
                    + n * ((size + 1023) // 1024) * 116
                legs[f"{size} points, {form}: pass at iters 0"] = (lambda run=run: run(0), model)
                legs[f"{size} points, {form}: pass at iters 8"] = (lambda run=run: run(8), 9 * model)
            continue
        icp(8)
        torch.cuda.synchronize()
        st = V.decode_icp_stats(stats)
        matched[size] = (int(st["matched"].min()), int(st["matched"].max()), sorted(set(st["iterations"].tolist())), sorted(set(st["status"].tolist())))
        model = n * size * 26 + n * ((size + 1023) // 1024) * 116
        legs[f"{size} points: pass at iters 0"] = (lambda icp=icp: icp(0), model)
        legs[f"{size} points: pass at iters 8"] = (lambda icp=icp: icp(8), 9 * model)
        legs[f"{size} points: yardstick, vors_render_points footprint 1, splat alone"] = (
            lambda xyz=xyz, gray=gray, counts=counts: V.render_points(xyz, gray, counts, intr, ROWS, COLS, V.DEPTH_SCALE, poses=poses, depth=False,
                                                                      gray=False, zkey=zkey), n * size * 12 + n * ROWS * COLS * 8)
    meds = {name: [] for name in legs}
    for _ in range(a.blocks):
        for name, (fn, _) in legs.items():
            meds[name].append(block(torch, fn))
    return [(name, float(np.median(meds[name])), min(meds[name]), max(meds[name]), legs[name][1]) for name in legs], matched


def report_robust(a, rows, matched):
    title = ("# Joint point-to-plane and photometric ICP: vors_icp_points_joint beside vors_icp_points_robust" if a.joint else
             "# Robust point-to-plane ICP: vors_icp_points_robust beside vors_icp_points")
    lines = [title, "",
             f"`python tools/icp_bench.py {'--joint' if a.joint else '--robust'} --lists {a.lists} --blocks {a.blocks}` on one MI355X: {a.lists} lists against {a.lists} planes "
             f"of {COLS}x{ROWS}; medians of {a.blocks} alternating blocks of 20 calls (range of the block medians in brackets). Byte model of "
             "an evaluation: 26 B per point, 38 B with the gather of the frame normal" + (", 43 B with the list's grey byte and the four taps." if a.joint else "."), "",
             "| leg | ms | range, ms | bytes of the model | GB/s of the model |", "|---|---|---|---|---|"]
    by = {}
    for name, med, lo, hi, nbytes in rows:
        by[name] = (med, lo, hi, nbytes)
        lines.append(f"| {name} | {med:.4f} | {lo:.4f} .. {hi:.4f} | {nbytes} | {nbytes / med / 1e6:.0f} |")
    lines += ["", "One round (an evaluation launch and a solve launch) = (pass at iters 8 - pass at iters 0) / 8, from the medians; the "
              "spread is that of the pass at iters 8 over 8:", ""]
    for (size, form), (lo, hi, its, sts) in matched.items():
        t0, _, _, m = by[f"{size} points, {form}: pass at iters 0"]
        t8, lo8, hi8, _ = by[f"{size} points, {form}: pass at iters 8"]
        lines.append(f"- {size} points, {form}: {(t8 - t0) / 8:.4f} ms (spread {(hi8 - lo8) / 8:.4f}), {m / ((t8 - t0) / 8) / 1e9:.2f} TB/s of the "
                     f"model; matched per list {lo} .. {hi}, updates {its}, statuses {sts}")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, default=SEQS)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_summary.md"))
    ap.add_argument("--robust", action="store_true")
    ap.add_argument("--joint", action="store_true")
    a = ap.parse_args()
    if (a.robust or a.joint) and a.out == ap.get_default("out"):
        a.out = os.path.join(ROOT, "profiles", "icp_joint_summary.md" if a.joint else "icp_robust_summary.md")
    rows, matched = measure(a)
    if a.robust or a.joint:
        return report_robust(a, rows, matched)
    lines = ["# Point-to-plane ICP: vors_icp_points", "",
             f"`python tools/icp_bench.py --lists {a.lists} --blocks {a.blocks}` on one MI355X: {a.lists} lists against {a.lists} planes of "
             f"{COLS}x{ROWS}; medians of {a.blocks} alternating blocks of 20 calls (range of the block medians in brackets).", "",
             "| leg | ms | range, ms | bytes of the model | GB/s of the model |", "|---|---|---|---|---|"]
    by = {}
    for name, med, lo, hi, nbytes in rows:
        by[name] = (med, nbytes)
        lines.append(f"| {name} | {med:.4f} | {lo:.4f} .. {hi:.4f} | {nbytes} | {nbytes / med / 1e6:.0f} |")
    lines += ["", "One round (an evaluation launch and a solve launch) = (pass at iters 8 - pass at iters 0) / 8:", ""]
    for size in SIZES:
        t0, m = by[f"{size} points: pass at iters 0"]
        t8, _ = by[f"{size} points: pass at iters 8"]
        lo, hi, its, sts = matched[size]
        lines.append(f"- {size} points: {(t8 - t0) / 8:.4f} ms, {m / ((t8 - t0) / 8) / 1e6:.0f} GB/s of the model; matched per list {lo} .. {hi}, "
                     f"updates {its}, statuses {sts}")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
