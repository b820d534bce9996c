#!/usr/bin/env python3
"""Time vors_render_points (64 sequences, 640x480) and write profiles/render_map_summary.md.

Lists of the sizes profiles/trackers_map_voxels_summary.md reports per sequence — 5 200 (coarse-to-fine, voxel filter), 18 100 (dense
level 1, voxel filter), 23 500 (coarse-to-fine) and 465 600 points (dense level 1) —, each point in view of its sequence's camera, rendered
with footprints 1, 2 and 3: the splat alone (d_zkey) and the whole pass (depth, grey, counts) into preallocated planes. Beside them, in
the same run, two yardsticks:
  (a) vors_batch_fuse_depth's splat alone (d_zkey) on a dense 640x480 batch of as many pairs as give about as many points (307 200 usable
      points per pair at most): the existing 64-bit-minimum splat, which also back-projects and warps its points;
  (b) the stream fill of the key plane (hipMemsetD32Async over 64 x 640 x 480 x 2 dwords), which both passes issue before their kernel.
HIP events around one call; a block = the median of 20 calls after 3 warm-up calls; the blocks of all legs alternate for `--blocks`
rounds, so the figure of a leg is the median of its block medians and its run-to-run spread their range. No threshold is fixed: the rate
of 64-bit atomic minima on this chip had not been measured before this tool.

A second section closes the loop once (the figures tests/test_gpu_render_map.py prints but does not bound): 6 dense sequences x 10 frames
at 120x160, the map rendered at the current pose with footprint 2 and handed to a fresh Batch as the keyframe, the real current frame
tracked against it — the pose error of that frame-to-model alignment against the synthetic ground truth, beside the tracker's own.

  python tools/render_map_bench.py [--sequences N] [--blocks K] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, SEQS = 480, 640, 64
SIZES = (5_200, 18_100, 23_500, 465_600)
YARD_A, YARD_B = "yardstick (a): fuse_depth splat alone", "yardstick (b): stream fill of the key plane"


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


def pose_error(pose7, gt7):
    """(translation error in m, rotation error in rad) between two camera -> world poses."""
    dq = abs(float(np.dot(pose7[3:], gt7[3:])))
    return float(np.linalg.norm(pose7[:3] - gt7[:3])), 2.0 * float(np.arccos(min(1.0, dq)))


def measure(a):
    sys.path[:0] = [os.path.join(ROOT, "visual-odometry-rs_amd"), ROOT]
    import torch
    import vors_amd as V
    intr = np.asarray(V.scaled_intrinsics(ROWS, COLS), np.float32)
    n = a.sequences
    lib = V.lib()
    fill = lib.hipMemsetD32Async   # the runtime call the pass itself makes, resolved through the library's dependency on the HIP runtime
    fill.argtypes, fill.restype = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p], C.c_int
    stream = lambda: torch.cuda.current_stream().cuda_stream
    shape = (n, ROWS, COLS)
    key = torch.empty(shape, dtype=torch.int64, device="cuda")
    depth = torch.empty(shape, dtype=torch.int16, device="cuda")
    gray = torch.empty(shape, dtype=torch.uint8, device="cuda")
    counts = torch.empty((n, V.RENDER_COUNTS), dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(1)
    # one pose per sequence; the lists are in view of it
    twists = np.concatenate([rng.uniform(-0.3, 0.3, (n, 3)), rng.uniform(-0.2, 0.2, (n, 3))], 1).astype(np.float32)
    poses = np.stack([V.se3_exp(t) for t in twists]).astype(np.float32)
    t_poses = torch.from_numpy(poses).cuda()
    # yardstick (a): a dense batch, prepared once
    pairs_max = max(1, int(round(n * max(SIZES) / (ROWS * COLS))))
    kg, kd, cg, _, _ = V.synth_render_pairs(0x5EEDB000, pairs_max, ROWS, COLS, tuple(float(x) for x in intr), want_cur_depth=True)
    cfg = V.Config(nb_levels=6, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=V.CANDIDATES_DENSE, arithmetic=V.ARITH_FUSED)
    b = V.Batch(cfg, pairs_max, ROWS, COLS)
    b.prepare_keyframes(kg, kd)
    models = torch.from_numpy(np.tile(np.array([0.01, -0.005, 0.003, 0, 0, 0, 1], np.float32), (pairs_max, 1))).cuda()
    ykey = torch.empty((pairs_max, ROWS, COLS), dtype=torch.int64, device="cuda")
    cur_depth = torch.zeros((pairs_max, ROWS, COLS), dtype=torch.int16, device="cuda")
    usable = b.reproject_depth(0, models, pred_z=False, counts=True)["counts"].cpu().numpy()[:, 0].astype(np.float64)
    result = {}
    for size in SIZES:
        xyz = np.empty((n, size, 3), np.float32)
        for s in range(n):
            xy = np.stack([rng.uniform(0, COLS - 1, size), rng.uniform(0, ROWS - 1, size)], 1).astype(np.float32)
            xyz[s] = V.camera_back_project(intr, poses[s], xy, rng.uniform(0.5, 6.0, size).astype(np.float32))
        t_xyz = torch.from_numpy(xyz).cuda()
        t_gray = torch.from_numpy(rng.integers(1, 256, (n, size)).astype(np.uint8)).cuda()
        t_cnt = torch.full((n,), size, dtype=torch.int32, device="cuda")
        pairs = max(1, min(pairs_max, int(round(n * size / float(usable.mean())))))

        def yard_a():
            p = lambda t: C.c_void_p(t.data_ptr())
            st = lib.vors_batch_fuse_depth(b._h, pairs, p(models), 0, p(cur_depth), 0.01, None, 255, 0, p(ykey), None, None, None, C.c_void_p(stream()))
            assert st == 0, lib.vors_last_error()

        def render(f, whole):
            return lambda: V.render_points(t_xyz, t_gray, t_cnt, intr, ROWS, COLS, V.DEPTH_SCALE, poses=t_poses, footprint=f, zkey=key,
                                           depth=depth if whole else False, gray=gray if whole else False, counts=counts if whole else False)

        legs = {YARD_B: lambda: fill(key.data_ptr(), -1, 2 * key.numel(), stream()), YARD_A: yard_a}
        for f in (1, 2, 3):
            legs[f"footprint {f}, splat alone"] = render(f, False)
            legs[f"footprint {f}, depth + grey + counts"] = render(f, True)
        meds = {k: [] for k in legs}
        for r in range(a.blocks):   # alternate the legs: the spread of a leg's block medians is its run-to-run spread in this process
            for k, fn in legs.items():
                meds[k].append(block(torch, fn))
            print(f"{size} points: round {r + 1}/{a.blocks} " + ", ".join(f"{k}: {v[-1]:.3f}" for k, v in meds.items()), file=sys.stderr, flush=True)
        res = {k: dict(ms=float(np.median(v)), lo=float(np.min(v)), hi=float(np.max(v))) for k, v in meds.items()}
        res["yard_points"] = float(usable[:pairs].sum())
        res["yard_pairs"] = pairs
        res["counts"] = {}
        for f in (1, 2, 3):
            render(f, True)()
            torch.cuda.synchronize()
            res["counts"][f] = counts.cpu().numpy().astype(np.float64).sum(axis=0).tolist()
        result[size] = res
        del t_xyz, t_gray
    del b
    result["loop"] = close_the_loop(torch, V)
    return result


def close_the_loop(torch, V):
    rows, cols, L, n_seq, n_frames = 120, 160, 4, 6, 10
    base, speed = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001]), np.array([4.0, 0.05, 9.0, 2.0, 6.0, 5.0])
    intr = V.scaled_intrinsics(rows, cols)
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=V.CANDIDATES_DENSE, arithmetic=V.ARITH_FUSED)
    frames = [V.synth_render_frames([1000 + s for s in range(n_seq)], [k] * n_seq, [base * speed[s] * k for s in range(n_seq)], rows, cols, intr,
                                    invalid_percent=2) for k in range(n_frames)]
    tr = V.Trackers(cfg, n_seq, rows, cols)
    tr.enable_map(0, rows * cols * n_frames, 16)
    for k, (g, d) in enumerate(frames):
        (tr.init if k == 0 else tr.track)(g, d)
    tracked, _, _ = tr.current_frames()
    out = tr.render_map(footprint=2)
    b = V.Batch(cfg, n_seq, rows, cols)
    model_pose = torch.zeros((n_seq, 7), dtype=torch.float32, device="cuda")
    status = torch.zeros(n_seq, dtype=torch.int32, device="cuda")
    b.prepare_keyframes(out["gray"], out["depth"])
    # the rendering is a keyframe AT the tracked pose: track_current composes the solved motion onto it
    b.track_current(frames[-1][0], model_pose, status, prev_poses7=None)
    torch.cuda.synchronize()
    rel = model_pose.cpu().numpy()
    rows_out = []
    for s in range(n_seq):
        # the frame's camera is at exp(xi) (keyframe -> camera): its camera -> world pose is the inverse
        gt = V.iso_inverse(V.se3_exp((base * speed[s] * (n_frames - 1)).astype(np.float32)))
        aligned = V.iso_mul(tracked[s], rel[s])   # the model's pose, then the motion found against it
        rows_out.append(dict(seq=s, status=int(status[s].item()), tracker=pose_error(tracked[s], gt), model=pose_error(aligned, gt),
                             covered=float((out["depth"][s] != 0).float().mean().item())))
    return rows_out


def fmt(t):
    return f"{t['ms']:.3f} ({t['lo']:.3f}-{t['hi']:.3f})"


def summary(a, res):
    n = a.sequences
    lines = [f"# vors_render_points, {n} sequences, {COLS}x{ROWS}, one MI355X", "",
             f"HIP events around one call. A block = median of 20 calls after 3 warm-up calls; the blocks of all legs alternate for {a.blocks} rounds:",
             "a figure is the median of a leg's block medians, (lowest-highest) their range = the run-to-run spread inside this process. ms.",
             "Every point of a list is in view of its sequence's camera (random pixel, depth 0.5-6 m); every plane is preallocated. The splat",
             "alone includes the fill of the key plane, like yardstick (a).", ""]
    for size in SIZES:
        r = res[size]
        lines += [f"## {size} points per sequence ({n * size / 1e6:.2f} M points)", "", "| leg | ms | minima | G minima/s beyond the fill |", "|---|---|---|---|"]
        fill_ms = r[YARD_B]["ms"]
        lines.append(f"| {YARD_B} ({n * ROWS * COLS * 8 / 1e6:.1f} MB) | {fmt(r[YARD_B])} | | |")
        t = r[YARD_A]
        lines.append(f"| {YARD_A}, {r['yard_pairs']} dense pairs ({r['yard_points'] / 1e6:.2f} M points, {r['yard_pairs'] * ROWS * COLS * 8 / 1e6:.1f} MB of keys) | {fmt(t)} | | |")
        for f in (1, 2, 3):
            c = r["counts"][f]
            for leg in (f"footprint {f}, splat alone", f"footprint {f}, depth + grey + counts"):
                t = r[leg]
                minima = c[2] * f * f   # an upper bound: border points write fewer pixels
                rate = f"{minima / (t['ms'] - fill_ms) / 1e6:.1f}" if leg.endswith("alone") and t["ms"] > fill_ms else ""
                lines.append(f"| {leg} | {fmt(t)} | {minima / 1e6:.2f} M | {rate} |")
        c = r["counts"][1]
        lines += ["", f"Footprint 1: {c[0]:.0f} considered, {c[1]:.0f} in front, {c[2]:.0f} landed, {c[3]:.0f} pixels covered of {n * ROWS * COLS}.", ""]
    lines += ["## The loop closed once: frame-to-model alignment, 6 dense sequences x 10 frames, 120x160 / 4 levels", "",
              "The map rendered at the tracked pose of the last frame (footprint 2) is the keyframe of a fresh Batch; the real last frame is tracked",
              "against it. Errors against the synthetic ground truth of that frame: translation in m / rotation in rad. No bound is asserted: the",
              "tolerance of frame-to-model alignment is not known.", "",
              "| sequence | status | pixels covered | tracker's own pose | pose after aligning against the model |", "|---|---|---|---|---|"]
    for r in res["loop"]:
        lines.append(f"| {r['seq']} | {r['status']} | {r['covered']:.3f} | {r['tracker'][0]:.5f} / {r['tracker'][1]:.5f} | {r['model'][0]:.5f} / {r['model'][1]:.5f} |")
    lines += ["", "Sequence 2 (the fastest: 0.11 m per frame) is far off in the tracker's own column: that is the tracker, not the ground truth or the",
              "renderer. The CPU oracle's Tracker on the same frames ends 0.684 m from the ground truth too, with every status OK: from the first",
              "frame on it solves the vertical translation with the wrong sign while x, z and the rotation follow. The model inherits that pose."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_map_summary.md"))
    ap.add_argument("--sequences", type=int, default=SEQS)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    text = summary(a, measure(a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
