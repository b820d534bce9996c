#!/usr/bin/env python
"""Times vors_pose_graph_optimize on the GPU and its host twin on one core (profiles/pose_graph_summary.md):
    1 graph of 65 536 nodes / 262 144 edges, and 64 graphs of 512 nodes / 2 048 edges,
each a chain with random extra edges, exact measurements, the start perturbed. Per shape: ms per outer round and per CG iteration (from
the difference of two calls that differ only in cg_iters, cg_tol = 0 so that every iteration runs), and the achieved share of the byte
model of DESIGN.md 7u, 448 N + 400 E bytes per CG iteration. Prints one JSON line per shape.

    python tools/pose_graph_bench.py [--host-nodes 65536] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-odometry-rs_amd"))
import vors_amd as V  # noqa: E402


def quat_mul(a, b):
    ai, aj, ak, aw = a.T
    bi, bj, bk, bw = b.T
    return np.stack([aw * bi + ai * bw + aj * bk - ak * bj, aw * bj - ai * bk + aj * bw + ak * bi, aw * bk + ai * bj - aj * bi + ak * bw,
                     aw * bw - ai * bi - aj * bj - ak * bk], 1)


def quat_rot(q, p):
    t = 2.0 * np.cross(q[:, :3], p)
    return p + q[:, 3:4] * t + np.cross(q[:, :3], t)


def small_pose(rng, n, trans, rot):
    w = rng.uniform(-rot, rot, (n, 3))
    q = np.concatenate([0.5 * w, np.ones((n, 1))], 1)
    return np.concatenate([rng.uniform(-trans, trans, (n, 3)), q / np.linalg.norm(q, axis=1, keepdims=True)], 1)


def make_graph(nodes, edges, seed):
    """A random walk of `nodes` poses, chain edges and random extra ones up to `edges`; exact measurements M_ij = T_j^-1 T_i."""
    rng = np.random.default_rng(seed)
    steps = small_pose(rng, nodes, 0.2, 0.2)
    truth = np.zeros((nodes, 7))
    truth[0, 6] = 1
    for k in range(1, nodes):  # (sequential composition; vectorised over nothing, 65 536 steps take a second)
        truth[k, :3] = truth[k - 1, :3] + quat_rot(truth[k - 1:k, 3:], steps[k:k + 1, :3])[0]
        truth[k, 3:] = quat_mul(truth[k - 1:k, 3:], steps[k:k + 1, 3:])[0]
    i = np.concatenate([np.arange(nodes - 1), rng.integers(0, nodes, edges - (nodes - 1))])
    j = np.concatenate([np.arange(1, nodes), rng.integers(0, nodes, edges - (nodes - 1))])
    j = np.where(i == j, (j + 1) % nodes, j)
    qi = truth[j, 3:] * np.array([-1, -1, -1, 1])
    meas = np.concatenate([quat_rot(qi, truth[i, :3] - truth[j, :3]), quat_mul(qi, truth[i, 3:])], 1)
    noise = small_pose(rng, nodes, 0.05, 0.05)
    noise[0] = [0, 0, 0, 0, 0, 0, 1]
    start = np.concatenate([truth[:, :3] + quat_rot(truth[:, 3:], noise[:, :3]), quat_mul(truth[:, 3:], noise[:, 3:])], 1)
    return start.astype(np.float32), np.stack([i, j], 1).astype(np.int32), meas.astype(np.float32)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-nodes", type=int, default=65536, help="the host twin is skipped for graphs with more nodes")
    args = ap.parse_args()
    for n, nodes, edges in ((1, 65536, 262144), (64, 512, 2048)):
        graphs = [make_graph(nodes, edges, 100 + g) for g in range(n)]
        dev = lambda k, dt: torch.from_numpy(np.stack([g[k] for g in graphs])).cuda().to(dt)  # noqa: E731
        a = dict(poses=dev(0, torch.float32), edges=dev(1, torch.int32), meas=dev(2, torch.float32),
                 node_counts=torch.full((n,), nodes, dtype=torch.int32, device="cuda"),
                 edge_counts=torch.full((n,), edges, dtype=torch.int32, device="cuda"))
        ws = torch.empty(V.pose_graph_workspace_bytes(n, nodes, edges), dtype=torch.uint8, device="cuda")

        def gpu_ms(iters, cg_iters):
            best = float("inf")
            for _ in range(args.reps + 1):  # (the first call is the warm-up)
                torch.cuda.synchronize()
                t = time.perf_counter()
                out = V.pose_graph_optimize(**a, iters=iters, cg_iters=cg_iters, cg_tol=0.0, step_eps=0.0, workspace=ws)
                torch.cuda.synchronize()
                best = min(best, (time.perf_counter() - t) * 1e3)
            return best, V.decode_pose_graph_stats(out["stats"])

        rounds = 4
        t0, _ = gpu_ms(0, 8)
        t8, s8 = gpu_ms(rounds, 8)
        t40, s40 = gpu_ms(rounds, 40)
        cg_ms = (t40 - t8) / (rounds * 32)
        model_bytes = n * (448 * nodes + 400 * edges)
        rec = dict(graphs=n, nodes=nodes, edges=edges, workspace_mib=round(ws.numel() / 2 ** 20, 1), evaluate_ms=round(t0, 3),
                   round_ms_cg8=round((t8 - t0) / rounds, 3), round_ms_cg40=round((t40 - t0) / rounds, 3), cg_iteration_ms=round(cg_ms, 4),
                   cg_iterations_run=[int(s8["cg_iterations"].sum()), int(s40["cg_iterations"].sum())],
                   byte_model_mb_per_cg_iteration=round(model_bytes / 1e6, 2), achieved_gb_s=round(model_bytes / (cg_ms * 1e-3) / 1e9, 1),
                   share_of_8_tb_s=round(model_bytes / (cg_ms * 1e-3) / 8e12, 4), energy=[float(s40["initial_energy"][0]), float(s40["final_energy"][0])])
        if nodes <= args.host_nodes:
            torch.set_num_threads(1)
            t = time.perf_counter()
            h = V.pose_graph_optimize_host(*graphs[0], iters=rounds, cg_iters=40, cg_tol=0.0, step_eps=0.0)
            host_ms = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            V.pose_graph_optimize_host(*graphs[0], iters=rounds, cg_iters=8, cg_tol=0.0, step_eps=0.0)
            host8_ms = (time.perf_counter() - t) * 1e3
            same = h["poses"].view(np.uint32) == V.pose_graph_optimize(**a, iters=rounds, cg_iters=40, cg_tol=0.0, step_eps=0.0)["poses"][0].cpu().numpy().view(np.uint32)
            rec.update(host_one_graph_ms_cg40=round(host_ms, 1), host_cg_iteration_ms=round((host_ms - host8_ms) / (rounds * 32), 3),
                       host_all_graphs_ms_cg40=round(host_ms * n, 1), device_equals_host_bits=bool(same.all()))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
