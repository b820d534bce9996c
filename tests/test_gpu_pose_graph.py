"""Pose-graph optimisation on the device (vors_pose_graph_optimize, include/vors_hip.h 2g) against its host twin, BIT FOR BIT: poses,
stats, per-edge residuals and energies; independence of a graph from its neighbours, the capacities and the stream; the refusals; and the
measurement convention against the tracker's own outputs (lm_model and info36 fed unchanged).

Graphs (tests/pose_graph_cases.py): a 23 x 23 grid with 1032 edges cut at 1000 and at 1025 edges (one and two energy chunks), a 33 x 33
grid (1089 nodes: two node chunks), the star whose hub has 200 edges with skipped edges of every kind appended, the noisy ring with
information matrices, and an empty graph."""
import numpy as np
import pytest

import pose_graph_cases as P
import vors_amd as V

pytestmark = pytest.mark.gpu
SOLVE = dict(lambda0=1e-4, step_eps=1e-6, cg_tol=1e-6, cg_iters=12)


def with_skipped(g):
    g = dict(g)
    n = len(g["edges"])
    bad = g["meas"][0].copy()
    bad[2] = np.nan
    g["edges"] = np.concatenate([g["edges"], np.array([(2, 5), (3, 3), (2, 100000), (6, 7)], np.uint32)])
    g["meas"] = np.concatenate([g["meas"], np.stack([bad, g["meas"][1], g["meas"][2], g["meas"][3]])])
    g["weight"] = np.concatenate([np.ones(n, np.float32), np.array([1, 1, 1, 0], np.float32)])
    return g


def cases():
    if not hasattr(cases, "made"):
        small = P.grid(23, extra=20)
        assert len(small["edges"]) == 1032
        ring = P.noisy_ring()
        ring["weight"] = np.linspace(0.5, 2.0, len(ring["edges"])).astype(np.float32)
        cases.made = dict(grid1000=dict(small, edge_count=1000), grid1025=dict(small, edge_count=1025), grid33=P.grid(33),
                          star=with_skipped(P.star()), ring=ring, empty=dict(P.ring(), node_count=0, edge_count=0))
        assert len(cases.made["grid33"]["poses"]) > 1024
    return cases.made


BATCHES = {"a": ("grid1000", "star", "empty"), "b": ("grid1025", "grid33", "ring")}
_twin = {}


def twin(name, iters):
    """The host twin on one graph alone with tight capacities, computed once per (graph, iters)."""
    if (name, iters) not in _twin:
        g = cases()[name]
        _twin[name, iters] = V.pose_graph_optimize_host(g["poses"], g["edges"], g["meas"], g.get("info"), g.get("weight"), iters=iters,
                                                        node_count=g.get("node_count"), edge_count=g.get("edge_count"), **SOLVE)
    return _twin[name, iters]


def pack(names, width=7, slack=(0, 0), with_info=True):
    """The graphs of `names` as one batch -> the device arguments of pose_graph_optimize."""
    import torch
    gs = [cases()[k] for k in names]
    ncap, ecap = max(len(g["poses"]) for g in gs) + slack[0], max(len(g["edges"]) for g in gs) + slack[1]
    n = len(gs)
    poses = np.full((n, ncap, width), 3.25, np.float32)
    edges = np.full((n, ecap, 2), 0, np.int32)
    meas = np.zeros((n, ecap, 7), np.float32)
    meas[:, :, 6] = 1
    info = np.tile(np.eye(6, dtype=np.float32).reshape(36), (n, ecap, 1))
    weight = np.ones((n, ecap), np.float32)
    counts = np.zeros((2, n), np.int32)
    for k, g in enumerate(gs):
        poses[k, :len(g["poses"]), :7] = g["poses"]
        edges[k, :len(g["edges"])] = g["edges"].view(np.int32)
        meas[k, :len(g["edges"])] = g["meas"]
        if "info" in g:
            info[k, :len(g["edges"])] = g["info"]
        if "weight" in g:
            weight[k, :len(g["edges"])] = g["weight"]
        counts[0, k] = g.get("node_count", len(g["poses"]))
        counts[1, k] = g.get("edge_count", len(g["edges"]))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return dict(poses=dev(poses), node_counts=dev(counts[0]), edges=dev(edges), edge_counts=dev(counts[1]), meas=dev(meas),
                info=dev(info) if with_info else None, edge_weight=dev(weight))


def assert_equals_twin(out, names, iters):
    import torch
    torch.cuda.synchronize()
    stats = V.decode_pose_graph_stats(out["stats"])
    poses, res, en = out["poses"].cpu().numpy(), out["edge_residuals"].cpu().numpy(), out["edge_energy"].cpu().numpy()
    for k, name in enumerate(names):
        t, g = twin(name, iters), cases()[name]
        nn, ne = g.get("node_count", len(g["poses"])), g.get("edge_count", len(g["edges"]))
        assert stats[k].tobytes() == t["stats"].tobytes(), (name, stats[k], t["stats"])
        assert (poses[k, :nn].view(np.uint32) == t["poses"][:nn].view(np.uint32)).all(), name
        assert (res[k, :ne].view(np.uint32) == t["edge_residuals"][:ne].view(np.uint32)).all(), name
        assert (en[k, :ne].view(np.uint32) == t["edge_energy"][:ne].view(np.uint32)).all(), name
        assert np.isnan(en[k, ne:]).all()  # nothing written beyond the count


@pytest.mark.parametrize("iters", [0, 1, 8])
@pytest.mark.parametrize("batch", ["a", "b"])
def test_device_equals_the_host_twin_bit_for_bit(batch, iters):
    names = BATCHES[batch]
    args = pack(names, width=9)  # a pose stride of 36 bytes
    out = V.pose_graph_optimize(**args, iters=iters, edge_residuals=True, edge_energy=True, **SOLVE)
    assert_equals_twin(out, names, iters)
    stats = V.decode_pose_graph_stats(out["stats"])
    if batch == "a":
        assert stats[1]["skipped_edges"] == 4 and stats[2]["status"] == V.PG_TOO_FEW and stats[2]["valid_edges"] == 0
    if iters == 8:
        assert all(s["accepted_steps"] > 0 and s["final_energy"] < s["initial_energy"] for s, k in zip(stats, names) if k != "empty")


def test_a_graph_does_not_depend_on_its_neighbours_or_the_capacities():
    alone = V.pose_graph_optimize(**pack(("ring",)), iters=8, edge_residuals=True, edge_energy=True, **SOLVE)
    assert_equals_twin(alone, ("ring",), 8)
    loose = V.pose_graph_optimize(**pack(("grid33", "ring", "star"), slack=(37, 501)), iters=8, edge_residuals=True, edge_energy=True, **SOLVE)
    assert_equals_twin(loose, ("grid33", "ring", "star"), 8)
    n, e = len(cases()["ring"]["poses"]), len(cases()["ring"]["edges"])
    assert (alone["poses"][0, :n].cpu().numpy().view(np.uint32) == loose["poses"][1, :n].cpu().numpy().view(np.uint32)).all()
    assert (alone["edge_energy"][0, :e].cpu().numpy().view(np.uint32) == loose["edge_energy"][1, :e].cpu().numpy().view(np.uint32)).all()
    assert alone["stats"][0].cpu().numpy().tobytes() == loose["stats"][1].cpu().numpy().tobytes()


def test_null_information_equals_identity_on_the_device():
    names = ("grid1000",)
    a = V.pose_graph_optimize(**pack(names), iters=4, edge_residuals=True, edge_energy=True, **SOLVE)
    b = V.pose_graph_optimize(**pack(names, with_info=False), iters=4, edge_residuals=True, edge_energy=True, **SOLVE)
    for key in a:
        assert a[key].cpu().numpy().tobytes() == b[key].cpu().numpy().tobytes(), key


def test_two_streams_with_separate_workspaces_equal_the_sequential_results():
    import torch
    batches = [pack(BATCHES["a"]), pack(BATCHES["b"])]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = []
    for args, s in zip(batches, streams):
        with torch.cuda.stream(s):
            outs.append(V.pose_graph_optimize(**args, iters=8, edge_residuals=True, edge_energy=True, **SOLVE))
    torch.cuda.synchronize()
    assert_equals_twin(outs[0], BATCHES["a"], 8)
    assert_equals_twin(outs[1], BATCHES["b"], 8)


def test_output_may_alias_packed_input():
    args = pack(("ring", "star"))
    out = V.pose_graph_optimize(**args, iters=8, out=args["poses"], edge_residuals=True, edge_energy=True, **SOLVE)
    assert out["poses"].data_ptr() == args["poses"].data_ptr()
    assert_equals_twin(out, ("ring", "star"), 8)


def test_refusals_enqueue_nothing():
    import torch
    args = pack(("ring",))
    n, ncap, ecap = 1, args["poses"].shape[1], args["edges"].shape[1]
    lib = V.lib()
    ws = torch.empty(V.pose_graph_workspace_bytes(n, ncap, ecap) + 16, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0 and V.pose_graph_workspace_bytes(0, 1, 1) == V.pose_graph_workspace_bytes(1, 0, 1) == 0
    out = torch.full((n, ncap, 7), 7.5, dtype=torch.float32, device="cuda")
    stats = torch.full((n, 52), 0xA5, dtype=torch.uint8, device="cuda")
    res = torch.full((n, ecap, 6), 7.5, dtype=torch.float32, device="cuda")
    en = torch.full((n, ecap), 7.5, dtype=torch.float32, device="cuda")
    dp = V.Batch._dp
    good = dict(n=n, poses=dp(args["poses"]), stride=0, node_counts=dp(args["node_counts"]), ncap=ncap, edges=dp(args["edges"]),
                edge_counts=dp(args["edge_counts"]), ecap=ecap, meas=dp(args["meas"]), lambda0=1e-4, step_eps=1e-6, cg_tol=1e-6, iters=4,
                cg_iters=8, ws=dp(ws), out=dp(out))
    cases_ = [dict(n=0), dict(poses=None), dict(node_counts=None), dict(edges=None), dict(edge_counts=None), dict(meas=None), dict(ws=None),
              dict(out=None), dict(ncap=0), dict(ecap=0), dict(stride=24), dict(stride=30), dict(lambda0=-1.0), dict(lambda0=float("nan")),
              dict(step_eps=float("nan")), dict(cg_tol=-1.0), dict(iters=65), dict(iters=-1), dict(cg_iters=0), dict(cg_iters=257),
              dict(ws=V.C.c_void_p(ws.data_ptr() + 4)), dict(meas=V.C.c_void_p(args["meas"].data_ptr() + 2))]
    for case in cases_:
        a = dict(good, **case)
        st = lib.vors_pose_graph_optimize(a["n"], a["poses"], a["stride"], a["node_counts"], a["ncap"], a["edges"], a["edge_counts"], a["ecap"],
                                          a["meas"], None, None, None, a["lambda0"], a["step_eps"], a["cg_tol"], a["iters"], a["cg_iters"],
                                          a["ws"], a["out"], dp(stats), dp(res), dp(en), V.Batch._stream())
        assert st != 0 and lib.vors_last_error().decode().startswith("pose_graph_optimize: "), case
    torch.cuda.synchronize()
    assert (out == 7.5).all() and (stats == 0xA5).all() and (res == 7.5).all() and (en == 7.5).all()


# Composition rounding of the 7 odometry models, measured with the host twin on these models (printed below and recorded in
# profiles/pose_graph_summary.md): the largest iters = 0 energy of an odometry edge under its own info36, 2.30e-07 (the seven: 1.4e-13
# 5.6e-10 5.6e-08 8.8e-09 7.9e-09 3.6e-08 2.3e-07; the loop edge carries 2.44e+07). Bound: 4 x.
MEASURED_ODOMETRY_ENERGY = 2.30e-07


def test_tracker_outputs_go_in_unchanged():
    """8 synthetic frames, the 7 consecutive pairs and the closing pair (0, 7) in one vors_batch_track_pairs; lm_model and info36 fed
    unchanged. With the poses composed from the odometry models (T_j = T_i M_ij^-1) every odometry edge is consistent up to rounding and
    the loop edge carries the rest; 8 rounds lower the energy. The ATE before and after is printed, NOT asserted."""
    import torch
    rows, cols, levels, frames_n = 120, 160, 4, 8
    intr = V.scaled_intrinsics(rows, cols)
    step = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001])
    xis = [step * k for k in range(frames_n)]
    gray, depth = V.synth_render_frames([500] * frames_n, list(range(frames_n)), xis, rows, cols, intr)
    pairs = [(k, k + 1) for k in range(frames_n - 1)] + [(0, frames_n - 1)]
    ii, jj = [p[0] for p in pairs], [p[1] for p in pairs]
    cfg = V.Config(nb_levels=levels, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), arithmetic=V.ARITH_FUSED)
    b = V.Batch(cfg, len(pairs), rows, cols)
    poses = torch.zeros((len(pairs), 7), dtype=torch.float32, device="cuda")
    status = torch.zeros(len(pairs), dtype=torch.int32, device="cuda")
    stats = V.stats_tensor(len(pairs))
    b.track_pairs(gray[ii].contiguous(), depth[ii].contiguous(), gray[jj].contiguous(), poses, status, stats)
    info = b.pose_information(0, stats)[0]
    torch.cuda.synchronize()
    models = np.ascontiguousarray(V.decode_stats(stats)["lm_model"])
    start = [P.iso_identity()]
    for k in range(frames_n - 1):
        start.append(P.iso_mul(start[-1], P.iso_inv(models[k].astype(np.float64))))
    start = np.array(start, np.float32)
    edges = np.array(pairs, np.int32)
    info36 = info.reshape(len(pairs), 36).contiguous()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    args = dict(poses=dev(start[None]), node_counts=dev(np.array([frames_n], np.int32)), edges=dev(edges[None]),
                edge_counts=dev(np.array([len(pairs)], np.int32)), meas=dev(models[None]), info=info36[None].contiguous())
    before = V.pose_graph_optimize(**args, iters=0, edge_energy=True)
    after = V.pose_graph_optimize(**args, iters=8, cg_iters=32, edge_energy=True)
    torch.cuda.synchronize()
    host = V.pose_graph_optimize_host(start, edges.view(np.uint32), models, info36.cpu().numpy(), iters=0)
    e0 = before["edge_energy"][0].cpu().numpy()
    assert (e0.view(np.uint32) == host["edge_energy"].view(np.uint32)).all()
    s0, s8 = V.decode_pose_graph_stats(before["stats"])[0], V.decode_pose_graph_stats(after["stats"])[0]
    truth = np.array([P.iso_inv(P.se3_exp(x)) for x in xis])  # camera -> world: the renderer's exp(xi) maps the scene into the camera
    ate = lambda p: float(np.sqrt(np.mean(np.sum((p[:, :3].astype(np.float64) - truth[:, :3]) ** 2, axis=1))))  # noqa: E731
    print(f"odometry edge energies at the composed poses {e0[:-1]} (largest {e0[:-1].max():.3g}), loop edge {e0[-1]:.6g}")
    print(f"energy {s0['initial_energy']:.6g} -> {s8['final_energy']:.6g}, status {s8['status']}, accepted {s8['accepted_steps']}, "
          f"rejected {s8['rejected_steps']}, CG iterations {s8['cg_iterations']}")
    print(f"ATE against the renderer's truth: before {ate(start):.6g} m, after {ate(after['poses'][0].cpu().numpy()):.6g} m (a finding, not a bound)")
    assert (e0[:-1] <= 4 * MEASURED_ODOMETRY_ENERGY).all()
    assert e0[-1] >= 0.99 * s0["initial_energy"] and e0[-1] > 100 * e0[:-1].max()
    assert s8["final_energy"] < s0["initial_energy"] and s8["status"] != V.PG_SINGULAR
