"""Pose-graph optimisation on the host (vors_pose_graph_optimize_host; needs no GPU): lie.h pg_* and the fixed order of the sums, the
texts the kernels run, held against the float64 numpy restatement of tests/pose_graph_cases.py (the same residual and energy, Gauss-Newton
with numerically differentiated Jacobians, a dense solve).

Measured here (recorded in profiles/pose_graph_summary.md as well), every bound 4 x the measurement:

  closed-form Jacobians, 32 random edges, rotations up to 1 rad, E.q.w of both signs (16 negative): largest |r32 - r64| 2.54e-07;
      largest |J_i - central differences| 3.10e-07, |J_j - ...| 3.11e-07 (entries of size 1; the differences' own error at h = 1e-6
      is below 1e-9).
  consistent graphs (exact measurements, start up to 5 cm / 0.05 rad off), 16 rounds of 64 CG iterations, lambda0 1e-4: error against
      the truth (translation m, rotation rad): ring 1.04e-06 / 9.9e-08, chain 3.5e-07 / 1.33e-07, star 3.3e-07 / 1.8e-07. All CONVERGED.
  noisy ring, random SPD information: final energy 0.0076709636 against the restatement's minimum 0.0076711511, relative 2.44e-05;
      poses within 1.59e-06 m / 4.5e-07 rad of the restatement's minimiser.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_graph_cases as P
import vors_amd as V

MEASURED_RESIDUAL_DIFF = 2.54e-07
MEASURED_JACOBIAN_DIFF = 3.11e-07
RESIDUAL_BOUND = 4 * MEASURED_RESIDUAL_DIFF
JACOBIAN_BOUND = 4 * MEASURED_JACOBIAN_DIFF
MEASURED_TRUTH_ERR = {"ring": (1.04e-06, 9.9e-08), "chain": (3.5e-07, 1.33e-07), "star": (3.3e-07, 1.8e-07)}  # m, rad
MEASURED_ENERGY_REL = 2.44e-05
MEASURED_MINIMISER_ERR = (1.59e-06, 4.5e-07)
SOLVE = dict(iters=16, cg_iters=64)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "visual-odometry-rs_amd", "csrc")


def f64(v):
    return np.asarray(v, np.float32).astype(np.float64)


def random_edges(count=32, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for e in range(count):
        ti, tj = P.random_pose(rng, 1, 1), P.random_pose(rng, 1, 1)
        m = P.iso_mul(P.measurement(ti, tj), P.random_pose(rng, 0.3, 1.0))
        if e % 2:
            m = np.concatenate([m[:3], -m[3:]])  # the same rotation, E.q.w of the other sign
        out.append((ti.astype(np.float32), tj.astype(np.float32), m.astype(np.float32)))
    return out


def test_closed_form_jacobians():
    edges = random_edges()
    poses = np.array([p for ti, tj, _ in edges for p in (ti, tj)], np.float32)
    idx = np.arange(2 * len(edges), dtype=np.uint32).reshape(-1, 2)
    meas = np.array([m for _, _, m in edges], np.float32)
    out = V.pose_graph_optimize_host(poses, idx, meas, iters=0)
    assert (out["poses"].view(np.uint32) == poses.view(np.uint32)).all()
    dr = dji = djj = 0.0
    negative = 0
    for e, (ti, tj, m) in enumerate(edges):
        r, ji, jj = V.pose_graph_jacobians_host(ti, tj, m)
        assert (r.view(np.uint32) == out["edge_residuals"][e].view(np.uint32)).all()  # one text
        r64 = P.residual(f64(ti), f64(tj), f64(m))
        nji, njj = P.numeric_jacobians(f64(ti), f64(tj), f64(m))
        negative += P.iso_mul(P.iso_mul(P.iso_inv(f64(ti)), f64(tj)), f64(m))[6] < 0
        dr, dji, djj = max(dr, np.abs(r - r64).max()), max(dji, np.abs(ji - nji).max()), max(djj, np.abs(jj - njj).max())
    print(f"residual {dr:.3g}  J_i {dji:.3g}  J_j {djj:.3g}  E.q.w < 0: {negative} of {len(edges)}")
    assert 8 <= negative <= 24
    assert dr <= RESIDUAL_BOUND and dji <= JACOBIAN_BOUND and djj <= JACOBIAN_BOUND


@pytest.mark.parametrize("name", ["ring", "chain", "star"])
def test_consistent_graph_returns_to_the_truth(name):
    g = getattr(P, name)()
    out = V.pose_graph_optimize_host(g["poses"], g["edges"], g["meas"], **SOLVE)
    dt, dr = P.pose_error(out["poses"], g["truth"])
    print(name, out["stats"], f"error {dt:.3g} m {dr:.3g} rad; start {P.pose_error(g['poses'], g['truth'])}")
    assert out["stats"]["status"] == V.PG_CONVERGED
    assert out["stats"]["valid_edges"] == len(g["edges"]) and out["stats"]["free_nodes"] == len(g["poses"]) - 1
    assert dt <= 4 * MEASURED_TRUTH_ERR[name][0] and dr <= 4 * MEASURED_TRUTH_ERR[name][1]
    assert (out["poses"][0].view(np.uint32) == g["poses"][0].view(np.uint32)).all()  # the gauge


def test_star_hub_has_a_long_incidence_list():
    g = P.star()
    assert (g["edges"] == 1).sum() == 200


def test_noisy_ring_against_the_restatement():
    g = P.noisy_ring()
    ref = P.gauss_newton(g["poses"], g["edges"], g["meas"], g["info"], rounds=6)
    e_ref = P.energy(ref, g["edges"], g["meas"], g["info"])
    out = V.pose_graph_optimize_host(g["poses"], g["edges"], g["meas"], g["info"], **SOLVE)
    rel = abs(float(out["stats"]["final_energy"]) - e_ref) / e_ref
    dt, dr = P.pose_error(out["poses"], ref)
    print(out["stats"], f"minimum {e_ref:.10g} relative {rel:.3g}; minimiser {dt:.3g} m {dr:.3g} rad")
    assert out["stats"]["status"] != V.PG_SINGULAR
    assert rel <= 4 * MEASURED_ENERGY_REL
    assert dt <= 4 * MEASURED_MINIMISER_ERR[0] and dr <= 4 * MEASURED_MINIMISER_ERR[1]
    # the energy never increases over accepted steps: the kept energy after k rounds, k = 0 .. 8
    kept = [float(V.pose_graph_optimize_host(g["poses"], g["edges"], g["meas"], g["info"], iters=k, cg_iters=64)["stats"]["final_energy"])
            for k in range(9)]
    assert kept[0] == float(out["stats"]["initial_energy"])
    assert all(b <= a for a, b in zip(kept, kept[1:])) and kept[-1] < kept[0]


def bits(out):
    return {k: np.ascontiguousarray(v).view(np.uint8).tobytes() for k, v in out.items()}


def test_evaluator_and_fixed_nodes_keep_their_bits():
    g = P.ring()
    out = V.pose_graph_optimize_host(g["poses"], g["edges"], g["meas"], iters=0)
    assert (out["poses"].view(np.uint32) == g["poses"].view(np.uint32)).all()
    assert out["stats"]["status"] == V.PG_ITERATIONS and out["stats"]["initial_energy"] == out["stats"]["final_energy"]
    e64 = P.energy(g["poses"], g["edges"], g["meas"])
    assert abs(float(out["stats"]["final_energy"]) - e64) <= 1e-5 * e64
    assert np.allclose(out["edge_energy"].astype(np.float64).sum(), e64, rtol=1e-5)
    fixed = np.zeros(len(g["poses"]), np.uint8)
    fixed[[3, 11]] = 1
    out = V.pose_graph_optimize_host(g["poses"], g["edges"], g["meas"], fixed=fixed, **SOLVE)
    assert (out["poses"][[3, 11]].view(np.uint32) == g["poses"][[3, 11]].view(np.uint32)).all()
    assert out["stats"]["fixed_nodes"] == 2 and out["stats"]["free_nodes"] == len(g["poses"]) - 2


def test_skipped_edges_change_no_other_bit():
    g = P.noisy_ring()
    base = V.pose_graph_optimize_host(g["poses"], g["edges"], g["meas"], g["info"], np.ones(len(g["edges"]), np.float32), iters=4, cg_iters=16)
    bad_meas = g["meas"][0].copy()
    bad_meas[4] = np.nan
    bad_info = g["info"][0].copy()
    bad_info[7] = np.inf
    extra = [((2, 5), bad_meas, g["info"][0], 1.0), ((2, 5), g["meas"][0], g["info"][0], 0.0), ((4, 4), g["meas"][0], g["info"][0], 1.0),
             ((2, 99), g["meas"][0], g["info"][0], 1.0), ((2, 5), g["meas"][0], bad_info, 1.0), ((2, 5), g["meas"][0], g["info"][0], -1.0),
             ((2, 5), g["meas"][0], g["info"][0], np.nan)]
    edges = np.concatenate([g["edges"], np.array([x[0] for x in extra], np.uint32)])
    meas = np.concatenate([g["meas"], np.array([x[1] for x in extra], np.float32)])
    info = np.concatenate([g["info"], np.array([x[2] for x in extra], np.float32)])
    weight = np.concatenate([np.ones(len(g["edges"]), np.float32), np.array([x[3] for x in extra], np.float32)])
    out = V.pose_graph_optimize_host(g["poses"], edges, meas, info, weight, iters=4, cg_iters=16)
    assert out["stats"]["skipped_edges"] == len(extra) and out["stats"]["valid_edges"] == len(g["edges"])
    assert np.isnan(out["edge_residuals"][len(g["edges"]):]).all() and np.isnan(out["edge_energy"][len(g["edges"]):]).all()
    a, b = bits(base), bits(out)
    assert a["poses"] == b["poses"]
    n = len(g["edges"])
    assert bits({"r": base["edge_residuals"]})["r"] == bits({"r": out["edge_residuals"][:n]})["r"]
    assert bits({"e": base["edge_energy"]})["e"] == bits({"e": out["edge_energy"][:n]})["e"]
    for field in base["stats"].dtype.names:
        if field != "skipped_edges":
            assert base["stats"][field].tobytes() == out["stats"][field].tobytes(), field


def test_isolated_nodes_and_graphs_without_a_valid_edge():
    g = P.ring()
    poses = np.concatenate([g["poses"], g["poses"][5:7]])  # two nodes nobody refers to
    out = V.pose_graph_optimize_host(poses, g["edges"], g["meas"], **SOLVE)
    assert out["stats"]["isolated_nodes"] == 2 and out["stats"]["status"] == V.PG_CONVERGED
    assert (out["poses"][-2:].view(np.uint32) == poses[-2:].view(np.uint32)).all()
    alone = V.pose_graph_optimize_host(g["poses"], g["edges"], g["meas"], **SOLVE)
    assert (out["poses"][:-2].view(np.uint32) == alone["poses"].view(np.uint32)).all()
    # no valid edge: every weight zero; and no edge at all; and no free node
    for kwargs in (dict(edge_weight=np.zeros(len(g["edges"]), np.float32)), dict(edge_count=0), dict(fixed=np.ones(len(g["poses"]), np.uint8))):
        out = V.pose_graph_optimize_host(g["poses"], g["edges"], g["meas"], **kwargs, **SOLVE)
        assert out["stats"]["status"] == V.PG_TOO_FEW
        assert (out["poses"].view(np.uint32) == g["poses"].view(np.uint32)).all()
        assert out["stats"]["accepted_steps"] == 0 and out["stats"]["cg_iterations"] == 0
    assert out["stats"]["final_energy"] > 0  # (every node fixed: the edges are still evaluated)


def test_null_information_equals_identity_bit_for_bit():
    g = P.ring()
    g["meas"] = P.noisy_ring()["meas"]
    eye = np.tile(np.eye(6, dtype=np.float32).reshape(36), (len(g["edges"]), 1))
    a = V.pose_graph_optimize_host(g["poses"], g["edges"], g["meas"], None, iters=6, cg_iters=32)
    b = V.pose_graph_optimize_host(g["poses"], g["edges"], g["meas"], eye, iters=6, cg_iters=32)
    assert bits(a) == bits(b) and a["stats"]["accepted_steps"] > 0


def test_every_refusal_writes_nothing():
    g = P.ring()
    lib = V.lib()
    n, e = len(g["poses"]), len(g["edges"])
    good = dict(poses=g["poses"], node_count=n, node_capacity=n, edges=g["edges"], edge_count=e, edge_capacity=e, meas=g["meas"], info=None,
                weight=None, fixed=None, lambda0=1e-4, step_eps=1e-6, cg_tol=1e-6, iters=4, cg_iters=16)
    cases = [dict(poses=None), dict(edges=None), dict(meas=None), dict(node_capacity=0), dict(edge_capacity=0), dict(lambda0=-1.0),
             dict(lambda0=float("nan")), dict(step_eps=float("nan")), dict(step_eps=-1e-3), dict(cg_tol=-1.0), dict(cg_tol=float("nan")),
             dict(iters=-1), dict(iters=65), dict(cg_iters=0), dict(cg_iters=257), dict(out_poses=None), dict(misaligned=True)]
    for case in [{}] + cases:
        a = dict(good, **{k: v for k, v in case.items() if k in good})
        out_poses = np.full((n, 7), 7.5, np.float32)
        stats = np.full(13, 0xA5A5A5A5, np.uint32)
        res = np.full((e, 6), 7.5, np.float32)
        en = np.full(e, 7.5, np.float32)
        ptr = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)  # noqa: E731
        meas_ptr = ptr(a["meas"])
        if case.get("misaligned"):
            meas_ptr = C.c_void_p(a["meas"].ctypes.data + 2)
        st = lib.vors_pose_graph_optimize_host(ptr(a["poses"]), a["node_count"], a["node_capacity"], ptr(a["edges"]), a["edge_count"],
                                               a["edge_capacity"], meas_ptr, ptr(a["info"]), ptr(a["weight"]), ptr(a["fixed"]), a["lambda0"],
                                               a["step_eps"], a["cg_tol"], a["iters"], a["cg_iters"],
                                               None if "out_poses" in case else ptr(out_poses), ptr(stats), ptr(res), ptr(en))
        if not case:
            assert st == 0 and (out_poses != 7.5).any() and stats[0] != 0xA5A5A5A5
            continue
        assert st != 0, case
        assert lib.vors_last_error().decode().startswith("pose_graph_optimize_host: "), case
        assert (out_poses == 7.5).all() and (stats == 0xA5A5A5A5).all() and (res == 7.5).all() and (en == 7.5).all(), case


def test_host_twin_under_the_sanitizers():
    """A stand-alone program (its own main) built with -fsanitize=address,undefined drives the twin; nothing is loaded into Python."""
    subprocess.check_call(["make", "-C", CSRC, "-s", "pose_graph_host_check"])
    out = subprocess.run([os.path.join(CSRC, "pose_graph_host_check")], capture_output=True, text=True)
    assert out.returncode == 0 and "pose_graph_host_check: ok" in out.stdout, out.stdout + out.stderr
