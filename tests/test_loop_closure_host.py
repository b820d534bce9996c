"""Loop closure on the host (vors_loop_signatures_host, vors_loop_candidates_host, vors_loop_verify_edges_host; need no GPU): lie.h lc_*,
the texts the kernels run, held against the numpy restatements of tests/loop_closure_cases.py. Signatures, dot products and numerators are
exact integers; the score is one correctly rounded f64 divide — so every comparison here is one of bits, there is no tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loop_closure_cases as L
import pose_graph_cases as P
import vors_amd as V

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "visual-odometry-rs_amd", "csrc")
INVALID = -1  # VORS_ERR_INVALID_ARGUMENT


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_candidates_equal(out, want):
    ci, cs, cc, counts = want
    assert (out["cand"]["i"] == ci).all()
    assert (bits(out["cand"]["score"]) == bits(cs)).all()
    assert (out["cand_counts"] == cc).all() and (out["counts"] == counts).all()
    assert int(out["counts"][1:].sum()) == int(out["counts"][0])


@pytest.mark.parametrize("rows,cols,tr,tc", L.SHAPES)
def test_signatures_equal_the_restatement(rows, cols, tr, tc):
    for plane in L.planes(rows, cols, seed=rows):
        sig, total, sumsq = V.loop_signatures_host(plane, tr, tc)
        want, wsum, wsumsq = L.signature(plane, tr, tc)
        assert (sig == want).all() and total == wsum and sumsq == wsumsq
    assert (V.loop_signatures_host(np.zeros((rows, cols), np.uint8), tr, tc)[0] == -128).all()
    assert (V.loop_signatures_host(np.full((rows, cols), 255, np.uint8), tr, tc)[0] == 127).all()


@pytest.mark.parametrize("min_gap", [1, 10])
@pytest.mark.parametrize("k", [1, 4, 8])
def test_candidates_equal_the_brute_force(min_gap, k):
    sig = L.random_signatures(40, 128, seed=min_gap * 10 + k)
    for min_score in (-2.0, 0.0, 0.05):
        out = V.loop_candidates_host(sig, L.meta_of(sig), min_gap, k, min_score)
        assert_candidates_equal(out, L.candidates(sig, min_gap, k, min_score))
    assert out["cand_counts"].max() <= k


def test_candidates_k_beyond_the_survivors_and_a_query_window():
    sig = L.random_signatures(12, 64, seed=5)
    out = V.loop_candidates_host(sig, L.meta_of(sig), 2, 8, -2.0)
    assert_candidates_equal(out, L.candidates(sig, 2, 8, -2.0))
    assert out["cand_counts"][5] == 4 and (out["cand"]["i"][5, 4:] == L.EMPTY).all() and (out["cand"]["score"][5, 4:] == 0).all()
    assert out["cand_counts"][1] == 0 and (out["cand"]["i"][1] == L.EMPTY).all()
    win = V.loop_candidates_host(sig, L.meta_of(sig), 2, 8, -2.0, query_first=9, count=11)
    assert_candidates_equal(win, L.candidates(sig, 2, 8, -2.0, query_first=9, count=11))
    assert (win["cand"]["i"][:9] == L.EMPTY).all() and (win["cand"]["i"][11] == L.EMPTY).all() and win["counts"][0] == 8 + 9
    assert (win["cand"][9:11] == out["cand"][9:11]).all()


def test_candidates_ties_flat_and_negative_signatures():
    sig = L.special_signatures()
    out = V.loop_candidates_host(sig, L.meta_of(sig), 1, 8, -2.0)
    assert_candidates_equal(out, L.candidates(sig, 1, 8, -2.0))
    # 6 and 7 are identical: every later query scores them equally and lists 6 first; 7 itself finds 6 with a score of exactly 1
    assert out["cand"]["i"][7, 0] == 6 and out["cand"]["score"][7, 0] == 1.0
    for j in range(8, 24):
        where = {int(i): p for p, i in enumerate(out["cand"]["i"][j])}
        if 6 in where and 7 in where:
            assert where[7] == where[6] + 1 and out["cand"]["score"][j, where[6]] == out["cand"]["score"][j, where[7]]
    assert any(6 in out["cand"]["i"][j] and 7 in out["cand"]["i"][j] for j in range(8, 24))
    # the flat one is counted and never returned, as candidate or as query
    assert out["counts"][1] == 23 and not (out["cand"]["i"] == 11).any() and out["cand_counts"][11] == 0
    # the negative image scores exactly -1: last of all at min_score -2, score-gated at -0.5
    k15 = L.candidates(sig, 1, 24, -2.0)
    assert k15[0][15, k15[2][15] - 1] == 2 and k15[1][15, k15[2][15] - 1] == -1.0
    gated = V.loop_candidates_host(sig, L.meta_of(sig), 1, 8, -0.5)
    assert_candidates_equal(gated, L.candidates(sig, 1, 8, -0.5))
    assert 2 not in gated["cand"]["i"][15] and gated["counts"][3] > 0


@pytest.mark.parametrize("max_dist_m,min_qdot", [(0.0, 0.0), (0.55, 0.0), (0.0, 0.9), (0.55, 0.9)])
def test_candidates_pose_gate_each_half_on_and_off(max_dist_m, min_qdot):
    sig = L.random_signatures(24, 64, seed=9)
    poses = L.line_poses(24)
    for r in range(0, 24, 3):  # every third keyframe looks the other way: |q_i . q_j| = cos(0.6) < 0.9 against the others
        poses[r, 3:] = L.f32(P.se3_exp([0, 0, 0, 0, 1.2, 0]))[3:]
    out = V.loop_candidates_host(sig, L.meta_of(sig), 1, 8, -2.0, poses=poses, max_dist_m=max_dist_m, min_qdot=min_qdot)
    assert_candidates_equal(out, L.candidates(sig, 1, 8, -2.0, poses, max_dist_m, min_qdot))
    assert (out["counts"][2] > 0) == (max_dist_m > 0 or min_qdot > 0)
    if max_dist_m > 0:
        assert all(j - int(i) <= 5 for j in range(24) for i in out["cand"]["i"][j] if i != L.EMPTY)
    if min_qdot > 0:
        assert all((j % 3 == 0) == (int(i) % 3 == 0) for j in range(24) for i in out["cand"]["i"][j] if i != L.EMPTY)


def test_candidates_a_pose_that_is_not_finite_fails_a_half_that_is_on():
    sig = L.random_signatures(9, 64, seed=2)  # query 8 has the 8 candidates its list can hold
    poses = L.line_poses(9, 0.01)
    poses[2, 1], poses[5, 5] = np.nan, np.inf
    for dist, qdot, gone in ((1.0, 0.0, {2}), (0.0, 0.5, {5}), (1.0, 0.5, {2, 5}), (0.0, 0.0, set())):
        out = V.loop_candidates_host(sig, L.meta_of(sig), 1, 8, -2.0, poses=poses, max_dist_m=dist, min_qdot=qdot)
        assert_candidates_equal(out, L.candidates(sig, 1, 8, -2.0, poses, dist, qdot))
        listed = set(int(i) for i in out["cand"]["i"][8])
        assert all((r in listed) == (r not in gone) for r in (2, 5))
        assert all(out["cand_counts"][r] == 0 for r in gone)


# ---- verification
def consistent(poses, i, j):
    return P.iso_mul(P.iso_inv(poses[j]), poses[i])


def one(model_fwd, model_bwd=None, pair=(0, 1), poses=None, info=None, sf=0, sb=0, **kw):
    args = dict(L.VERIFY_BOUNDS)
    args.update(kw)
    return V.loop_verify_edges_host([pair], [L.f32(model_fwd)], [sf], 4, model_bwd=None if model_bwd is None else [L.f32(model_bwd)],
                                    status_bwd=None if model_bwd is None else [sb], info=info, poses=poses, **args)


def test_verify_reaches_every_verdict_and_keeps_the_precedence():
    rng = np.random.default_rng(1)
    poses = np.array([P.random_pose(rng, 1.0, 1.0) for _ in range(3)])
    p32 = L.f32(poses)
    m = consistent(poses, 0, 1)
    off_t, off_r = P.se3_exp([0.2, 0, 0, 0, 0, 0]), P.se3_exp([0, 0, 0, 0.2, 0, 0])
    nan_model = np.array(m)
    nan_model[2] = np.nan
    cases = [
        (V.LOOP_ACCEPTED, dict(model_fwd=m, model_bwd=P.iso_inv(m), poses=p32)),
        (V.LOOP_ACCEPTED, dict(model_fwd=m)),
        (V.LOOP_STATUS, dict(model_fwd=m, model_bwd=P.iso_inv(m), poses=p32, sf=1)),
        (V.LOOP_STATUS, dict(model_fwd=m, model_bwd=P.iso_inv(m), poses=p32, sb=1)),
        (V.LOOP_INDEX, dict(model_fwd=m, pair=(1, 1))),
        (V.LOOP_INDEX, dict(model_fwd=m, pair=(0, 3), poses=p32)),
        (V.LOOP_ACCEPTED, dict(model_fwd=m, pair=(0, 3))),  # without poses an index has no range
        (V.LOOP_NONFINITE, dict(model_fwd=nan_model)),
        (V.LOOP_NONFINITE, dict(model_fwd=m, model_bwd=nan_model)),
        (V.LOOP_NONFINITE, dict(model_fwd=m, info=np.full((1, 36), np.inf, np.float32))),
        (V.LOOP_CYCLE_TRANS, dict(model_fwd=m, model_bwd=P.iso_mul(off_t, P.iso_inv(m)))),
        (V.LOOP_CYCLE_ROT, dict(model_fwd=m, model_bwd=P.iso_mul(off_r, P.iso_inv(m)))),
        (V.LOOP_PRIOR_TRANS, dict(model_fwd=P.iso_mul(m, off_t), model_bwd=P.iso_inv(P.iso_mul(m, off_t)), poses=p32)),
        (V.LOOP_PRIOR_ROT, dict(model_fwd=P.iso_mul(m, off_r), model_bwd=P.iso_inv(P.iso_mul(m, off_r)), poses=p32)),
        # precedence: the first rule that applies
        (V.LOOP_STATUS, dict(model_fwd=nan_model, pair=(1, 1), sf=1)),
        (V.LOOP_INDEX, dict(model_fwd=nan_model, pair=(1, 1))),
        (V.LOOP_CYCLE_TRANS, dict(model_fwd=P.iso_mul(m, off_t), model_bwd=P.iso_inv(m), poses=p32)),  # cycle and prior both off
        (V.LOOP_CYCLE_TRANS, dict(model_fwd=m, model_bwd=P.iso_mul(P.iso_mul(off_t, off_r), P.iso_inv(m)))),  # translation before rotation
        # a bound of 0 switches its test off
        (V.LOOP_CYCLE_ROT, dict(model_fwd=m, model_bwd=P.iso_mul(P.iso_mul(off_t, off_r), P.iso_inv(m)), max_cycle_trans=0.0)),
        (V.LOOP_ACCEPTED, dict(model_fwd=P.iso_mul(m, off_t), poses=p32, max_prior_trans=0.0)),
    ]
    for want, kw in cases:
        out = one(**kw)
        assert out["verdict"][0] == want, (want, kw.keys(), out["verdict"], out["residuals"])
        assert out["counts"][want] == 1 and out["counts"].sum() == 1
        assert out["edge_count"] == (1 if want == V.LOOP_ACCEPTED else 0)
    r = one(model_fwd=m, model_bwd=P.iso_mul(off_t, P.iso_inv(m)), poses=p32)["residuals"][0]
    assert abs(r[0] - 0.2) < 1e-6 and np.abs(r[1:6]).max() < 1e-6 and np.abs(r[6:]).max() < 1e-6  # both residuals, whatever the verdict
    r = one(model_fwd=m, sf=1)["residuals"][0]
    assert np.isnan(r).all()
    r = one(model_fwd=m)["residuals"][0]
    assert np.isnan(r).all()  # no backward model, no poses: neither residual exists


def test_verify_appends_in_candidate_order_from_the_incoming_count_and_reports_capacity():
    case, kind = L.verify_cases(40, seed=4)
    ecap = 6
    edges = np.full((ecap, 2), 77, np.uint32)
    meas = np.full((ecap, 7), 7.5, np.float32)
    out = V.loop_verify_edges_host(edge_capacity=ecap, edges=edges, meas=meas, edge_count=3, weight=0.25, **case, **L.VERIFY_BOUNDS)
    good = [e for e in range(40) if kind[e] == 0]
    assert len(good) > ecap - 3 and len(good) < 40 - 8
    fit, over = good[:ecap - 3], good[ecap - 3:]
    want = np.array([L.EXPECTED_VERDICT[int(k)] for k in kind], np.uint32)
    want[over] = V.LOOP_CAPACITY
    assert (out["verdict"] == want).all() and out["edge_count"] == ecap
    assert (out["edges"][:3] == 77).all() and (out["meas"][:3] == 7.5).all() and np.isnan(out["edge_weight"][:3]).all()
    assert (out["edges"][3:] == case["pairs"][fit]).all() and (bits(out["meas"][3:]) == bits(case["model_fwd"][fit])).all()
    assert (bits(out["info"][3:]) == bits(case["info"][fit])).all() and (out["edge_weight"][3:] == 0.25).all()
    assert (out["counts"] == np.bincount(want, minlength=V.LOOP_VERDICTS)).all()
    # no information given: identity rows
    case.pop("info")
    ident = V.loop_verify_edges_host(edge_capacity=64, **case, **L.VERIFY_BOUNDS)
    assert ident["edge_count"] == len(good) and (ident["info"][:len(good)] == np.eye(6, dtype=np.float32).reshape(36)).all()
    assert np.isnan(ident["info"][len(good):]).all()
    # an incoming count above the capacity is clipped to it: nothing is appended
    full = V.loop_verify_edges_host(edge_capacity=5, edge_count=9, **case, **L.VERIFY_BOUNDS)
    assert full["edge_count"] == 5 and (full["edges"] == L.EMPTY).all() and (full["verdict"][good] == V.LOOP_CAPACITY).all()


def test_end_to_end_on_the_host_the_verdicts_keep_the_graph_from_the_false_edge():
    """8 poses on a circle of 1 m; odometry drifts by 2 mm per step and by 0.3 m in the badly tracked step 3 -> 4, whose information is a
    hundredth of the others'; for (0, 7) a true candidate and a false one 0.5 m off, with a hundred times the information and a backward
    model that is the genuine inverse of ANOTHER motion: DESIGN.md 7u's finding. A check of the plumbing, with wide margins."""
    ang = np.arange(8) * (2 * np.pi / 9)
    truth = np.array([P.iso_mul(P.se3_exp([0, 0, 0, 0, a, 0]), P.se3_exp([1.0, 0, 0, 0, 0, 0])) for a in ang])
    drift, slip = P.se3_exp([0.002, 0.0, 0.001, 0, 0.0004, 0]), P.se3_exp([0.3, 0.0, 0.1, 0, 0.02, 0])
    odo = [P.iso_mul(consistent(truth, k, k + 1), slip if k == 3 else drift) for k in range(7)]
    start = [truth[0]]
    for k in range(7):
        start.append(P.iso_mul(start[-1], P.iso_inv(odo[k])))
    start = L.f32(start)
    ate = lambda p: float(np.sqrt(np.mean(np.sum((np.asarray(p, np.float64)[:, :3] - truth[:, :3]) ** 2, axis=1))))  # noqa: E731
    true_m = consistent(truth, 0, 7)
    false_m = P.iso_mul(true_m, P.se3_exp([0.5, 0, 0, 0, 0, 0]))
    other = P.iso_mul(true_m, P.se3_exp([0.1, 0.3, 0, 0, 0, 0]))
    ecap = 9
    edges = np.zeros((ecap, 2), np.uint32)
    edges[:7] = [(k, k + 1) for k in range(7)]
    meas = np.zeros((ecap, 7), np.float32)
    meas[:7] = L.f32(odo)
    info_in = np.zeros((ecap, 36), np.float32)
    info_in[:7] = 100.0 * np.eye(6, dtype=np.float32).reshape(36)
    info_in[3] = np.eye(6, dtype=np.float32).reshape(36)
    cand_info = np.stack([1e4 * np.eye(6).reshape(36), 1e6 * np.eye(6).reshape(36)]).astype(np.float32)
    common = dict(pairs=[(0, 7), (0, 7)], model_fwd=L.f32([true_m, false_m]), status_fwd=[0, 0], model_bwd=L.f32([P.iso_inv(true_m), P.iso_inv(other)]),
                  status_bwd=[0, 0], info=cand_info, edge_capacity=ecap, edges=edges, meas=meas, info_out=info_in, edge_weight=np.ones(ecap, np.float32),
                  edge_count=7)
    kept = V.loop_verify_edges_host(max_cycle_trans=0.05, max_cycle_rot=0.05, **common)
    assert list(kept["verdict"]) == [V.LOOP_ACCEPTED, V.LOOP_CYCLE_TRANS] and kept["edge_count"] == 8
    forced = V.loop_verify_edges_host(**common)  # every test off: both become edges
    assert list(forced["verdict"]) == [V.LOOP_ACCEPTED, V.LOOP_ACCEPTED] and forced["edge_count"] == 9
    solve = lambda lst: V.pose_graph_optimize_host(start, lst["edges"], lst["meas"], lst["info"], lst["edge_weight"], iters=16, cg_iters=64,  # noqa: E731
                                                   edge_count=lst["edge_count"])["poses"]
    a0, a_kept, a_forced = ate(start), ate(solve(kept)), ate(solve(forced))
    print(f"ATE drifted {a0:.4f} m, with the accepted list {a_kept:.4f} m, with the false edge forced in {a_forced:.4f} m")
    assert a_kept < 0.5 * a0 and a_forced > 2.0 * a_kept


# ---- refusals: nothing is written
def ptr(a, shift=0):
    """a's address (shifted by some bytes: off its alignment), None for None"""
    return None if a is None else C.c_void_p(a.ctypes.data + shift)


NAN = float("nan")


def test_every_refusal_of_the_signatures_leaves_the_outputs_untouched():
    lib = V.lib()
    plane, sig, meta = np.zeros((64, 64), np.uint8), np.full(2048, 77, np.int8), np.full(4, 77, np.int32)

    def call(rows=64, cols=64, tr=8, tc=8, g=ptr(plane), s=ptr(sig), m=ptr(meta)):
        return lib.vors_loop_signatures_host(g, rows, cols, tr, tc, s, m)

    for kw in (dict(g=None), dict(s=None), dict(m=None), dict(tc=7), dict(tr=4, tc=8), dict(tr=64, tc=32), dict(tr=0, tc=64), dict(tr=64, tc=0),
               dict(tr=-8, tc=-8), dict(rows=4), dict(cols=4), dict(rows=70000), dict(cols=70000), dict(rows=20000, cols=20000),
               dict(s=ptr(sig, 1)), dict(s=ptr(sig, 4)), dict(m=ptr(meta, 1)), dict(m=ptr(meta, 2))):
        assert call(**kw) == INVALID, kw
    assert (sig == 77).all() and (meta == 77).all()
    assert call() == 0 and (sig[:64] == -128).all() and (sig[64:] == 77).all() and tuple(meta) == (-128 * 64, 128 * 128 * 64, 77, 77)
    with pytest.raises(V.VorsError):
        V.loop_signatures_host(plane, 8, 7)


def test_every_refusal_of_the_candidates_leaves_the_outputs_untouched():
    lib = V.lib()
    s = L.random_signatures(8, 64, seed=1)
    s16 = np.zeros(8 * 64 + 16, np.int8)  # (a copy at a 16-byte aligned address, whatever numpy gave s)
    base = (-s16.ctypes.data) % 16
    s16[base:base + 512] = s.reshape(-1)
    sp = C.c_void_p(s16.ctypes.data + base)
    m, poses = L.meta_of(s), L.line_poses(8)
    cand, cc, counts = np.full((8, 4, 2), 77, np.uint32), np.full(8, 77, np.uint32), np.full(6, 77, np.uint32)

    def call(sig_=sp, meta_=ptr(m), cap=8, d=64, poses_=ptr(poses), gap=1, k=4, dist=0.0, qdot=0.0, cand_=ptr(cand), cc_=ptr(cc), counts_=ptr(counts)):
        return lib.vors_loop_candidates_host(sig_, meta_, 8, cap, d, poses_, 0, gap, k, 0.0, dist, qdot, cand_, cc_, counts_)

    for kw in (dict(sig_=None), dict(meta_=None), dict(cand_=None), dict(cc_=None), dict(cap=0), dict(cap=-1), dict(cap=(1 << 20) + 1), dict(d=0),
               dict(d=32), dict(d=96), dict(d=1088), dict(d=2048), dict(gap=0), dict(k=0), dict(k=-1), dict(k=9), dict(dist=-1.0), dict(dist=NAN),
               dict(qdot=-0.5), dict(qdot=NAN), dict(sig_=C.c_void_p(sp.value + 4)), dict(sig_=C.c_void_p(sp.value + 1)), dict(meta_=ptr(m, 2)),
               dict(poses_=ptr(poses, 1)), dict(cand_=ptr(cand, 2)), dict(cc_=ptr(cc, 1)), dict(counts_=ptr(counts, 2))):
        assert call(**kw) == INVALID, kw
    assert (cand == 77).all() and (cc == 77).all() and (counts == 77).all()
    assert call() == 0 and counts[0] == 28 and counts[5] == 77 and cc[0] == 0
    with pytest.raises(V.VorsError):
        V.loop_candidates_host(s, m, 0, 4, 0.0)


def test_every_refusal_of_the_verification_leaves_the_outputs_untouched():
    lib = V.lib()
    case, _ = L.verify_cases(6, seed=8)
    edges, meas, info_out, weights = np.full((4, 2), 77, np.uint32), np.full((4, 7), 7.5, np.float32), np.full((4, 36), 7.5, np.float32), np.full(4, 7.5, np.float32)
    count, verdict, res, counts = np.array([1, 77], np.uint32), np.full(6, 77, np.uint32), np.full((6, 12), 7.5, np.float32), np.full(10, 77, np.uint32)
    given = dict(m=6, pairs=ptr(case["pairs"]), fwd=ptr(case["model_fwd"]), fstride=0, bwd=ptr(case["model_bwd"]), bstride=0, sf=ptr(case["status_fwd"]),
                 sb=ptr(case["status_bwd"]), info=ptr(case["info"]), poses=ptr(case["poses"]), pstride=0, nodes=16, b0=0.01, b1=0.01, b2=0.01, b3=0.01,
                 weight=1.0, edges=ptr(edges), meas=ptr(meas), info_out=ptr(info_out), weights=ptr(weights), count=ptr(count), ecap=4,
                 verdict=ptr(verdict), res=ptr(res), counts=ptr(counts))

    def call(**kw):
        a = dict(given)
        a.update(kw)
        return lib.vors_loop_verify_edges_host(*a.values())

    refused = [dict(m=0), dict(m=(1 << 28) + 1), dict(ecap=0), dict(ecap=-1), dict(ecap=(1 << 28) + 1), dict(weight=0.0), dict(weight=-1.0),
               dict(weight=NAN), dict(weight=float("inf"))]
    refused += [{name: None} for name in ("pairs", "fwd", "sf", "edges", "meas", "count", "verdict")]
    refused += [{name: bad} for name in ("fstride", "bstride", "pstride") for bad in (24, 30, 1 << 31)]
    refused += [{name: bad} for name in ("b0", "b1", "b2", "b3") for bad in (-0.1, NAN)]
    arrays = dict(pairs=case["pairs"], fwd=case["model_fwd"], bwd=case["model_bwd"], sf=case["status_fwd"], sb=case["status_bwd"], info=case["info"],
                  poses=case["poses"], edges=edges, meas=meas, info_out=info_out, weights=weights, count=count, verdict=verdict, res=res, counts=counts)
    refused += [{name: ptr(a, 2)} for name, a in arrays.items()]  # every pointer off its 4 bytes
    for kw in refused:
        assert call(**kw) == INVALID, kw
    assert (edges == 77).all() and (meas == 7.5).all() and (info_out == 7.5).all() and (weights == 7.5).all() and tuple(count) == (1, 77)
    assert (verdict == 77).all() and (res == 7.5).all() and (counts == 77).all()
    assert call() == 0 and count[0] > 1 and count[1] == 77 and counts[:9].sum() == 6 and counts[9] == 77
    with pytest.raises(V.VorsError):
        V.loop_verify_edges_host(weight=-1.0, edge_capacity=4, **case)


def test_the_host_twins_run_clean_under_the_sanitizers():
    """loop_closure_host_check: a stand-alone program (its own main) of the three host twins, built with ASan and UBSan on the host side."""
    subprocess.check_call(["make", "-C", CSRC, "-s", "loop_closure_host_check"])
    out = subprocess.run([os.path.join(CSRC, "loop_closure_host_check")], capture_output=True, text=True)
    assert out.returncode == 0 and "loop_closure_host_check: ok" in out.stdout, out.stdout + out.stderr
