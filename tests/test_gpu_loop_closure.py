"""Loop closure on the device (vors_loop_signatures, vors_loop_candidates, vors_loop_verify_edges): equal to the host twins bit for bit —
signatures, scores, lists, counts, verdicts, residuals and the appended edge lists. The twins themselves are held against numpy
restatements in tests/test_loop_closure_host.py. Nothing here has a tolerance."""
import numpy as np
import pytest

import loop_closure_cases as L
import vors_amd as V

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 31, 32, 33, 63, 64, 65, 200]  # straddle the 32-wide tiles and the 64-wide pairs of them


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cand_bits(out):
    """the device's [n, capacity, k, 2] int32 records as uint32"""
    return out["cand"].cpu().numpy().view(np.uint32)


# ---- signatures
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("rows,cols,tr,tc", L.SHAPES)
def test_signatures_equal_the_host_twin(rows, cols, tr, tc, n):
    import torch
    planes = np.stack((L.planes(rows, cols, seed=n) * 2)[:n])
    out = V.loop_signatures(dev(planes), tr, tc)
    torch.cuda.synchronize()
    sig, meta = out["sig"].cpu().numpy(), out["meta"].cpu().numpy()
    for p in range(n):
        want, total, sumsq = V.loop_signatures_host(planes[p], tr, tc)
        assert (sig[p] == want).all() and meta[p, 0] == total and meta[p, 1] == sumsq


def test_signatures_into_a_window_of_a_larger_array_and_from_an_odd_address():
    import torch
    rows, cols, tr, tc = 61, 83, 12, 16
    planes = np.stack(L.planes(rows, cols, seed=3)[1:])  # 3 planes of 5063 bytes: the second and third start off every alignment
    sig = torch.full((8, tr * tc), 77, dtype=torch.int8, device="cuda")
    meta = torch.full((8, 2), 77, dtype=torch.int32, device="cuda")
    V.loop_signatures(dev(planes), tr, tc, sig=sig, meta=meta, at=4)
    torch.cuda.synchronize()
    s, m = sig.cpu().numpy(), meta.cpu().numpy()
    assert (s[:4] == 77).all() and (s[7] == 77).all() and (m[:4] == 77).all() and (m[7] == 77).all()
    for p in range(3):
        want, total, sumsq = V.loop_signatures_host(planes[p], tr, tc)
        assert (s[4 + p] == want).all() and tuple(m[4 + p]) == (total, sumsq)


# ---- candidates
def assert_sets_equal_twin(sigs, counts, min_gap, k, min_score, poses=None, max_dist_m=0.0, min_qdot=0.0, query_first=None, width=7):
    """sigs [n, capacity, D] -> one device call over the n sets against n calls of the twin"""
    import torch
    n, cap, _ = sigs.shape
    meta = L.meta_of(sigs)
    dposes = None
    if poses is not None:
        wide = np.full((n, cap, width), 9.0, np.float32)
        wide[:, :, :7] = poses
        dposes = dev(wide)
    out = V.loop_candidates(dev(sigs), dev(meta), dev(np.array(counts, np.int32)), min_gap, k, min_score, poses=dposes, max_dist_m=max_dist_m,
                            min_qdot=min_qdot, query_first=None if query_first is None else dev(np.array(query_first, np.int32)))
    torch.cuda.synchronize()
    got, got_cc, got_counts = cand_bits(out), out["cand_counts"].cpu().numpy(), out["counts"].cpu().numpy()
    for g in range(n):
        twin = V.loop_candidates_host(sigs[g], meta[g], min_gap, k, min_score, poses=None if poses is None else poses[g], max_dist_m=max_dist_m,
                                      min_qdot=min_qdot, query_first=0 if query_first is None else query_first[g], count=counts[g])
        assert (got[g, :, :, 0] == twin["cand"]["i"]).all(), (g, counts[g])
        assert (got[g, :, :, 1] == bits(twin["cand"]["score"])).all(), (g, counts[g])
        assert (got_cc[g] == twin["cand_counts"]).all() and (got_counts[g].view(np.uint32) == twin["counts"]).all(), (g, counts[g])
    return out


@pytest.mark.parametrize("d", [64, 192, 1024])
def test_candidates_equal_the_host_twin_at_every_count(d):
    """nine sets of different counts under one capacity, random signatures; then a count above the capacity"""
    sigs = np.stack([L.random_signatures(200, d, seed=100 + c) for c in COUNTS])
    assert_sets_equal_twin(sigs, COUNTS, 1, 4, -2.0)
    assert_sets_equal_twin(sigs, COUNTS, 1, 8, 0.02)
    assert_sets_equal_twin(sigs[:2], [1000, 200], 10, 1, 0.0)


@pytest.mark.parametrize("d", [64, 192, 1024])
def test_candidates_asymmetric_data_pins_the_row_and_column_map(d):
    sigs = L.asymmetric_signatures(200, d)[None]
    assert_sets_equal_twin(sigs, [200], 1, 8, -2.0)
    assert_sets_equal_twin(sigs, [65], 3, 4, 0.1)


def test_candidates_the_largest_dot_products_and_flat_sets():
    sigs = np.full((2, 70, 1024), -128, np.int8)
    sigs[1, :, 0] = np.arange(70) - 128  # one cell differs: not flat, dot products at the top of the range
    out = assert_sets_equal_twin(sigs, [70, 70], 1, 8, -2.0)
    counts = out["counts"].cpu().numpy()
    assert counts[0, 1] == counts[0, 0] == 70 * 69 // 2 and counts[1, 4] > 0


def test_candidates_gates_windows_and_ties():
    special = L.special_signatures()[None]
    for k in (1, 4, 8):
        for gap in (1, 10):
            assert_sets_equal_twin(special, [24], gap, k, -2.0)
            assert_sets_equal_twin(special, [24], gap, k, -0.5)
    sigs = np.stack([L.random_signatures(80, 64, seed=s) for s in (1, 2, 3)])
    poses = np.stack([L.line_poses(80, 0.1)] * 3)
    poses[:, ::3, 3:] = np.float32([0.0, np.sin(0.6), 0.0, np.cos(0.6)])
    poses[1, 20, 1], poses[1, 41, 5], poses[2, 7, 6] = np.nan, np.inf, -np.inf
    for dist, qdot in ((0.0, 0.0), (3.35, 0.0), (0.0, 0.9), (3.35, 0.9)):
        assert_sets_equal_twin(sigs, [80, 64, 33], 2, 4, -2.0, poses, dist, qdot)
        assert_sets_equal_twin(sigs, [80, 64, 33], 2, 4, 0.05, poses, dist, qdot, query_first=[70, 0, 40], width=9)


# ---- verification
@pytest.mark.parametrize("m", [1, 1023, 1025, 3000])
def test_verify_equals_the_host_twin(m):
    import torch
    case, kind = L.verify_cases(m, seed=m)
    good = int((kind == 0).sum())
    for ecap, start in ((good + 5, 3), (max(good // 2, 1), 0)):  # room for all; an overflow
        edges = np.full((ecap, 2), 77, np.uint32)
        meas, info, weight = np.full((ecap, 7), 7.5, np.float32), np.full((ecap, 36), 7.5, np.float32), np.full(ecap, 7.5, np.float32)
        twin = V.loop_verify_edges_host(edge_capacity=ecap, edges=edges, meas=meas, info_out=info, edge_weight=weight, edge_count=start, weight=0.5,
                                        **case, **L.VERIFY_BOUNDS)
        d_edges, d_meas, d_info, d_weight = dev(edges.view(np.int32)), dev(meas), dev(info), dev(weight)
        d_count = dev(np.array([start], np.int32))
        wide = np.full((m, 9), 3.0, np.float32)  # the backward models in records of 9 floats
        wide[:, :7] = case["model_bwd"]
        out = V.loop_verify_edges(dev(case["pairs"].view(np.int32)), dev(case["model_fwd"]), dev(case["status_fwd"]), d_edges, d_meas, d_count,
                                  model_bwd=dev(wide), status_bwd=dev(case["status_bwd"]), info=dev(case["info"]), poses=dev(case["poses"]),
                                  weight=0.5, info_out=d_info, edge_weight=d_weight, **L.VERIFY_BOUNDS)
        torch.cuda.synchronize()
        assert (out["verdict"].cpu().numpy().view(np.uint32) == twin["verdict"]).all()
        assert (bits(out["residuals"].cpu().numpy()) == bits(twin["residuals"])).all()
        assert (out["counts"].cpu().numpy().view(np.uint32) == twin["counts"]).all()
        assert int(d_count.cpu()[0]) == twin["edge_count"] == min(start + good, ecap)
        assert (d_edges.cpu().numpy().view(np.uint32) == twin["edges"]).all() and (bits(d_meas.cpu().numpy()) == bits(twin["meas"])).all()
        assert (bits(d_info.cpu().numpy()) == bits(twin["info"])).all() and (bits(d_weight.cpu().numpy()) == bits(twin["edge_weight"])).all()
        if ecap < good:
            assert (twin["verdict"] == V.LOOP_CAPACITY).sum() == good - ecap


def test_verify_without_the_optional_inputs_and_refusals_enqueue_nothing():
    import torch
    case, kind = L.verify_cases(50, seed=11)
    twin = V.loop_verify_edges_host(case["pairs"], case["model_fwd"], case["status_fwd"], 64)
    edges, meas, info = dev(np.full((64, 2), -1, np.int32)), dev(np.full((64, 7), np.nan, np.float32)), dev(np.full((64, 36), np.nan, np.float32))
    count = dev(np.zeros(1, np.int32))
    out = V.loop_verify_edges(dev(case["pairs"].view(np.int32)), dev(case["model_fwd"]), dev(case["status_fwd"]), edges, meas, count, info_out=info)
    torch.cuda.synchronize()
    assert (out["verdict"].cpu().numpy().view(np.uint32) == twin["verdict"]).all() and int(count.cpu()[0]) == twin["edge_count"]
    assert (bits(info.cpu().numpy()) == bits(twin["info"])).all() and (bits(meas.cpu().numpy()) == bits(twin["meas"])).all()
    assert np.isnan(out["residuals"].cpu().numpy()[twin["verdict"] == V.LOOP_ACCEPTED]).all()
    before = (edges.clone(), meas.clone(), count.clone())
    for kw in (dict(weight=0.0), dict(max_cycle_trans=-1.0), dict(max_prior_rot=float("nan"))):
        with pytest.raises(V.VorsError):
            V.loop_verify_edges(dev(case["pairs"].view(np.int32)), dev(case["model_fwd"]), dev(case["status_fwd"]), edges, meas, count, **kw)
    sig = dev(L.random_signatures(8, 64, seed=1)[None])
    meta = dev(L.meta_of(L.random_signatures(8, 64, seed=1))[None])
    for kw in (dict(min_gap=0, k=4), dict(min_gap=1, k=9), dict(min_gap=1, k=4, max_dist_m=-1.0)):
        with pytest.raises(V.VorsError):
            V.loop_candidates(sig, meta, dev(np.array([8], np.int32)), min_score=0.0, **kw)
    with pytest.raises(V.VorsError):
        V.loop_signatures(dev(np.zeros((1, 64, 64), np.uint8)), 8, 7)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, (edges, meas, count)))  # (bits: NaN rows)


def test_every_refusal_of_the_device_entries_enqueues_nothing():
    """the refusals of include/vors_hip.h 2h on the device entries, the device-only ones (n < 1, a NULL count array, a bad pose stride)
    included, through the C entries themselves: VORS_ERR_INVALID_ARGUMENT, and afterwards every output holds its bits"""
    import ctypes as C
    import torch
    lib, invalid, nan = V.lib(), -1, float("nan")
    dp = lambda t, shift=0: C.c_void_p(t.data_ptr() + shift)  # noqa: E731
    fill = lambda shape, dtype: torch.full(shape, 77, dtype=dtype, device="cuda")  # noqa: E731

    def refuse(entry, given, refused, outputs):
        before = [t.clone() for t in outputs]
        for kw in refused:
            a = dict(given)
            a.update(kw)
            assert entry(*a.values()) == invalid, kw
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(before, outputs))
        assert entry(*given.values()) == 0  # ... and the call they were cut from is a good one
        torch.cuda.synchronize()
        assert not all(torch.equal(x, y) for x, y in zip(before, outputs))

    # signatures
    gray, sig, meta = dev(np.zeros((2, 64, 64), np.uint8)), fill((4, 64), torch.int8), fill((4, 2), torch.int32)
    given = dict(n=2, gray=dp(gray), rows=64, cols=64, tr=8, tc=8, sig=dp(sig), meta=dp(meta), stream=None)
    refuse(lib.vors_loop_signatures, given,
           [dict(n=0), dict(n=-1), dict(gray=None), dict(sig=None), dict(meta=None), dict(tc=7), dict(tr=64, tc=32), dict(tr=0, tc=64), dict(rows=4),
            dict(cols=4), dict(rows=70000), dict(cols=70000), dict(rows=20000, cols=20000), dict(sig=dp(sig, 4)), dict(meta=dp(meta, 2))], [sig, meta])
    # candidates
    s = L.random_signatures(8, 64, seed=1)
    d_sig, d_meta, d_in, d_poses = dev(s), dev(L.meta_of(s)), dev(np.array([8], np.int32)), dev(L.line_poses(8))
    cand, cc, counts = fill((8, 4, 2), torch.int32), fill((8,), torch.int32), fill((5,), torch.int32)
    given = dict(n=1, sig=dp(d_sig), meta=dp(d_meta), counts_in=dp(d_in), cap=8, d=64, poses=dp(d_poses), pstride=0, first=None, gap=1, k=4,
                 min_score=0.0, dist=0.0, qdot=0.0, cand=dp(cand), cc=dp(cc), counts=dp(counts), stream=None)
    refuse(lib.vors_loop_candidates, given,
           [dict(n=0), dict(sig=None), dict(meta=None), dict(counts_in=None), dict(cand=None), dict(cc=None), dict(cap=0), dict(cap=(1 << 20) + 1),
            dict(d=32), dict(d=96), dict(d=2048), dict(gap=0), dict(k=0), dict(k=9), dict(dist=-1.0), dict(dist=nan), dict(qdot=-0.5), dict(qdot=nan),
            dict(pstride=24), dict(pstride=30), dict(pstride=1 << 31), dict(sig=dp(d_sig, 4)), dict(meta=dp(d_meta, 2)), dict(counts_in=dp(d_in, 2)),
            dict(poses=dp(d_poses, 2)), dict(first=dp(d_in, 2)), dict(cand=dp(cand, 2)), dict(cc=dp(cc, 2)), dict(counts=dp(counts, 2))],
           [cand, cc, counts])
    # verification
    case, _ = L.verify_cases(6, seed=8)
    d = {k: dev(v.view(np.int32) if v.dtype == np.uint32 else v) for k, v in case.items()}
    edges, meas, info_out, weights = fill((4, 2), torch.int32), fill((4, 7), torch.float32), fill((4, 36), torch.float32), fill((4,), torch.float32)
    count, verdict, res, tally = dev(np.array([1], np.int32)), fill((6,), torch.int32), fill((6, 12), torch.float32), fill((9,), torch.int32)
    given = dict(m=6, pairs=dp(d["pairs"]), fwd=dp(d["model_fwd"]), fstride=0, bwd=dp(d["model_bwd"]), bstride=0, sf=dp(d["status_fwd"]),
                 sb=dp(d["status_bwd"]), info=dp(d["info"]), poses=dp(d["poses"]), pstride=0, nodes=16, b0=0.01, b1=0.01, b2=0.01, b3=0.01, weight=1.0,
                 edges=dp(edges), meas=dp(meas), info_out=dp(info_out), weights=dp(weights), count=dp(count), ecap=4, verdict=dp(verdict), res=dp(res),
                 counts=dp(tally), stream=None)
    refused = [dict(m=0), dict(m=(1 << 28) + 1), dict(ecap=0), dict(ecap=(1 << 28) + 1), dict(weight=0.0), dict(weight=nan), dict(weight=float("inf"))]
    refused += [{name: None} for name in ("pairs", "fwd", "sf", "edges", "meas", "count", "verdict")]
    refused += [{name: bad} for name in ("fstride", "bstride", "pstride") for bad in (24, 30, 1 << 31)]
    refused += [{name: bad} for name in ("b0", "b1", "b2", "b3") for bad in (-0.1, nan)]
    tensors = dict(pairs=d["pairs"], fwd=d["model_fwd"], bwd=d["model_bwd"], sf=d["status_fwd"], sb=d["status_bwd"], info=d["info"], poses=d["poses"],
                   edges=edges, meas=meas, info_out=info_out, weights=weights, count=count, verdict=verdict, res=res, counts=tally)
    refused += [{name: dp(t, 2)} for name, t in tensors.items()]
    refuse(lib.vors_loop_verify_edges, given, refused, [edges, meas, info_out, weights, count, verdict, res, tally])


# ---- the chain
def test_the_chain_on_the_device_equals_the_chain_of_the_twins():
    """signatures -> candidates -> track_pairs both ways -> pose_information -> verify_edges -> pose_graph_optimize on 8 frames of the
    80 x 60, 3-level dense scene, through device tensors alone (an unused candidate slot becomes the pair (j, j), which the verification
    turns away as INDEX); against the host twins around the same, already tested, device tracking. Nothing about accuracy is asserted."""
    import torch
    rows, cols, levels, frames_n, k, gap = 60, 80, 3, 8, 2, 3
    intr = V.scaled_intrinsics(rows, cols)
    step = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001])
    gray, depth = V.synth_render_frames([500] * frames_n, list(range(frames_n)), [step * f for f in range(frames_n)], rows, cols, intr)
    cfg = V.Config(nb_levels=levels, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=V.CANDIDATES_DENSE,
                   arithmetic=V.ARITH_FUSED)
    m, odo = frames_n * k, frames_n - 1
    fwd_batch, bwd_batch = V.Batch(cfg, odo + m, rows, cols), V.Batch(cfg, m, rows, cols)
    width = V.PAIR_STATS_DTYPE.itemsize // 4
    bounds = dict(max_cycle_trans=0.05, max_cycle_rot=0.05, max_prior_trans=1.0, max_prior_rot=1.0)
    poses0 = np.zeros((frames_n, 7), np.float32)
    poses0[:, 6] = 1.0
    odo_i = torch.arange(odo, device="cuda")

    def track(ci_all, cj_all):
        """the odometry pairs and the candidates forward, the candidates backward -> models as [*, width] views, statuses, info36"""
        fi, fj = torch.cat([odo_i, ci_all]), torch.cat([odo_i + 1, cj_all])
        out = []
        for batch, a, b in ((fwd_batch, fi, fj), (bwd_batch, cj_all, ci_all)):
            n = a.shape[0]
            poses = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
            status = torch.zeros(n, dtype=torch.int32, device="cuda")
            stats = V.stats_tensor(n)
            batch.track_pairs(gray[a].contiguous(), depth[a].contiguous(), gray[b].contiguous(), poses, status, stats)
            info = batch.pose_information(0, stats)[0].reshape(n, 36).contiguous()
            out.append((stats.view(torch.float32).view(n, width), status, info))
        return out

    # on the device
    sig = V.loop_signatures(gray, 8, 8)
    cands = V.loop_candidates(sig["sig"][None], sig["meta"][None], dev(np.array([frames_n], np.int32)), gap, k, -2.0, counts=False)
    cj = torch.arange(frames_n, device="cuda").repeat_interleave(k)
    ci = cands["cand_i"][0].reshape(-1).to(torch.int64)
    ci = torch.where(ci < 0, cj, ci)
    (f_model, f_status, f_info), (b_model, b_status, _) = track(ci, cj)
    ecap = odo + m
    edges = torch.zeros((ecap, 2), dtype=torch.int32, device="cuda")
    edges[:odo, 0], edges[:odo, 1] = odo_i.to(torch.int32), odo_i.to(torch.int32) + 1
    meas = torch.zeros((ecap, 7), dtype=torch.float32, device="cuda")
    meas[:odo] = f_model[:odo, :7]
    info = torch.zeros((ecap, 36), dtype=torch.float32, device="cuda")
    info[:odo] = f_info[:odo]
    weight = torch.ones(ecap, dtype=torch.float32, device="cuda")
    count = dev(np.array([odo], np.int32))
    pairs = torch.stack([ci, cj], dim=1).to(torch.int32).contiguous()
    ver = V.loop_verify_edges(pairs, f_model[odo:], f_status[odo:].contiguous(), edges, meas, count, model_bwd=b_model, status_bwd=b_status,
                              info=f_info[odo:].contiguous(), poses=dev(poses0), weight=0.5, info_out=info, edge_weight=weight, **bounds)
    graph = V.pose_graph_optimize(dev(poses0[None]), dev(np.array([frames_n], np.int32)), edges[None], count, meas[None], info=info[None],
                                  edge_weight=weight[None], iters=4, cg_iters=16)
    torch.cuda.synchronize()
    # the twins around the same tracking
    gh = gray.cpu().numpy()
    hs = [V.loop_signatures_host(gh[f], 8, 8) for f in range(frames_n)]
    hsig, hmeta = np.stack([s[0] for s in hs]), np.array([[s[1], s[2]] for s in hs], np.int32)
    assert (sig["sig"].cpu().numpy() == hsig).all() and (sig["meta"].cpu().numpy() == hmeta).all()
    hc = V.loop_candidates_host(hsig, hmeta, gap, k, -2.0)
    assert (cand_bits(cands)[0, :, :, 0] == hc["cand"]["i"]).all() and (cand_bits(cands)[0, :, :, 1] == bits(hc["cand"]["score"])).all()
    hj = np.repeat(np.arange(frames_n), k)
    hi = hc["cand"]["i"].reshape(-1).astype(np.int64)
    hi = np.where(hi == L.EMPTY, hj, hi)
    (tf_model, tf_status, tf_info), (tb_model, tb_status, _) = track(dev(hi), dev(hj))
    torch.cuda.synchronize()
    tfm, tbm = tf_model.cpu().numpy()[:, :7], tb_model.cpu().numpy()[:, :7]
    assert (bits(tfm) == bits(f_model.cpu().numpy()[:, :7])).all()  # the tracking is a function of its inputs
    h_edges, h_meas = np.zeros((ecap, 2), np.uint32), np.zeros((ecap, 7), np.float32)
    h_edges[:odo] = [(f, f + 1) for f in range(odo)]
    h_meas[:odo] = tfm[:odo]
    h_info = np.zeros((ecap, 36), np.float32)
    h_info[:odo] = tf_info.cpu().numpy()[:odo]
    hv = V.loop_verify_edges_host(np.stack([hi, hj], axis=1), tfm[odo:], tf_status.cpu().numpy()[odo:], ecap, model_bwd=tbm,
                                  status_bwd=tb_status.cpu().numpy(), info=tf_info.cpu().numpy()[odo:], poses=poses0, weight=0.5, edges=h_edges,
                                  meas=h_meas, info_out=h_info, edge_weight=np.ones(ecap, np.float32), edge_count=odo, **bounds)
    assert (ver["verdict"].cpu().numpy().view(np.uint32) == hv["verdict"]).all() and int(count.cpu()[0]) == hv["edge_count"]
    assert (bits(ver["residuals"].cpu().numpy()) == bits(hv["residuals"])).all()
    assert (hv["verdict"][hi == hj] == V.LOOP_INDEX).all()
    assert (edges.cpu().numpy().view(np.uint32) == hv["edges"]).all() and (bits(meas.cpu().numpy()) == bits(hv["meas"])).all()
    assert (bits(info.cpu().numpy()) == bits(hv["info"])).all() and (bits(weight.cpu().numpy()) == bits(hv["edge_weight"])).all()
    hg = V.pose_graph_optimize_host(poses0, hv["edges"], hv["meas"], hv["info"], hv["edge_weight"], iters=4, cg_iters=16, edge_count=hv["edge_count"])
    assert (bits(graph["poses"][0].cpu().numpy()) == bits(hg["poses"])).all()
    print(f"verdicts {hv['verdict'].tolist()}, {hv['edge_count']} edges, status {V.decode_pose_graph_stats(graph['stats'])[0]['status']}")
