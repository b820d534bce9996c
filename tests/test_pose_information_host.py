"""Pose information on the host (vors_pose_information_from_sums) and the argument checks of the batched evaluation that need no GPU.

The 29 sums come from the oracle (oracle.Tracker on the CPU, oracle.lm_eval at the tracked model); the algebra — H mirrored, the residual
variance, sigma^2 H^-1 through a float64 Cholesky — is compared with numpy's float64 on the same H. The bound on the covariance scales with
the problem: 100 cond(H) 2^-52 max|Sigma| (what a backward-stable float64 inverse may lose) plus one f32 ulp (the final rounding)."""
import ctypes as C

import numpy as np
import pytest

import vors_amd as V
from oracle import oracle as O

ROWS, COLS, LEVELS = 120, 160, 4


def pack29(e_mean, n_inside, g, H):
    s = np.zeros(29, np.float32)
    s[0] = np.float32(e_mean) * np.float32(n_inside)  # the oracle returns energy_sum / n (lm_optimizer.rs:86)
    s[1] = n_inside
    s[2:8] = g
    s[8:29] = np.asarray(H, np.float32)[np.triu_indices(6)]
    return s


def mirrored(s):
    H = np.zeros((6, 6), np.float32)
    H[np.triu_indices(6)] = s[8:29]
    return H + np.triu(H, 1).T


def same_bits(a, b):
    return (np.asarray(a, np.float32).view(np.uint32) == np.asarray(b, np.float32).view(np.uint32)).all()


def cov_bound(H64, cov64):
    return 100.0 * np.linalg.cond(H64) * 2.0 ** -52 * np.abs(cov64).max() + np.spacing(np.abs(cov64).astype(np.float32))


def test_symbols_exported_and_null_handle_rejected():
    lib = V.lib()
    for name in ("vors_batch_eval_pairs", "vors_batch_pose_information", "vors_pose_information_from_sums"):
        assert hasattr(lib, name) and name in V.EXPORTED_SYMBOLS
    dummy = np.zeros(64, np.float32)
    p = dummy.ctypes.data_as(C.c_void_p)
    st = lib.vors_batch_eval_pairs(None, 1, 0, 1, p, 0, V.ARITH_EXACT, 0, p, None)
    assert st == -1 and b"b is NULL" in lib.vors_last_error()
    st = lib.vors_batch_pose_information(None, 1, 0, p, 0, p, p, p, p, None)
    assert st == -1 and b"b is NULL" in lib.vors_last_error()
    assert lib.vors_pose_information_from_sums(None, p, p, None, None) == -1 and b"sums29" in lib.vors_last_error()


@pytest.fixture(scope="module", params=[0, 1], ids=["coarse_to_fine", "dense"])
def tracked(request):
    mode = request.param
    intr = O.scaled_intrinsics(ROWS, COLS)
    kg, kd, cg, cd, gt = O.synth_pair(0x5EED9100, ROWS, COLS, intr)
    tr = O.Tracker(O.make_config(LEVELS, intr, candidates_mode=mode), 0.0, kd, 0.0, kg)
    tr.track(1.0, cd, 1.0, cg)
    last = tr.last()
    assert last["went_well"]
    xy, iz, jac = tr.points(0)
    _, _, _, k = tr.level(0)
    return dict(k=k, tmpl=tr.image(0), img=cg, xy=xy, iz=iz, jac=jac, model=last["lm_model"])


@pytest.mark.parametrize("huber", [0.0, 10.0], ids=["l2", "huber10"])
def test_covariance_algebra_against_numpy_float64(tracked, huber):
    t = tracked
    e, n, g, H = O.lm_eval(t["k"], t["tmpl"], t["img"], t["xy"], t["iz"], t["jac"], t["model"], huber_delta=huber)
    assert n > 100
    s = pack29(e, n, g, H)
    info, cov, sigma2, flags = V.pose_information_from_sums(s)
    assert flags == 0
    assert same_bits(info, mirrored(s))
    assert same_bits(sigma2, np.float32(np.float64(s[0]) / (np.float64(s[1]) - 6.0)))
    H64 = mirrored(s).astype(np.float64)
    ref = (np.float64(s[0]) / (np.float64(s[1]) - 6.0)) * np.linalg.inv(H64)
    err, bound = np.abs(cov.astype(np.float64) - ref), cov_bound(H64, ref)
    print(f"cond(H) = {np.linalg.cond(H64):.3e}, max |cov - ref| / bound = {(err / bound).max():.3e}")
    assert (err <= bound).all()
    assert same_bits(cov, cov.T)
    np.linalg.cholesky(cov.astype(np.float64))  # raises LinAlgError unless positive definite


def test_flags_too_few_points_and_rank_deficiency(tracked):
    t = tracked
    e, n, g, H = O.lm_eval(t["k"], t["tmpl"], t["img"], t["xy"], t["iz"], t["jac"], t["model"])
    s = pack29(e, n, g, H)
    few = s.copy()
    few[1] = 6
    info, cov, sigma2, flags = V.pose_information_from_sums(few)
    assert flags & 1 and np.isnan(cov).all() and np.isnan(sigma2) and same_bits(info, mirrored(few))
    seven = s.copy()
    seven[1] = 7
    assert V.pose_information_from_sums(seven)[3] == 0
    # rank 5: one twist direction carries no information (its row and column of H are zero)
    Hd = np.asarray(H, np.float32).copy()
    Hd[4, :] = 0
    Hd[:, 4] = 0
    sing = pack29(e, n, g, Hd)
    info, cov, sigma2, flags = V.pose_information_from_sums(sing)
    assert flags == 2 and np.isnan(cov).all() and np.isnan(sigma2) and same_bits(info, Hd)
