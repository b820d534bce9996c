"""The scale of a residual histogram on the host (vors_residual_scale_from_hist) and the argument checks of vors_batch_residual_maps that
need no GPU.

The formula of include/vors_hip.h restated in float64: n = sum of the bins, target = n / 2, b = the first bin whose cumulative count reaches
target, median_abs = b + (target - count below b) / hist[b], sigma_mad = 1.4826 median_abs, each rounded to f32 at the end; n = 0 -> NaN.
Every operation is one IEEE float64 operation on exactly representable counts, so the library must give the same BITS. Against numpy's median
of the samples themselves the only error is the bin width: |median_abs - median| < 1."""
import ctypes as C

import numpy as np
import pytest

import vors_amd as V

BINS = 256


def restated(hist):
    hist = [int(x) for x in hist]
    n = sum(hist)
    if n == 0:
        return np.float32(np.nan), np.float32(np.nan), 0
    target = np.float64(0.5) * np.float64(n)
    below = 0
    for b in range(BINS):
        if np.float64(below + hist[b]) >= target:
            break
        below += hist[b]
    med = np.float64(b) + (target - np.float64(below)) / np.float64(hist[b])
    return np.float32(med), np.float32(np.float64(1.4826) * med), n


def same_bits(a, b):
    return (np.asarray(a, np.float32).view(np.uint32) == np.asarray(b, np.float32).view(np.uint32)).all()


def single(bin_, count):
    h = np.zeros(BINS, np.uint32)
    h[bin_] = count
    return h


def cases():
    rng = np.random.default_rng(0xD15C)
    out = {}
    for k in range(8):   # random histograms: flat, and piled up in the lowest bins like real residuals
        out[f"flat{k}"] = rng.integers(0, 5000, BINS).astype(np.uint32)
        out[f"piled{k}"] = np.bincount(np.minimum(rng.exponential(3.0 + k, 20000 + k).astype(int), 255), minlength=BINS).astype(np.uint32)
        out[f"holes{k}"] = (rng.integers(0, 3000, BINS) * (rng.uniform(size=BINS) < 0.1)).astype(np.uint32)
    out["single_bin_17"] = single(17, 12345)
    out["single_point"] = single(40, 1)
    out["all_in_bin_0"] = single(0, 307200)
    out["all_in_bin_255"] = single(255, 307200)
    even = np.zeros(BINS, np.uint32)
    even[[3, 4, 9]] = (5, 5, 10)        # n = 20: the target 10 is reached exactly at the end of bin 4
    out["even_n"] = even
    odd = even.copy()
    odd[200] = 1                        # n = 21: target 10.5 falls inside bin 9
    out["odd_n"] = odd
    out["large_counts"] = np.full(BINS, 0xffffffff // 2, np.uint32)   # n beyond 2^32: the count is summed in 64 bits
    return out


CASES = cases()


def test_symbols_exported_and_null_arguments_rejected():
    lib = V.lib()
    for name in ("vors_batch_residual_maps", "vors_residual_scale_from_hist"):
        assert hasattr(lib, name) and name in V.EXPORTED_SYMBOLS
    dummy = np.zeros(64, np.float32)
    p = dummy.ctypes.data_as(C.c_void_p)
    st = lib.vors_batch_residual_maps(None, 1, 0, p, 0, p, p, p, p, None)
    assert st == -1 and b"b is NULL" in lib.vors_last_error()
    assert lib.vors_residual_scale_from_hist(None, None, None, None) == -1 and b"hist" in lib.vors_last_error()
    assert V.RESIDUAL_BINS == BINS


@pytest.mark.parametrize("name", list(CASES))
def test_scale_equals_the_float64_formula_bit_for_bit(name):
    hist = CASES[name]
    med, sig, n = V.residual_scale_from_hist(hist)
    rmed, rsig, rn = restated(hist)
    print(f"{name}: n = {n}, median_abs = {med!r} (restated {rmed!r}), sigma_mad = {sig!r} (restated {rsig!r})")
    assert n == rn % (1 << 32)   # (*n_inside is 32 bits wide; the scales use the full count)
    assert same_bits(med, rmed) and same_bits(sig, rsig)


def test_known_values():
    assert V.residual_scale_from_hist(CASES["even_n"])[0] == np.float32(5.0)        # 4 + (10 - 5) / 5
    assert V.residual_scale_from_hist(CASES["odd_n"])[0] == np.float32(9.05)        # 9 + (10.5 - 10) / 10
    assert V.residual_scale_from_hist(CASES["all_in_bin_0"])[0] == np.float32(0.5)
    assert V.residual_scale_from_hist(CASES["all_in_bin_255"])[0] == np.float32(255.5)
    assert V.residual_scale_from_hist(CASES["single_point"])[0] == np.float32(40.5)


def test_empty_histogram_gives_nan_with_status_ok():
    lib = V.lib()
    hist = np.zeros(BINS, np.uint32)
    med, sig, n = C.c_float(1.0), C.c_float(1.0), C.c_uint32(7)
    assert lib.vors_residual_scale_from_hist(hist.ctypes.data_as(C.c_void_p), C.byref(med), C.byref(sig), C.byref(n)) == 0
    assert np.isnan(med.value) and np.isnan(sig.value) and n.value == 0
    # every output is nullable
    assert lib.vors_residual_scale_from_hist(hist.ctypes.data_as(C.c_void_p), None, None, None) == 0
    assert lib.vors_residual_scale_from_hist(CASES["odd_n"].ctypes.data_as(C.c_void_p), None, C.byref(sig), None) == 0
    assert same_bits(sig.value, restated(CASES["odd_n"])[1])


def samples(dist, n, rng):
    r = {"exponential": lambda: rng.exponential(4.0, n), "half_normal": lambda: np.abs(rng.normal(0.0, 12.0, n)),
         "uniform": lambda: rng.uniform(0.0, 255.0, n),
         "two_clusters": lambda: np.where(rng.uniform(size=n) < 0.5, rng.uniform(2.0, 3.0, n), rng.uniform(100.0, 101.0, n))}[dist]()
    return np.minimum(r, 255.0) + rng.uniform(1e-6, 5e-4, n)   # integer-free samples of |r| in (0, 256)


# Why the bound is the bin width. The interpolated median lies in the bin b of the sample of rank ceil(n / 2). n odd: that sample IS
# numpy's median, both lie in (b, b + 1): the distance is below 1 whatever the distribution. n even: numpy's median is the mean of the
# samples of rank n / 2 and n / 2 + 1; with both in bin b the same holds, and with the upper one in bin b + 1 or b + 2 the interpolated
# median is b + 1 exactly and the mean lies in (b + 1/2, b + 2): still below 1. Only a gap of more than two EMPTY bins in the middle of the
# sample separates the two definitions of an even median (and then neither is "the" median), so the even cases draw 20000 samples from
# densities without a hole (the chance of a gap of two grey levels at the median is below exp(-100)); the clustered one runs at odd n.
@pytest.mark.parametrize("dist,n", [(d, n) for d in ("exponential", "half_normal", "uniform") for n in (1, 101, 20000, 20001)]
                         + [("two_clusters", n) for n in (1, 3, 101, 20001)])
def test_median_within_one_bin_of_the_sample_median(dist, n):
    r = samples(dist, n, np.random.default_rng(n * 31 + len(dist)))
    hist = np.bincount(np.minimum(r.astype(int), 255), minlength=BINS)
    med, sig, cnt = V.residual_scale_from_hist(hist)
    assert cnt == n
    print(f"{dist} n = {n}: median_abs = {med}, numpy median = {np.median(r)}")
    assert abs(float(med) - float(np.median(r))) < 1.0
