"""inverse_depth.rs:24-29 and :37-42 for arrays on the host (vors_from_depth, vors_to_depth): needs no GPU.

to_depth is `(scale / x).round() as u16`: one IEEE float32 division, f32::round (halves AWAY from zero), and Rust's saturating cast
(NaN -> 0, <= 0 -> 0, >= 65535 -> 65535). The Python statement below makes the same division in float32 and rounds by rule:
  q in [1, 2^23):  floor(q + 0.5f) in float32 — q + 0.5 is exact there (the spacing of q is at most 0.5), so this IS round-half-away;
  q in [0, 1):     1 if q >= 0.5 else 0 (q + 0.5 would round up to 1.0 for the float just below 0.5);
  q >= 2^23, inf:  q itself (every such float is an integer);
  q < 0, NaN:      the cast gives 0 whatever the rounding does.
Equality with the library must be exact."""
import numpy as np

import vors_amd as V

SCALE = 5000.0


def restated(scale, x):
    x = np.asarray(x, np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = np.float32(scale) / x
        r = np.where(q < np.float32(1.0), np.where(q >= np.float32(0.5), np.float32(1.0), np.float32(0.0)),
                     np.where(q < np.float32(2.0 ** 23), np.floor(q + np.float32(0.5)), q)).astype(np.float32)
        out = np.zeros(x.shape, np.uint16)                      # NaN (every comparison False), zero, negative
        big = r >= np.float32(65535.0)
        mid = (r > 0) & ~big
        out[big] = 65535
        out[mid] = r[mid].astype(np.uint16)
    return out


def check(scale, x):
    x = np.asarray(x, np.float32)
    got = V.to_depth(scale, x)
    assert got.dtype == np.uint16 and got.shape == x.shape
    want = restated(scale, x)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (scale, x[bad[:5]], got[bad[:5]], want[bad[:5]])


def test_random_inverse_depths():
    rng = np.random.default_rng(7)
    check(SCALE, rng.uniform(0.05, 50.0, 10000).astype(np.float32))
    check(SCALE, np.exp(rng.uniform(np.log(0.05), np.log(50.0), 10000)).astype(np.float32))


def test_every_exact_half_integer_quotient():
    # at scale 5000 the quotient 5000 / x is exactly k + 0.5 only for x = 10000 / (2k + 1) with 2k + 1 an odd divisor of 10000
    x = np.array([10000.0 / d for d in (1, 5, 25, 125, 625)], np.float32)
    assert (np.float32(SCALE) / x == np.array([0.5, 2.5, 12.5, 62.5, 312.5], np.float32)).all()
    assert (V.to_depth(SCALE, x) == np.array([1, 3, 13, 63, 313], np.uint16)).all()   # away from zero, not to even
    check(SCALE, x)
    check(SCALE, -x)
    # every k + 0.5 up to the saturation, built exactly: scale = k + 0.5 over x = 1 (and over -1: nothing negative survives the cast)
    one, minus = np.ones(1, np.float32), -np.ones(1, np.float32)
    for k in range(0, 65538):
        got = int(V.to_depth(k + 0.5, one)[0])
        assert got == min(k + 1, 65535), k
        if k % 997 == 0:
            assert int(V.to_depth(k + 0.5, minus)[0]) == 0, k
    # the same quotients through a power-of-two inverse depth
    for k in (0, 1, 2, 3, 254, 255, 4094, 4095, 32767, 65534, 65535, 65536):
        assert int(V.to_depth((k + 0.5) / 4.0, np.array([0.25], np.float32))[0]) == min(k + 1, 65535), k


def test_special_values_and_saturation():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    x = np.array([0.0, -0.0, -1.0, -1e-30, -1e30, nan, -nan, inf, -inf, 1e-38, 1e-45, 3e38, 1e30], np.float32)
    got = V.to_depth(SCALE, x)
    #                      0 -> +inf  -0 -> -inf                          NaN    inf -> 0   -inf  overflow -> inf   q tiny
    assert got.tolist() == [65535, 0, 0, 0, 0, 0, 0, 0, 0, 65535, 65535, 0, 0]
    check(SCALE, x)
    # quotients around the saturation: 65534.5 rounds up to 65535; everything from 65535.5 on would not fit and saturates
    x0 = np.float32(SCALE / 65535.5)
    near = [x0]
    for _ in range(200):
        near.append(np.nextafter(near[-1], np.float32(0)))
    lo = x0
    for _ in range(200):
        lo = np.nextafter(lo, np.float32(1))
        near.append(lo)
    near = np.array(near, np.float32)
    q = np.float32(SCALE) / near
    assert (q >= 65535.5).any() and (q < 65534.5).any()
    check(SCALE, near)
    assert (V.to_depth(SCALE, near[q >= 65534.5]) == 65535).all()
    check(SCALE, np.array([SCALE / 65535.5, SCALE / 65536.0, SCALE / 70000.0, SCALE / 1e6, SCALE / 1e9, SCALE / 2.0 ** 23, SCALE / 2.0 ** 24], np.float32))
    check(65535.5, np.ones(1, np.float32))
    check(65536.0, np.ones(1, np.float32))
    check(1e30, np.ones(1, np.float32))
    # below one: 0.5 rounds up, the float just below it rounds down (floor(q + 0.5) alone would get this one wrong)
    below_half = np.nextafter(np.float32(0.5), np.float32(0))
    assert V.to_depth(0.5, np.ones(1, np.float32))[0] == 1 and V.to_depth(float(below_half), np.ones(1, np.float32))[0] == 0
    assert V.to_depth(SCALE, np.empty(0, np.float32)).shape == (0,)


def test_from_depth_and_the_round_trip():
    d = np.arange(0, 65536, dtype=np.uint16)
    f = V.from_depth(SCALE, d)
    assert f.dtype == np.float32 and np.isnan(f[0]) and np.isfinite(f[1:]).all()           # 0 is Unknown
    assert (f[1:].view(np.uint32) == (np.float32(SCALE) / d[1:].astype(np.float32)).view(np.uint32)).all()
    back = V.to_depth(SCALE, f)
    assert back[0] == 0                                                                      # Unknown is encoded with 0
    assert (back[1:] == d[1:]).all()
    again = V.from_depth(SCALE, back)
    assert (again[1:].view(np.uint32) == f[1:].view(np.uint32)).all() and np.isnan(again[0])
    img = d[:60000].reshape(200, 300)
    assert V.from_depth(SCALE, img).shape == (200, 300) and V.to_depth(SCALE, V.from_depth(SCALE, img)).shape == (200, 300)
