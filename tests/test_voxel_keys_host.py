"""The voxel key of the keyframe map's voxel filter on the host (vors_voxel_keys, lie.h voxel_key — the text the device kernels run), and
the argument plumbing of the filter that needs no device: the map_voxels pair of Tracker / Trackers.enable_map_voxels, the exported
symbols and the NULL-handle refusals.

The restatement below is the definition of include/vors_hip.h in numpy: per axis q = floor(w / voxel_m) in float32 (numpy's float32
division and floor are IEEE and exact), a key iff every q is finite and -2^20 <= q < 2^20, then
(q_x + 2^20) | (q_y + 2^20) << 21 | (q_z + 2^20) << 42; all ones otherwise. Every comparison is on bits."""
import numpy as np
import pytest

import vors_amd as V

F32 = np.float32
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
NEW = ("vors_trackers_enable_map_voxels", "vors_trackers_map_voxels", "vors_tracker_enable_map_voxels", "vors_tracker_read_map_voxels",
       "vors_voxel_keys")


def keys_numpy(voxel_m, xyz):
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = np.floor(xyz / F32(voxel_m))
    assert q.dtype == F32
    ok = (np.isfinite(q) & (q >= F32(-2 ** 20)) & (q < F32(2 ** 20))).all(axis=1)
    qi = np.where(ok[:, None], q, 0).astype(np.int64) + 2 ** 20
    key = (qi[:, 0] | (qi[:, 1] << 21) | (qi[:, 2] << 42)).astype(np.uint64)
    return np.where(ok, key, NONE)


def below(x):
    return np.nextafter(F32(x), F32(-np.inf))


def above(x):
    return np.nextafter(F32(x), F32(np.inf))


def hard_values(v):
    """Coordinates that sit on the rule's edges for a voxel of edge v."""
    v = F32(v)
    out = [0.0, -0.0, 1.0, -1.0, 1.85, -2.97, 123.456, -123.456, 1e-30, -1e-30, 1e-45, -1e-45]
    for k in (1, 2, 3, 7, 50, 1000, -1, -2, -3, -7, -50, -1000):    # exact multiples of the edge, and their neighbours
        m = F32(k) * v
        out += [m, below(m), above(m)]
    lo, hi = F32(-2 ** 20) * v, F32(2 ** 20) * v                   # q = -2^20, 2^20 - 1 and 2^20
    out += [lo, below(lo), above(lo), hi, below(hi), above(hi), F32(2 ** 20 - 1) * v, below(F32(2 ** 20 - 1) * v), F32(2 ** 20 - 0.5) * v]
    out += [np.nan, np.inf, -np.inf, 3e38, -3e38]
    return np.array(out, F32)


@pytest.mark.parametrize("voxel_m", [0.02, 0.05, 0.25, 1.0, 3.0, 0.1])
def test_keys_equal_the_definition(voxel_m):
    h = hard_values(voxel_m)
    rng = np.random.default_rng(7)
    # every hard value on every axis, the other two axes ordinary or hard as well
    cols = [np.stack([h, rng.uniform(-3, 3, len(h)).astype(F32), rng.uniform(-3, 3, len(h)).astype(F32)], axis=1)]
    cols += [np.roll(cols[0], 1, axis=1), np.roll(cols[0], 2, axis=1)]
    cols.append(np.stack([h, np.roll(h, 5), np.roll(h, 11)], axis=1))
    cols.append(rng.uniform(-4, 4, (4000, 3)).astype(F32))
    xyz = np.concatenate(cols)
    got, want = V.voxel_keys(voxel_m, xyz), keys_numpy(voxel_m, xyz)
    assert got.dtype == np.uint64 and got.shape == (len(xyz),)
    assert got.tobytes() == want.tobytes()
    assert (got == NONE).any() and (got != NONE).any() and (got[got != NONE] < np.uint64(1 << 63)).all()


def test_the_named_cases():
    v = F32(0.25)   # a power of two: every product and quotient below is exact, so the expected keys can be written down
    one = lambda x, y=0.0, z=0.0: int(V.voxel_keys(v, np.array([[x, y, z]], F32))[0])
    B = 1 << 20
    origin = B | B << 21 | B << 42
    assert one(0.0) == origin and one(-0.0) == origin                 # -0.0 / v = -0.0, floor keeps it, and it converts to 0
    assert one(0.1) == origin and one(-0.1) == origin - 1             # negative coordinates: floor, not truncation
    assert one(0.0, -0.1, 0.0) == origin - (1 << 21) and one(0.0, 0.0, -0.1) == origin - (1 << 42)
    m = F32(7) * v                                                    # an exact multiple opens its voxel; the value below is the one before
    assert one(m) == origin + 7 and one(below(m)) == origin + 6 and one(above(m)) == origin + 7
    assert one(-m) == origin - 7 and one(below(-m)) == origin - 8 and one(above(-m)) == origin - 7
    lo, hi = F32(-B) * v, F32(B) * v
    assert one(lo) == origin - B and (one(lo) & 0x1FFFFF) == 0        # q = -2^20: the lowest field value
    assert one(below(lo)) == V.VOXEL_NONE                             # q = -2^20 - 1
    assert one(F32(B - 1) * v) == origin + B - 1                      # q = 2^20 - 1: the highest
    assert one(hi) == V.VOXEL_NONE                                    # q = 2^20
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            p = np.zeros((1, 3), F32)
            p[0, axis] = bad
            assert int(V.voxel_keys(v, p)[0]) == V.VOXEL_NONE
    tiny = F32(1e-30)                                                 # the quotient leaves the range (1e30) or overflows to inf
    assert int(V.voxel_keys(tiny, np.array([[1.0, 0.0, 0.0]], F32))[0]) == V.VOXEL_NONE
    assert int(V.voxel_keys(tiny, np.array([[3e38, 0.0, 0.0]], F32))[0]) == V.VOXEL_NONE
    assert int(V.voxel_keys(tiny, np.array([[0.0, -0.0, 0.0]], F32))[0]) == origin
    assert keys_numpy(tiny, [[1.0, 0.0, 0.0], [3e38, 0.0, 0.0], [0.0, -0.0, 0.0]]).tolist() == [V.VOXEL_NONE, V.VOXEL_NONE, origin]


def test_division_not_a_reciprocal():
    """Coordinates whose f32 quotient w / v and product w * (1 / v) floor differently must follow the quotient."""
    v = F32(0.02)
    r = F32(1) / v
    w = (np.arange(1, 200001, dtype=F32) * v).astype(F32)
    with np.errstate(all="ignore"):
        differ = np.floor(w / v) != np.floor(w * r)
    assert differ.any(), "no coordinate tells the division from the reciprocal"
    xyz = np.stack([w[differ], np.zeros(differ.sum(), F32), np.zeros(differ.sum(), F32)], axis=1)
    assert V.voxel_keys(v, xyz).tobytes() == keys_numpy(v, xyz).tobytes()


def test_shapes_and_unusable_edges():
    xyz = np.random.default_rng(3).uniform(-2, 2, (5, 7, 3)).astype(F32)
    k = V.voxel_keys(0.05, xyz)
    assert k.shape == (5, 7) and k.tobytes() == keys_numpy(0.05, xyz).tobytes()
    assert V.voxel_keys(0.05, xyz.astype(np.float64)).tobytes() == k.tobytes()
    assert V.voxel_keys(0.05, np.zeros((0, 3), F32)).shape == (0,)
    for bad in (0.0, -0.02, np.nan, np.inf):   # an edge no handle accepts gives no point a key
        assert (V.voxel_keys(bad, xyz) == NONE).all()
    with pytest.raises(V.VorsError, match="xyz"):
        V.voxel_keys(0.05, np.zeros((4, 2), F32))


def test_symbols_exported_and_null_handles_refused():
    lib = V.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in V.EXPORTED_SYMBOLS
    assert lib.vors_abi_version() == 5
    assert lib.vors_trackers_enable_map_voxels(None, 0.02, 65536) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_trackers_map_voxels(None, None, None) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_tracker_enable_map_voxels(None, 0.02, 65536) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_tracker_read_map_voxels(None, None, None) == -1 and b"NULL" in lib.vors_last_error()


def test_map_voxels_pair():
    f = V._map_voxels_args
    assert f(None) is None
    assert f((0.02, 65536)) == (0.02, 65536) and f([1, 64]) == (1.0, 64)
    t = f((np.float32(0.5), np.int64(128)))
    assert t == (0.5, 128) and type(t[0]) is float and type(t[1]) is int
    assert f((-1.0, 3)) == (-1.0, 3) and f((float("nan"), 0))[1] == 0   # values are judged by the library, once for every caller
    for bad in ((), (0.02,), (0.02, 64, 1), "ab", 5, object(), (0.02, 64.0), (0.02, None), (0.02, True), (True, 64), ("0.02", 64), (None, 64),
                (0.02, 2 ** 31)):
        with pytest.raises(V.VorsError, match="map_voxels"):
            f(bad)


def test_a_bad_pair_is_refused_before_any_handle_is_created():
    img, depth = np.zeros((60, 80), np.uint8), np.zeros((60, 80), np.uint16)
    for bad in ((0.02,), (0.02, 64.0), "ab"):
        with pytest.raises(V.VorsError, match="map_voxels"):
            V.Tracker(V.Config(nb_levels=3), 0.0, depth, 0.0, img, map=(0, 1000, 8), map_voxels=bad)
    with pytest.raises(V.VorsError, match="needs the keyframe map"):   # a good pair without the map it filters
        V.Tracker(V.Config(nb_levels=3), 0.0, depth, 0.0, img, map_voxels=(0.02, 65536))
