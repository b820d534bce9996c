"""The host twins of the voxel statistics (vors_voxel_stats_host, vors_voxel_means_host; no GPU): against a plain numpy restatement of
the definition (group by key, the f32 operations through np.float32, np.rint), on hand-made lists, and the refusals of every new entry
on a NULL handle or bad arguments. Comparisons are on bits."""
import ctypes as C

import numpy as np
import pytest

import vors_amd as V

NONE = np.uint64(V.VOXEL_NONE)
NAN_BITS = np.uint32(0x7FC00000)
F = np.float32


def numpy_stats(xyz, gray, segment_of, voxel_m, capacity):
    """The definition, restated: ranks in order of first occurrence of a key; q = rint(((w - f) / voxel_m) * 2^20) in f32."""
    keys = V.voxel_keys(voxel_m, xyz)
    uniq, first = np.unique(keys, return_index=True)
    first = np.sort(first[uniq != NONE])
    rank = {int(keys[i]): r for r, i in enumerate(first)}
    k = min(len(first), capacity)
    sums, obs = np.zeros((k, 4), np.int64), np.zeros((k, 2), np.uint32)
    vm = F(voxel_m)
    for i in range(len(xyz)):
        if keys[i] == NONE or rank[int(keys[i])] >= capacity:
            continue
        r = rank[int(keys[i])]
        f = xyz[first[r]]
        with np.errstate(all="ignore"):
            q = np.rint(((xyz[i].astype(F) - f.astype(F)).astype(F) / vm).astype(F) * F(1048576.0)).astype(np.int64)
        sums[r, :3] += q
        sums[r, 3] += int(gray[i])
        obs[r, 0] += 1
        obs[r, 1] = max(int(obs[r, 1]), int(segment_of[i]))
    return len(first), first[:k].astype(np.uint32), sums, obs


def numpy_means(xyz, sums, obs, voxel_m, min_count, min_span, first_segment):
    out, gray = np.zeros((len(xyz), 3), F), np.zeros(len(xyz), np.uint8)
    kept = 0
    for r in range(len(xyz)):
        count, last = int(obs[r, 0]), int(obs[r, 1])
        span = max(last - int(first_segment[r]), 0) if first_segment is not None else 0
        if count < max(min_count, 1) or span < min_span:
            out[r] = np.array([NAN_BITS] * 3, np.uint32).view(F)
            continue
        kept += 1
        for a in range(3):
            off = F(np.float64(sums[r, a]) / (np.float64(count) * 1048576.0))
            out[r, a] = F(xyz[r, a]) + F(F(voxel_m) * off)
        gray[r] = (2 * int(sums[r, 3]) + count) // (2 * count)
    return out, gray, kept


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("voxel_m, capacity", [(0.02, 10 ** 6), (0.1, 10 ** 6), (0.05, 37), (0.013, 1)])
def test_random_lists_against_numpy(voxel_m, capacity):
    rng = np.random.default_rng(7)
    n = 4000
    xyz = (rng.normal(size=(n, 3)) * 0.15 + np.array([0.3, -0.2, 2.4])).astype(F)
    xyz[rng.integers(0, n, 40)] = np.nan                       # no key
    xyz[rng.integers(0, n, 10), 1] = np.inf
    xyz[rng.integers(0, n, 10)] = F(1e9)                       # a quotient out of range
    gray = rng.integers(0, 256, n).astype(np.uint8)
    seg = np.sort(rng.integers(0, 9, n)).astype(np.uint32)
    got = V.voxel_stats_host(xyz, gray, voxel_m, capacity, seg)
    total, first, sums, obs = numpy_stats(xyz, gray, seg, voxel_m, capacity)
    assert got["total"] == total and same_bits(got["first_index"], first)
    assert same_bits(got["sums"], sums) and same_bits(got["obs"], obs)
    assert (obs[:, 0] >= 2).any() and (obs[:, 0] == 1).any() or capacity == 1
    k = len(first)
    fs = seg[first]
    for min_count, min_span, with_fs in ((1, 0, False), (2, 0, False), (1, 2, True), (3, 1, True), (0, 0, True)):
        res = V.voxel_means_host(xyz[first], sums, obs, voxel_m, min_count, min_span, fs if with_fs else None)
        want = numpy_means(xyz[first], sums, obs, voxel_m, min_count, min_span, fs if with_fs else None)
        assert same_bits(res["xyz_mean"].view(np.uint32), want[0].view(np.uint32)), (min_count, min_span)
        assert same_bits(res["gray_mean"], want[1]) and res["kept"] == want[2] == int(np.isfinite(res["xyz_mean"][:, 0]).sum())
    half = V.voxel_means_host(xyz[first], sums, obs, voxel_m, count=k // 2)   # a count below the capacity: nothing beyond it is written
    assert not half["xyz_mean"][k // 2:].any() and not half["gray_mean"][k // 2:].any() and half["kept"] == k // 2


def test_hand_made_lists():
    vm = 0.5   # exactly representable: the offsets below are exact
    # a voxel with one point: zero sums, the mean is f bit for bit
    one = np.array([[0.1, 0.2, 0.3]], F)
    st = V.voxel_stats_host(one, [200], vm, 4)
    assert st["total"] == 1 and not st["sums"][0, :3].any() and st["sums"][0, 3] == 200 and st["obs"].tolist() == [[1, 0]]
    res = V.voxel_means_host(one, st["sums"], st["obs"], vm)
    assert same_bits(res["xyz_mean"], one) and res["gray_mean"].tolist() == [200] and res["kept"] == 1
    # round half to even: offsets of (k + 1/2) units of vm / 2^20 — 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0, -1.5 -> -2
    unit = vm / 2 ** 20
    xs = np.array([0.0, 0.5, 1.5, 2.5, -0.5, -1.5]) * unit + 0.25
    pts = np.stack([xs, np.full(6, 0.25), np.full(6, 0.25)], axis=1).astype(F)
    assert ((pts[:, 0].astype(np.float64) - 0.25) / unit == np.array([0.0, 0.5, 1.5, 2.5, -0.5, -1.5])).all()   # the inputs are exact
    st = V.voxel_stats_host(pts, np.arange(6), vm, 4, [0, 0, 1, 3, 3, 2])
    assert st["total"] == 1 and st["sums"].tolist() == [[0 + 0 + 2 + 2 - 0 - 2, 0, 0, 15]] and st["obs"].tolist() == [[6, 3]]
    # grey: (2 * 15 + 6) / 12 = 3 (2.5 rounds half up); two points straddling a half
    assert V.voxel_means_host(pts[:1], st["sums"], st["obs"], vm)["gray_mean"].tolist() == [3]
    assert V.voxel_means_host(pts[:1], [[0, 0, 0, 3]], [[2, 0]], vm)["gray_mean"].tolist() == [2]
    assert V.voxel_means_host(pts[:1], [[0, 0, 0, 255 * 7]], [[7, 0]], vm)["gray_mean"].tolist() == [255]
    # a point without a key is neither ranked nor counted; capacity clipping: the voxel of rank >= capacity accumulates nothing
    pts = np.array([[0.1, 0.1, 0.1], [np.nan, 0, 0], [0.7, 0.1, 0.1], [0.2, 0.1, 0.1], [0.8, 0.1, 0.1], [1.2, 0.1, 0.1]], F)
    full = V.voxel_stats_host(pts, [10, 20, 30, 40, 50, 60], vm, 8, [0, 0, 0, 1, 1, 2])
    assert full["total"] == 3 and full["first_index"].tolist() == [0, 2, 5] and full["obs"].tolist() == [[2, 1], [2, 1], [1, 2]]
    assert full["sums"][:, 3].tolist() == [50, 80, 60]
    clip = V.voxel_stats_host(pts, [10, 20, 30, 40, 50, 60], vm, 2, [0, 0, 0, 1, 1, 2])
    assert clip["total"] == 3 and same_bits(clip["sums"], full["sums"][:2]) and same_bits(clip["obs"], full["obs"][:2])
    # NaN (one bit pattern) and grey 0 below min_count and below min_span; the other ranks keep their values
    f = pts[full["first_index"]]
    by_count = V.voxel_means_host(f, full["sums"], full["obs"], vm, min_count=2)
    assert (by_count["xyz_mean"][2].view(np.uint32) == NAN_BITS).all() and by_count["gray_mean"].tolist() == [25, 40, 0] and by_count["kept"] == 2
    by_span = V.voxel_means_host(f, full["sums"], full["obs"], vm, min_span=1, first_segment_of_rank=[0, 0, 2])
    assert np.isfinite(by_span["xyz_mean"][:2]).all() and (by_span["xyz_mean"][2].view(np.uint32) == NAN_BITS).all() and by_span["kept"] == 2
    everything = V.voxel_means_host(f, full["sums"], full["obs"], vm, min_count=0)   # min_count 0 is min_count 1: a rank is seen at least once
    assert np.isfinite(everything["xyz_mean"]).all() and everything["kept"] == 3
    assert same_bits(everything["xyz_mean"][2], f[2])
    mean_x = F(f[0, 0]) + F(F(vm) * F(float(full["sums"][0, 0]) / (2 * 1048576.0)))
    assert everything["xyz_mean"][0, 0] == mean_x and abs(float(mean_x) - 0.15) < 1e-6


def test_refusals():
    lib = V.lib()
    xyz, gray = np.zeros((4, 3), F), np.zeros(4, np.uint8)
    sums, obs = np.zeros((4, 4), np.int64), np.zeros((4, 2), np.uint32)
    for bad, word in ((0.0, "voxel size"), (-1.0, "voxel size"), (float("nan"), "voxel size"), (float("inf"), "voxel size")):
        with pytest.raises(V.VorsError, match=word):
            V.voxel_stats_host(xyz, gray, bad, 4)
        with pytest.raises(V.VorsError, match=word):
            V.voxel_means_host(xyz, sums, obs, bad)
    with pytest.raises(V.VorsError, match="capacity"):
        V.voxel_stats_host(xyz, gray, 0.1, 0)
    with pytest.raises(V.VorsError, match="min_span must be 0"):
        V.voxel_means_host(xyz, sums, obs, 0.1, min_span=1)
    with pytest.raises(V.VorsError):
        V.voxel_means_host(xyz, sums[:3], obs, 0.1)
    with pytest.raises(V.VorsError, match="min_count"):
        V.voxel_means_host(xyz, sums, obs, 0.1, min_count=-1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    kept = C.c_uint32()
    assert lib.vors_voxel_stats_host(None, p(gray), None, 4, 0.1, 4, None, None, p(sums), p(obs)) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_voxel_stats_host(p(xyz), p(gray), None, 4, 0.1, 4, None, None, None, p(obs)) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_voxel_stats_host(p(xyz), p(gray), None, 4, 0.1, 4, None, None, p(sums), p(obs)) == 0   # total and first_index may be NULL
    assert lib.vors_voxel_means_host(None, 4, 4, p(sums), p(obs), 0.1, 1, 0, None, None, None, C.byref(kept)) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_voxel_means_host(p(xyz), 4, 4, p(sums), p(obs), 0.1, 1, 0, None, None, None, None) == -1 and b"no output" in lib.vors_last_error()
    assert lib.vors_voxel_means_host(p(xyz), 4, 0, p(sums), p(obs), 0.1, 1, 0, None, None, None, C.byref(kept)) == -1 and b"capacity" in lib.vors_last_error()
    odd = np.zeros(4 * 4 * 8 + 8, np.uint8)
    assert lib.vors_voxel_means_host(p(xyz), 4, 4, C.c_void_p(odd.ctypes.data + 4), p(obs), 0.1, 1, 0, None, None, None, C.byref(kept)) == -1
    assert b"8-byte" in lib.vors_last_error()
    # the device entry refuses the same before it looks for a device; then the handles
    dk = C.c_void_p(64)   # (never dereferenced: every call below is refused first)
    assert lib.vors_voxel_means(0, dk, dk, 4, dk, dk, 0.1, 1, 0, None, dk, None, None, None) == -1 and b"n must be" in lib.vors_last_error()
    assert lib.vors_voxel_means(1, dk, None, 4, dk, dk, 0.1, 1, 0, None, dk, None, None, None) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_voxel_means(1, None, dk, 4, dk, dk, 0.1, 1, 0, None, dk, None, None, None) == -1 and b"NULL" in lib.vors_last_error()
    assert lib.vors_voxel_means(1, dk, dk, 4, dk, dk, 0.1, 1, 0, None, None, None, None, None) == -1 and b"no output" in lib.vors_last_error()
    assert lib.vors_voxel_means(1, dk, dk, 4, C.c_void_p(68), dk, 0.1, 1, 0, None, dk, None, None, None) == -1 and b"8-byte" in lib.vors_last_error()
    assert lib.vors_voxel_means(1, dk, dk, 4, dk, C.c_void_p(66), 0.1, 1, 0, None, dk, None, None, None) == -1 and b"4-byte" in lib.vors_last_error()
    assert lib.vors_voxel_means(1, dk, dk, 4, dk, dk, 0.0, 1, 0, None, dk, None, None, None) == -1 and b"voxel size" in lib.vors_last_error()
    assert lib.vors_voxel_means(1, dk, dk, 0, dk, dk, 0.1, 1, 0, None, dk, None, None, None) == -1 and b"capacity" in lib.vors_last_error()
    assert lib.vors_voxel_means(1, dk, dk, 4, dk, dk, 0.1, 1, 1, None, dk, None, None, None) == -1 and b"min_span" in lib.vors_last_error()
    for call in (lambda: lib.vors_trackers_enable_map_voxel_stats(None), lambda: lib.vors_trackers_map_voxel_stats(None, None, None),
                 lambda: lib.vors_trackers_map_voxel_means(None, 1, 0, dk, None, None, None), lambda: lib.vors_tracker_enable_map_voxel_stats(None),
                 lambda: lib.vors_tracker_read_map_voxel_stats(None, 0, None, None),
                 lambda: lib.vors_tracker_map_voxel_means(None, 1, 0, 0, None, None, C.byref(kept))):
        assert call() == -1 and b"handle t is NULL" in lib.vors_last_error()
    for name in ("vors_trackers_enable_map_voxel_stats", "vors_trackers_map_voxel_stats", "vors_trackers_map_voxel_means",
                 "vors_tracker_enable_map_voxel_stats", "vors_tracker_read_map_voxel_stats", "vors_tracker_map_voxel_means", "vors_voxel_means",
                 "vors_voxel_means_host", "vors_voxel_stats_host"):
        assert name in V.EXPORTED_SYMBOLS and hasattr(lib, name)
