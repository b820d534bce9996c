"""The host twins of the corrected map (vors_repose_points_host, vors_voxel_filter_points_host; include/vors_hip.h 2i; no
GPU): the re-pose against a float64 numpy restatement of the same two-step formula, its statements on bits, the filter against a Python
dictionary over V.voxel_keys, and every refusal of the four entries.

The tolerance of the f64 comparison is the issue's: a moved point within 64 * 2^-24 * (|p| + |t_A| + |t_B|) of the restatement, a moved
normal within 64 * 2^-24 — two rotations of about a dozen roundings each on magnitudes bounded by |p| + |t_A|, plus two translations.
Measured here (recorded in DESIGN.md 7w): the largest ratio error / bound is 0.047 for points and 0.062 for normals."""
import ctypes as C

import numpy as np
import pytest

import vors_amd as V

F = np.float32
EPS = 64.0 * 2.0 ** -24
INVALID = -1  # VORS_ERR_INVALID_ARGUMENT
SEG = V.MAP_SEGMENT_DTYPE


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def random_poses(rng, k, trans=2.0):
    """k poses (t, q): the quaternion normalised in f64, then cast."""
    q = rng.normal(size=(k, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([rng.uniform(-trans, trans, (k, 3)), q], axis=1).astype(F)


def segments_of(sizes, poses):
    seg = np.zeros(len(sizes), SEG)
    seg["frame"] = 3 * np.arange(len(sizes))
    seg["count"] = sizes
    seg["first"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    seg["pose7"] = poses
    return seg


def rot64(q, v):
    """UnitQuaternion * Vector3 in f64 (q = i, j, k, w)."""
    qv, w = q[:3], q[3]
    t = 2.0 * np.cross(qv, v)
    return v + w * t + np.cross(qv, t)


def repose64(a, b, p):
    a, b, p = a.astype(np.float64), b.astype(np.float64), p.astype(np.float64)
    c = rot64(np.concatenate([-a[3:6], a[6:]]), p - a[:3])
    return rot64(b[3:], c) + b[:3]


def normal64(a, b, n):
    a, b, n = a.astype(np.float64), b.astype(np.float64), n.astype(np.float64)
    return rot64(b[3:], rot64(np.concatenate([-a[3:6], a[6:]]), n))


def scene(seed, sizes, nan_rows=0):
    rng = np.random.default_rng(seed)
    n = int(np.sum(sizes))
    xyz = rng.uniform(-4, 4, (n, 3)).astype(F)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    for r in rng.choice(n, nan_rows, replace=False) if nan_rows else []:
        xyz[r, rng.integers(3)] = np.array([0x7FC01234], np.uint32).view(F)[0]  # a NaN with a payload
    a, b = random_poses(rng, len(sizes)), random_poses(rng, len(sizes))
    return xyz, nrm, segments_of(sizes, a), b


def segment_of_rank(seg, n):
    out = np.full(n, -1)
    for k, s in enumerate(seg):
        out[s["first"]:min(int(s["first"]) + int(s["count"]), n)] = k
    return out


SIZES = [0, 1, 7, 64, 65, 300, 0, 5, 129]


def test_twin_against_float64_restatement():
    xyz, nrm, seg, b = scene(1, SIZES)
    out = V.repose_points_host(xyz, seg, b, normals=nrm)
    owner = segment_of_rank(seg, len(xyz))
    worst_p = worst_n = 0.0
    for r in range(len(xyz)):
        a7, b7 = seg["pose7"][owner[r]], b[owner[r]]
        bound = EPS * (np.linalg.norm(xyz[r].astype(np.float64)) + np.linalg.norm(a7[:3].astype(np.float64)) + np.linalg.norm(b7[:3].astype(np.float64)))
        ep = np.linalg.norm(out["xyz"][r].astype(np.float64) - repose64(a7, b7, xyz[r]))
        en = np.linalg.norm(out["normals"][r].astype(np.float64) - normal64(a7, b7, nrm[r]))
        worst_p, worst_n = max(worst_p, ep / bound), max(worst_n, en / EPS)
    print(f"largest error / bound: points {worst_p:.3f}, normals {worst_n:.3f}")
    assert worst_p <= 1.0 and worst_n <= 1.0
    c = out["counts"]
    assert c[0] == len(xyz) and c[1] == c[2] == c[3] == 0 and c[4] == len(SIZES)
    assert (out["segments"]["pose7"].view(np.uint32) == b.view(np.uint32)).all()
    for name in ("frame", "first", "count"):
        assert (out["segments"][name] == seg[name]).all()


def test_own_poses_are_the_identity_on_bits():
    xyz, nrm, seg, _ = scene(2, SIZES, nan_rows=9)
    out = V.repose_points_host(xyz, seg, seg["pose7"].copy(), normals=nrm)
    assert (bits(out["xyz"]) == bits(xyz)).all() and (bits(out["normals"]) == bits(nrm)).all()
    assert out["segments"].tobytes() == seg.tobytes()
    assert out["counts"].tolist() == [0, len(xyz) - 9, 9, 0, 0, 0]


def test_there_and_back():
    xyz, nrm, seg, b = scene(3, SIZES, nan_rows=11)
    b[3] = seg["pose7"][3]  # kept by identical bits
    nos = np.arange(len(SIZES), dtype=np.uint32)
    nos[5] = V.REPOSE_NO_NODE  # kept: not in the graph
    fwd = V.repose_points_host(xyz, seg, b, normals=nrm, node_of_segment=nos)
    back = V.repose_points_host(fwd["xyz"], fwd["segments"], seg["pose7"].copy(), normals=fwd["normals"], node_of_segment=nos)
    owner = segment_of_rank(seg, len(xyz))
    still = np.isin(owner, [3, 5]) | ~np.isfinite(xyz).all(1)
    assert (bits(fwd["xyz"])[still] == bits(xyz)[still]).all() and (bits(back["xyz"])[still] == bits(xyz)[still]).all()
    assert (bits(back["normals"])[np.isin(owner, [3, 5])] == bits(nrm)[np.isin(owner, [3, 5])]).all()
    assert back["segments"].tobytes() == seg.tobytes()
    for r in np.flatnonzero(~still):
        a7, b7 = seg["pose7"][owner[r]], b[owner[r]]
        bound = EPS * (np.linalg.norm(xyz[r].astype(np.float64)) + np.linalg.norm(a7[:3].astype(np.float64)) + np.linalg.norm(b7[:3].astype(np.float64)))
        assert np.linalg.norm(back["xyz"][r].astype(np.float64) - xyz[r].astype(np.float64)) <= 2 * bound
        assert np.linalg.norm(back["normals"][r].astype(np.float64) - nrm[r].astype(np.float64)) <= 2 * EPS


def test_segments_left_alone_and_counted():
    xyz, nrm, seg, b = scene(4, SIZES, nan_rows=5)
    nos = np.arange(len(SIZES), dtype=np.uint32)
    nos[2] = V.REPOSE_NO_NODE          # the sentinel
    nos[3] = 7                         # a node at or beyond node_count (7 below)
    nos[4], nos[5] = 4, 5
    b[4, 1] = np.inf                   # a non-finite new pose
    b[5] = seg["pose7"][5]             # identical bits
    nos[7], nos[8] = 0, 1
    out = V.repose_points_host(xyz, seg, b, normals=nrm, node_of_segment=nos, node_count=7)
    owner = segment_of_rank(seg, len(xyz))
    alone = np.isin(owner, [2, 3, 4, 5])
    assert (bits(out["xyz"])[alone] == bits(xyz)[alone]).all() and (bits(out["normals"])[alone] == bits(nrm)[alone]).all()
    assert out["segments"][[2, 3, 4, 5]].tobytes() == seg[[2, 3, 4, 5]].tobytes()
    finite = np.isfinite(xyz).all(1)
    nan = ~finite
    assert (bits(out["xyz"])[nan] == bits(xyz)[nan]).all()  # with their payloads
    moved_seg = [k for k in range(len(SIZES)) if k not in (2, 3, 4, 5)]
    moved = np.isin(owner, moved_seg) & finite
    c = out["counts"]
    assert c[0] == moved.sum() and c[1] == (alone & finite).sum() and c[2] == nan.sum() and c[3] == 0 and c[4] == len(moved_seg)
    assert (bits(out["xyz"])[moved] != bits(xyz)[moved]).any(1).all()
    # the largest shift: the maximum of the twin's own shifts, taken the way the text takes it (f32, contraction off)
    d = (out["xyz"][moved] - xyz[moved]).astype(F)
    s = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)).astype(F)
    assert c[5] == s.view(np.uint32).max()


def test_ranks_without_a_record_and_clipping():
    xyz, nrm, seg, b = scene(5, [10, 20, 30, 40])
    # two records used of four: the ranks of the last two keyframes have no record; count beyond capacity is clipped
    out = V.repose_points_host(xyz, seg, b, normals=nrm, n_segments=9, count=10 ** 6)
    assert out["counts"].tolist()[:5] == [100, 0, 0, 0, 4]
    out = V.repose_points_host(xyz[:70], seg[:2], b, normals=nrm[:70], n_segments=4)
    assert out["counts"].tolist()[:5] == [30, 0, 0, 40, 2]
    assert (bits(out["xyz"])[30:] == bits(xyz)[30:70]).all() and (bits(out["normals"])[30:] == bits(nrm)[30:70]).all()
    # an empty list, and a list clipped inside a segment
    out = V.repose_points_host(xyz, seg, b, count=0)
    assert out["counts"].tolist() == [0, 0, 0, 0, 4, 0] and (bits(out["xyz"]) == bits(xyz)).all()
    out = V.repose_points_host(xyz, seg, b, count=15)
    assert out["counts"].tolist()[:4] == [15, 0, 0, 0] and (bits(out["xyz"])[15:] == bits(xyz)[15:]).all()


def dict_filter(xyz, voxel_m):
    keys = V.voxel_keys(voxel_m, xyz)
    seen, index = set(), []
    for r, k in enumerate(keys.tolist()):
        if k != V.VOXEL_NONE and k not in seen:
            seen.add(k)
            index.append(r)
    return np.array(index, np.uint32)


@pytest.mark.parametrize("kind", ["grid", "all_duplicates", "no_duplicates", "none_keys"])
def test_filter_twin_against_dictionary(kind):
    rng = np.random.default_rng(7)
    n = 700
    if kind == "grid":
        xyz = (rng.integers(-6, 6, (n, 3)) * 0.05 + rng.uniform(0.001, 0.049, (n, 3))).astype(F)
    elif kind == "all_duplicates":
        xyz = np.tile(np.array([[0.31, -0.2, 1.7]], F), (n, 1)) + rng.uniform(0, 0.01, (n, 3)).astype(F)
    elif kind == "no_duplicates":
        xyz = (np.stack(np.unravel_index(rng.permutation(1000)[:n], (10, 10, 10)), 1) * 0.05 + 0.02).astype(F)
    else:
        xyz = (rng.integers(-3, 3, (n, 3)) * 0.05 + 0.01).astype(F)
        xyz[::5, 0] = np.nan
        xyz[3::7, 2] = 1e30
    pixel = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    gray = rng.integers(0, 256, n).astype(np.uint8)
    nrm = rng.normal(size=(n, 3)).astype(F)
    index = dict_filter(xyz, 0.05)
    out = V.voxel_filter_points_host(xyz, 0.05, 1024, pixel=pixel, gray=gray, normals=nrm)
    assert out["count"] == len(index) and out["overflow"] == 0 and (out["index"] == index).all()
    assert (bits(out["xyz"]) == bits(xyz[index])).all() and (out["pixel"] == pixel[index]).all() and (out["gray"] == gray[index]).all()
    assert (bits(out["normals"]) == bits(nrm[index])).all()
    if kind == "all_duplicates":
        assert out["count"] == 1
    if kind == "no_duplicates":
        assert out["count"] == n
    assert V.voxel_filter_points_host(xyz, 0.05, 64)["overflow"] == (1 if len(index) > 64 else 0)


def test_filter_rewrites_segments_with_an_emptied_middle():
    rng = np.random.default_rng(8)
    a = (rng.integers(0, 5, (40, 3)) * 0.1 + 0.05).astype(F)
    xyz = np.concatenate([a, a[rng.integers(0, 40, 25)], (rng.integers(5, 9, (30, 3)) * 0.1 + 0.05).astype(F)])  # the middle repeats the first
    seg = segments_of([40, 25, 0, 30], random_poses(rng, 4))
    out = V.voxel_filter_points_host(xyz, 0.1, 256, segments=seg)
    index = dict_filter(xyz, 0.1)
    want_first = [int((index < f).sum()) for f in seg["first"]]
    want_count = [int(((index >= f) & (index < f + c)).sum()) for f, c in zip(seg["first"].astype(int), seg["count"].astype(int))]
    assert out["segments"]["first"].tolist() == want_first and out["segments"]["count"].tolist() == want_count
    assert want_count[1] == 0 and want_count[2] == 0 and sum(want_count) == out["count"]
    assert (out["segments"]["frame"] == seg["frame"]).all() and out["segments"]["pose7"].tobytes() == seg["pose7"].tobytes()


def test_repose_then_filter_keeps_one_point_per_voxel():
    xyz, nrm, seg, b = scene(9, [200, 300, 250])
    xyz = (xyz * 0.1).astype(F)
    b[:] = seg["pose7"]
    b[1, :3] += F(0.02)  # the middle keyframe slides into its neighbours
    moved = V.repose_points_host(xyz, seg, b, normals=nrm)
    out = V.voxel_filter_points_host(moved["xyz"], 0.05, 2048, normals=moved["normals"], segments=moved["segments"])
    keys = V.voxel_keys(0.05, out["xyz"])
    assert len(np.unique(keys)) == len(keys) == out["count"] and V.VOXEL_NONE not in keys.tolist()
    assert set(keys.tolist()) == set(V.voxel_keys(0.05, moved["xyz"]).tolist()) - {V.VOXEL_NONE}
    assert int(out["segments"]["count"].sum()) == out["count"]


# --------------------------------------------------------------------------------------------------------- refusals
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class ReposeArgs:
    def __init__(self):
        self.xyz, self.nrm, seg, self.b = scene(11, [4, 4])
        self.seg = seg
        self.xo, self.no, self.so, self.co = self.xyz.copy(), self.nrm.copy(), seg.copy(), np.zeros(6, np.uint32)
        self.nos = np.arange(2, dtype=np.uint32)
        self.kw = dict(count=8, capacity=8, n_segments=2, max_keyframes=2, node_count=2, node_capacity=2)

    def host(self, **over):
        a = dict(xyz=_p(self.xyz), normals=_p(self.nrm), segments=_p(self.seg), poses=_p(self.b), nos=_p(self.nos), xo=_p(self.xo), no=_p(self.no),
                 so=_p(self.so), co=_p(self.co), **self.kw)
        a.update(over)
        return V.lib().vors_repose_points_host(a["xyz"], a["normals"], a["count"], a["capacity"], a["segments"], a["n_segments"], a["max_keyframes"],
                                               a["poses"], a["node_count"], a["node_capacity"], a["nos"], a["xo"], a["no"], a["so"], a["co"])

    def device(self, n=1, stride=0, **over):
        a = dict(xyz=_p(self.xyz), normals=_p(self.nrm), segments=_p(self.seg), poses=_p(self.b), nos=_p(self.nos), xo=_p(self.xo), no=_p(self.no),
                 so=_p(self.so), co=_p(self.co), counts=_p(self.co), **self.kw)
        a.update(over)
        return V.lib().vors_repose_points(n, a["xyz"], a["normals"], a["counts"], a["capacity"], a["segments"], a["counts"], a["max_keyframes"],
                                          a["poses"], stride, a["node_capacity"], a["counts"], a["nos"], a["xo"], a["no"], a["so"], None, None)


def off(a, nbytes):
    return C.c_void_p(a.ctypes.data + nbytes)


def test_repose_refusals():
    r = ReposeArgs()
    assert r.host() == 0
    for over in (dict(xyz=None), dict(segments=None), dict(poses=None), dict(xo=None, no=None), dict(normals=None),  # normals_out without normals
                 dict(capacity=0), dict(max_keyframes=0), dict(node_capacity=0),
                 dict(xyz=off(r.xyz, 2)), dict(xo=off(r.xo, 1)), dict(so=off(r.so, 2)),
                 dict(xo=off(r.xyz, 12), capacity=7), dict(no=_p(r.xyz)), dict(xo=_p(r.nrm)), dict(so=off(r.seg, 20), max_keyframes=1),
                 dict(co=_p(r.nos)), dict(no=_p(r.xo))):
        assert r.host(**over) == INVALID, over
        assert b"repose_points_host" in V.lib().vors_last_error()
    # exact aliasing is legal
    assert r.host(xo=_p(r.xyz), no=_p(r.nrm), so=_p(r.seg)) == 0
    # the device entry refuses the same before it looks for a device, and bad strides and n besides
    for kw in (dict(n=0), dict(n=65536), dict(stride=24), dict(stride=30), dict(xyz=None), dict(xo=None, no=None), dict(normals=None),
               dict(capacity=0), dict(xo=off(r.xyz, 12), capacity=7), dict(xo=off(r.xo, 2))):
        assert r.device(**kw) == INVALID, kw
    assert V.lib().vors_trackers_repose_map(None, _p(r.b), 0, 2, _p(r.co), None, _p(r.xo), None, None, None, None) == INVALID


def test_filter_refusals():
    rng = np.random.default_rng(12)
    xyz = rng.uniform(0, 1, (16, 3)).astype(F)
    index, xo = np.zeros(16, np.uint32), np.zeros((16, 3), F)
    pixel, gray = np.zeros(16, np.uint32), np.zeros(16, np.uint8)
    seg = segments_of([16], random_poses(rng, 1))
    so = seg.copy()
    kept, over = C.c_uint32(), C.c_uint32()

    def host(**o):
        a = dict(xyz=_p(xyz), count=16, capacity=16, voxel_m=0.1, slots=64, pixel=None, gray=None, normals=None, segments=None, n_segments=0,
                 max_keyframes=0, index=_p(index), kept=C.byref(kept), over=C.byref(over), xo=_p(xo), po=None, go=None, no=None, so=None)
        a.update(o)
        return V.lib().vors_voxel_filter_points_host(a["xyz"], a["count"], a["capacity"], a["voxel_m"], a["slots"], a["pixel"], a["gray"], a["normals"],
                                                     a["segments"], a["n_segments"], a["max_keyframes"], a["index"], a["kept"], a["over"], a["xo"],
                                                     a["po"], a["go"], a["no"], a["so"])
    assert host() == 0
    assert host(segments=_p(seg), n_segments=1, max_keyframes=1, so=_p(so)) == 0
    for o in (dict(xyz=None), dict(index=None), dict(kept=None), dict(over=None), dict(capacity=0), dict(voxel_m=0.0), dict(voxel_m=float("nan")),
              dict(voxel_m=float("inf")), dict(slots=63), dict(slots=96), dict(slots=32), dict(slots=-64), dict(po=_p(pixel)), dict(go=_p(gray)),
              dict(no=_p(xo)), dict(so=_p(so)), dict(segments=_p(seg), n_segments=1, max_keyframes=0, so=_p(so)),
              dict(xo=_p(xyz)), dict(xo=off(xyz, 12), capacity=15), dict(index=_p(xo)), dict(xyz=off(xyz, 2)),
              dict(segments=_p(seg), n_segments=1, max_keyframes=1, so=_p(seg)), dict(pixel=_p(pixel), po=_p(pixel))):
        assert host(**o) == INVALID, o
        assert b"voxel_filter_points_host" in V.lib().vors_last_error()
    # the device entry: its own refusals come before the device is looked for
    lib = V.lib()
    ws = np.zeros(V.voxel_filter_workspace_bytes(1, 16, 64) + 16, np.uint8)
    assert V.voxel_filter_workspace_bytes(1, 16, 64) == 64 * 16 + 4 + 4
    assert V.voxel_filter_workspace_bytes(0, 16, 64) == 0 and V.voxel_filter_workspace_bytes(1, 0, 64) == 0 and V.voxel_filter_workspace_bytes(1, 16, 8) == 0
    base = ws.ctypes.data + (-ws.ctypes.data) % 16
    cnt, cnt_out, ovf = np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros(1, np.uint32)

    def device(n=1, w=C.c_void_p(base), slots=64, xyz_=_p(xyz), xo_=_p(xo), index_=_p(index)):
        return lib.vors_voxel_filter_points(n, xyz_, _p(cnt), 16, 0.1, slots, w, None, None, None, None, None, 0, index_, _p(cnt_out), _p(ovf), xo_,
                                            None, None, None, None, None)
    for kw in (dict(n=0), dict(n=65536), dict(w=None), dict(w=C.c_void_p(base + 8)), dict(slots=100), dict(xyz_=None), dict(xo_=_p(xyz)),
               dict(index_=C.c_void_p(base))):
        assert device(**kw) == INVALID, kw
    for name in ("vors_repose_points", "vors_repose_points_host", "vors_trackers_repose_map", "vors_voxel_filter_points",
                 "vors_voxel_filter_points_host", "vors_voxel_filter_workspace_bytes"):
        assert name in V.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert V.REPOSE_COUNTS == 6
