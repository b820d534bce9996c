"""The corrected map on the device (vors_repose_points, vors_voxel_filter_points, vors_trackers_repose_map; include/vors_hip.h 2i,
DESIGN.md 7w) against the host twins, against the trackers' own voxel-filtered map and through the handle. GPU only; every comparison is
on bits, nothing has a tolerance.

Shapes: the point pass gives a lane 4 ranks and a workgroup 1024, the filter sweeps 256 ranks at a time in chunks of 1024 — the list
counts 1 .. 3001 put list ends and segment boundaries inside a lane's group, inside a wavefront, inside a chunk and in a later chunk.
Every output is a tensor filled with a sentinel before the call, so that what lies beyond the clipped count (and beyond the used records)
is checked to be untouched.

The map tests run three sequences of tests/test_gpu_trackers_map.py's dense scene (120x160, 4 levels; twists BASE * SPEED of sequences
0, 2 and 4, which promote 3, 3 and 4 times in 8 frames as asserted below: at least two keyframes per sequence)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V

F = np.float32
SEG = V.MAP_SEGMENT_DTYPE
COUNTS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3001]
SENTINEL = 0x5EA7BEEF  # (a NaN-free f32 pattern: comparisons are on bits anyway)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == SEG:
        a = a.view(np.uint8).reshape(a.shape + (40,))
    return torch.from_numpy(a).cuda()


def host(t, dtype=None):
    a = t.cpu().numpy()
    if dtype == SEG:
        return np.ascontiguousarray(a).view(SEG)[..., 0]
    return a.view(dtype) if dtype is not None else a


def filled(shape, dtype, offset_words=0):
    """A sentinel-filled tensor of `shape`; offset_words > 0: a window that starts that many 4-byte words into a larger buffer."""
    import torch
    words = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4
    if torch.empty(0, dtype=dtype).element_size() == 1:
        buf = torch.full((int(np.prod(shape)),), 0xEF, dtype=torch.uint8, device="cuda")
        return buf.view(shape)
    buf = torch.full((words + offset_words + 4,), SENTINEL, dtype=torch.int32, device="cuda")
    return buf[offset_words:offset_words + words].view(dtype).view(shape)


def layout_sizes(layout, count):
    if layout == "one":
        return [count]
    if layout == "ones":
        return [1] * count
    sizes, cyc = [], [0, 1, 7, 64, 65, 300]
    while sum(sizes) < count:
        sizes.append(cyc[len(sizes) % 6])
    return sizes  # (the last one may reach beyond the list: clipped by the count)


def random_poses(rng, shape):
    q = rng.normal(size=shape + (4,))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    return np.concatenate([rng.uniform(-2, 2, shape + (3,)), q], axis=-1).astype(F)


def make_case(seed, counts, layout, capacity=None, max_kf=None, width=7, node_table=True, nan_every=37, count_over=0, seg_over=0):
    """n = len(counts) lists. A quarter of the segments keep their pose bits; with node_table every fifth segment is not in the graph and
    the nodes are a permutation; NaN rows every nan_every ranks."""
    rng = np.random.default_rng(seed)
    n = len(counts)
    sizes = [layout_sizes(layout, c) for c in counts]
    cap = capacity or max(counts)
    nkf = max_kf or max(len(s) for s in sizes)
    xyz = rng.uniform(-4, 4, (n, cap, 3)).astype(F)
    nrm = rng.normal(size=(n, cap, 3)).astype(F)
    xyz[:, 2::nan_every, 1] = np.nan
    nrm[:, 5::nan_every * 2, 0] = np.inf
    seg = np.zeros((n, nkf), SEG)
    seg["pose7"] = random_poses(rng, (n, nkf))
    n_seg = np.zeros(n, np.uint32)
    for i, s in enumerate(sizes):
        k = min(len(s), nkf)
        seg["count"][i, :k] = s[:k]
        seg["first"][i, :k] = np.concatenate([[0], np.cumsum(s)[:-1]])[:k]
        seg["frame"][i, :k] = 2 * np.arange(k)
        n_seg[i] = len(s) + (seg_over if len(s) >= nkf else 0)  # (records beyond a list's own stay unused: their `first` does not ascend)
    ncap = nkf + 3
    poses = rng.uniform(-1, 1, (n, ncap, width)).astype(F)
    poses[:, :, :7] = random_poses(rng, (n, ncap))
    node_counts = np.full(n, ncap - 1, np.uint32)
    nos = None
    if node_table:
        nos = np.stack([rng.permutation(ncap)[:nkf] for _ in range(n)]).astype(np.uint32)
        nos[:, 4::5] = V.REPOSE_NO_NODE
    for i in range(n):
        for k in range(0, nkf, 4):  # kept by identical bits
            node = k if nos is None else int(nos[i, k])
            if node < ncap:
                poses[i, node, :7] = seg["pose7"][i, k]
    list_counts = (np.array(counts) + count_over).astype(np.uint32)
    return dict(xyz=xyz, nrm=nrm, seg=seg, n_seg=n_seg, poses=poses, node_counts=node_counts, nos=nos, list_counts=list_counts, cap=cap, nkf=nkf)


def twin(c, i, normals=True):
    return V.repose_points_host(c["xyz"][i], c["seg"][i], np.ascontiguousarray(c["poses"][i, :, :7]), normals=c["nrm"][i] if normals else None,
                                node_of_segment=None if c["nos"] is None else c["nos"][i], count=int(c["list_counts"][i]),
                                n_segments=int(c["n_seg"][i]), node_count=int(c["node_counts"][i]))


def run_device(c, normals=True, offset_words=0, in_place=False):
    import torch
    n, cap, nkf = len(c["list_counts"]), c["cap"], c["nkf"]
    if offset_words:  # the inputs too start at a 4-byte but not 16-byte aligned offset of a larger buffer
        xyz, nrm = filled((n, cap, 3), torch.float32, offset_words), filled((n, cap, 3), torch.float32, offset_words)
        xyz.copy_(dev(c["xyz"]))
        nrm.copy_(dev(c["nrm"]))
    else:
        xyz, nrm = dev(c["xyz"]), dev(c["nrm"])
    seg = dev(c["seg"])
    if in_place:
        outs = dict(xyz_out=xyz, normals_out=nrm if normals else False, segments_out=seg)
    else:
        outs = dict(xyz_out=filled((n, cap, 3), torch.float32, offset_words), normals_out=filled((n, cap, 3), torch.float32, offset_words) if normals else False,
                    segments_out=filled((n, nkf, 40), torch.uint8))
    out = V.repose_points(xyz, dev(c["list_counts"]), seg, dev(c["n_seg"]), dev(c["poses"]), dev(c["node_counts"]), normals=nrm if normals else None,
                          node_of_segment=None if c["nos"] is None else dev(c["nos"]), counts=filled((n, V.REPOSE_COUNTS), torch.int32), **outs)
    torch.cuda.synchronize()
    return out


def check_against_twin(c, out, normals=True, in_place=False):
    for i in range(len(c["list_counts"])):
        t = twin(c, i, normals)
        total = min(int(c["list_counts"][i]), c["cap"])
        n_rec = min(int(c["n_seg"][i]), c["nkf"])
        got = host(out["xyz"][i], np.uint32)
        assert (got[:total] == t["xyz"].view(np.uint32)[:total]).all(), (i, total)
        beyond = c["xyz"][i].view(np.uint32)[total:] if in_place else SENTINEL
        assert (got[total:] == beyond).all()
        if normals:
            got = host(out["normals"][i], np.uint32)
            assert (got[:total] == t["normals"].view(np.uint32)[:total]).all(), (i, total)
            assert (got[total:] == (c["nrm"][i].view(np.uint32)[total:] if in_place else SENTINEL)).all()
        got = host(out["segments"][i])
        assert got[:n_rec].tobytes() == t["segments"][:n_rec].tobytes(), (i, n_rec)
        assert (got[n_rec:] == (c["seg"][i][n_rec:].view(np.uint8).reshape(-1, 40) if in_place else 0xEF)).all()
        assert (host(out["counts"][i], np.uint32) == t["counts"]).all(), (i, host(out["counts"][i], np.uint32), t["counts"])
        assert t["counts"][:4].sum() == total


@pytest.mark.parametrize("layout", ["one", "ones", "cycle"])
def test_device_equals_twin(layout):
    for k, count in enumerate(COUNTS):
        c = make_case(100 + k, [count], layout, node_table=k % 2 == 1)
        check_against_twin(c, run_device(c))
    c = make_case(130, [3001], layout)
    check_against_twin(c, run_device(c, normals=False), normals=False)


def test_three_lists_clipped_counts_and_unrecorded_keyframes():
    c = make_case(200, [1025, 64, 3001], "cycle")                       # different counts and segment numbers per list
    check_against_twin(c, run_device(c))
    c = make_case(201, [257, 1024, 5], "cycle", count_over=1000, capacity=1030)   # count > capacity in lists 0 and 1; list 2 has ranks no record covers
    check_against_twin(c, run_device(c))
    c = make_case(202, [3001, 1025, 300], "cycle", max_kf=9, seg_over=2)  # n_segments > max_keyframes: the later ranks have no record
    out = run_device(c)
    check_against_twin(c, out)
    assert host(out["counts"], np.uint32)[0, 3] > 0
    c = make_case(203, [1023, 257, 3001], "ones", width=9)              # poses in 9-float rows (stride 36)
    check_against_twin(c, run_device(c))


def test_lists_at_an_odd_offset_and_in_place():
    c = make_case(300, [3001, 1025, 255], "cycle", capacity=3001)        # capacity * 12 is no multiple of 16 either
    for words in (1, 2, 3):
        check_against_twin(c, run_device(c, offset_words=words))
    for case in (c, make_case(301, [1024, 1024, 64], "cycle")):          # aligned lists take the 16-byte path
        check_against_twin(case, run_device(case, in_place=True), in_place=True)
        check_against_twin(case, run_device(case, in_place=True, normals=False), normals=False, in_place=True)


# ------------------------------------------------------------------------------------------------------------ the filter
def grid_points(rng, n, cells, voxel_m=0.05):
    """n points in `cells` distinct voxels of a coarse grid (every voxel hit when n >= cells), the order shuffled."""
    base = np.stack(np.unravel_index(rng.permutation(32 ** 3)[:cells], (32, 32, 32)), 1) - 16
    pick = np.concatenate([np.arange(min(cells, n)), rng.integers(0, cells, max(n - cells, 0))])
    rng.shuffle(pick)
    return ((base[pick] + rng.uniform(0.1, 0.9, (n, 3))) * voxel_m).astype(F)


def filter_case(seed, counts, cells, capacity=None, segments=True):
    rng = np.random.default_rng(seed)
    n, cap = len(counts), capacity or max(counts)
    xyz = np.zeros((n, cap, 3), F)
    for i, cnt in enumerate(counts):
        xyz[i, :min(cnt, cap)] = grid_points(rng, min(cnt, cap), cells if isinstance(cells, int) else cells[i])
    xyz[:, 3::41, 2] = np.nan  # rows without a key
    c = dict(xyz=xyz, pixel=rng.integers(0, 2 ** 31, (n, cap)).astype(np.uint32), gray=rng.integers(0, 256, (n, cap)).astype(np.uint8),
             nrm=rng.normal(size=(n, cap, 3)).astype(F), list_counts=np.array(counts, np.uint32), cap=cap)
    if segments:
        sizes = [layout_sizes("cycle", cnt) for cnt in counts]
        nkf = max(len(s) for s in sizes)
        seg = np.zeros((n, nkf), SEG)
        seg["pose7"] = random_poses(rng, (n, nkf))
        for i, s in enumerate(sizes):
            seg["count"][i, :len(s)] = s
            seg["first"][i, :len(s)] = np.concatenate([[0], np.cumsum(s)[:-1]])
        c.update(seg=seg, n_seg=np.array([len(s) for s in sizes], np.uint32), nkf=nkf)
    return c


def run_filter(c, slots, voxel_m=0.05):
    import torch
    n, cap = len(c["list_counts"]), c["cap"]
    kw = {}
    if "seg" in c:
        kw = dict(segments=dev(c["seg"]), n_segments=dev(c["n_seg"]), segments_out=filled((n, c["nkf"], 40), torch.uint8))
    out = V.voxel_filter_points(dev(c["xyz"]), dev(c["list_counts"]), voxel_m, slots, pixel=dev(c["pixel"]), gray=dev(c["gray"]), normals=dev(c["nrm"]),
                                index=filled((n, cap), torch.int32), xyz_out=filled((n, cap, 3), torch.float32), pixel_out=filled((n, cap), torch.int32),
                                gray_out=filled((n, cap), torch.uint8), normals_out=filled((n, cap, 3), torch.float32), **kw)
    torch.cuda.synchronize()
    return {k: host(v) for k, v in out.items()}


def check_filter(c, out, slots, lists=None, voxel_m=0.05):
    for i in (range(len(c["list_counts"])) if lists is None else lists):
        t = V.voxel_filter_points_host(c["xyz"][i], voxel_m, slots, pixel=c["pixel"][i], gray=c["gray"][i], normals=c["nrm"][i],
                                       segments=c.get("seg", [None] * 9)[i], count=int(c["list_counts"][i]),
                                       n_segments=None if "seg" not in c else int(c["n_seg"][i]))
        k = t["count"]
        assert out["counts"][i] == k and out["overflow"][i] == 0 and t["overflow"] == 0
        assert (out["index"][i].view(np.uint32)[:k] == t["index"]).all() and (out["index"][i].view(np.uint32)[k:] == SENTINEL).all()
        assert (out["xyz"][i].view(np.uint32)[:k] == t["xyz"].view(np.uint32)).all() and (out["xyz"][i].view(np.uint32)[k:] == SENTINEL).all()
        assert (out["normals"][i].view(np.uint32)[:k] == t["normals"].view(np.uint32)).all()
        assert (out["pixel"][i].view(np.uint32)[:k] == t["pixel"]).all() and (out["gray"][i][:k] == t["gray"]).all() and (out["gray"][i][k:] == 0xEF).all()
        if "seg" in c:
            n_rec = int(c["n_seg"][i])
            got = np.ascontiguousarray(out["segments"][i]).view(SEG)[:, 0]
            assert got[:n_rec].tobytes() == t["segments"][:n_rec].tobytes() and (out["segments"][i][n_rec:] == 0xEF).all()


def test_filter_device_equals_twin():
    for k, count in enumerate(COUNTS):
        c = filter_case(400 + k, [count], max(count // 2, 1))  # about half of the entries are duplicates
        check_filter(c, run_filter(c, 4096), 4096)
    # three lists; in the long ones most first occurrences lie in an earlier chunk than their duplicates
    c = filter_case(420, [3001, 257, 1025], [300, 257, 40])
    out = run_filter(c, 4096)
    check_filter(c, out, 4096)
    again = run_filter(c, 4096)
    assert all((out[k] == again[k]).all() for k in out)  # two runs: identical bits, sentinels included


def test_filter_full_table_overflow_and_table_size():
    # list 0: exactly 64 distinct voxels in a table of 64; list 1: 65 (no NaN rows here: the counts are exact)
    rng = np.random.default_rng(5)
    c = filter_case(500, [200, 200], [64, 65], segments=False)
    c["xyz"][0], c["xyz"][1] = grid_points(rng, 200, 64), grid_points(rng, 200, 65)
    assert len(np.unique(V.voxel_keys(0.05, c["xyz"][0]))) == 64 and len(np.unique(V.voxel_keys(0.05, c["xyz"][1]))) == 65
    out = run_filter(c, 64)  # (every buffer a sentinel-filled tensor: check_filter reads what lies behind the written part)
    assert out["overflow"][0] == 0 and out["overflow"][1] != 0 and out["counts"][0] == 64
    check_filter(c, out, 64, lists=[0])
    assert out["counts"][1] <= 200 and (out["index"][1].view(np.uint32)[out["counts"][1]:] == SENTINEL).all()
    big = run_filter(c, 4096)
    check_filter(c, big, 4096)
    for name in ("index", "xyz", "pixel", "gray", "normals"):
        assert (out[name][0] == big[name][0]).all()
    # the workspace inside guards: nothing is written outside the bytes vors_voxel_filter_workspace_bytes states
    import torch
    need = V.voxel_filter_workspace_bytes(2, 200, 64)
    ws = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    V.voxel_filter_points(dev(c["xyz"]), dev(c["list_counts"]), 0.05, 64, workspace=ws[256:256 + need])
    torch.cuda.synchronize()
    assert (ws[:256] == 0xA5).all() and (ws[256 + need:] == 0xA5).all()


# ------------------------------------------------------------------------------------------------------------ the trackers' map
N_FRAMES, ROWS, COLS, LEVELS = 8, 120, 160, 4
SPEEDS = [4.0, 9.0, 6.0]
BASE = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001])
CAPACITY, MAX_KF, VOXEL_M, SLOTS = ROWS * COLS * N_FRAMES, 16, 0.02, 1 << 18


@functools.lru_cache(maxsize=None)
def tracked(voxels):
    """A handle over the three sequences after 8 frames: the map at level 0 with normals, and the voxel filter when asked."""
    import torch
    intr = V.scaled_intrinsics(ROWS, COLS)
    cfg = V.Config(nb_levels=LEVELS, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=V.CANDIDATES_DENSE, arithmetic=V.ARITH_FUSED)
    seeds = [1000, 1002, 1004]
    tr = V.Trackers(cfg, 3, ROWS, COLS)
    tr.enable_map(0, CAPACITY, MAX_KF)
    if voxels:
        tr.enable_map_voxels(VOXEL_M, SLOTS)
    tr.enable_map_normals(1, 0.05)
    for k in range(N_FRAMES):
        frame = V.synth_render_frames(seeds, [k] * 3, [BASE * s * k for s in SPEEDS], ROWS, COLS, intr, invalid_percent=2)
        (tr.init if k == 0 else tr.track)(*frame)
    torch.cuda.synchronize()
    return tr


def test_filter_equals_the_trackers_filtered_map():
    import torch
    plain, filtered = tracked(False).map(), tracked(True).map()
    want_normals = tracked(True).map_normals()
    n_seg = host(plain["n_segments"])
    assert (n_seg >= 3).all() and (n_seg <= MAX_KF).all() and (host(plain["counts"]) <= CAPACITY).all()  # promotions; nothing clipped
    assert (host(tracked(True).map_voxels()["overflow"]) == 0).all()
    out = V.voxel_filter_points(plain["xyz"], plain["counts"], VOXEL_M, SLOTS, pixel=plain["pixel"], gray=plain["gray"],
                                normals=tracked(False).map_normals(), segments=plain["segments"], n_segments=plain["n_segments"])
    torch.cuda.synchronize()
    counts = host(out["counts"])
    assert (counts == host(filtered["counts"])).all() and (host(out["overflow"]) == 0).all()
    got_seg, want_seg = host(out["segments"], SEG), host(filtered["segments"], SEG)
    for i in range(3):
        k = counts[i]
        assert 0 < k < host(plain["counts"])[i]
        for name, want in (("xyz", filtered["xyz"]), ("pixel", filtered["pixel"]), ("gray", filtered["gray"]), ("normals", want_normals)):
            assert torch.equal(out[name][i, :k].view(torch.uint8), want[i, :k].view(torch.uint8)), (i, name)
        assert got_seg[i, :n_seg[i]].tobytes() == want_seg[i, :n_seg[i]].tobytes()


def test_through_the_handle():
    import torch
    tr = tracked(False)
    before = {k: v.clone() for k, v in tr.map().items()}
    normals_before = tr.map_normals()
    seg = host(before["segments"], SEG)
    n_seg, counts = host(before["n_segments"]), host(before["counts"])
    node_counts = dev(n_seg.astype(np.uint32))
    # the handle's own poses: its lists, bit for bit
    own = tr.repose_map(dev(np.ascontiguousarray(seg["pose7"])), node_counts)
    torch.cuda.synchronize()
    for i in range(3):
        assert torch.equal(own["xyz"][i, :counts[i]].view(torch.int32), before["xyz"][i, :counts[i]].view(torch.int32))
        assert torch.equal(own["normals"][i, :counts[i]].view(torch.int32), normals_before[i, :counts[i]].view(torch.int32))
    assert host(own["counts"])[:, [0, 4, 5]].sum() == 0 and (host(own["counts"])[:, 1] + host(own["counts"])[:, 2] == counts).all()
    assert torch.equal(own["segments"], before["segments"])
    # B_k = G * A_k for one rigid G, composed on the host with iso_mul: equals repose_points on the handle's pointers
    g = np.array([0.3, -0.2, 0.1, 0.0, np.sin(0.05), 0.0, np.cos(0.05)], F)
    b = np.zeros((3, MAX_KF, 7), F)
    for i in range(3):
        for k in range(n_seg[i]):
            V.lib().vors_iso_mul(V._ptr(g), V._ptr(np.ascontiguousarray(seg["pose7"][i, k])), V._ptr(b[i, k]))
    views = tr.map(copy=False)
    moved = tr.repose_map(dev(b), node_counts)
    free = V.repose_points(views["xyz"], views["counts"], views["segments"], views["n_segments"], dev(b), node_counts,
                           normals=tr.map_normals(copy=False))
    torch.cuda.synchronize()
    for name in ("xyz", "normals"):
        for i in range(3):
            assert torch.equal(moved[name][i, :counts[i]].view(torch.int32), free[name][i, :counts[i]].view(torch.int32)), name
    assert torch.equal(moved["counts"], free["counts"]) and (host(moved["counts"])[:, 4] == n_seg).all() and (host(moved["counts"])[:, 0] > 0).all()
    for i in range(3):
        assert torch.equal(moved["segments"][i, :n_seg[i]], free["segments"][i, :n_seg[i]])
        assert host(moved["segments"], SEG)[i, :n_seg[i]]["pose7"].tobytes() == b[i, :n_seg[i]].tobytes()
    # the handle's map has not changed a bit
    after = tr.map()
    assert all(torch.equal(after[k], before[k]) for k in before) and torch.equal(tr.map_normals(), normals_before)
