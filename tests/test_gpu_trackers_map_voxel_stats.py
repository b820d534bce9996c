"""Statistics of the keyframe map's voxels (vors_trackers_enable_map_voxel_stats, vors_trackers_map_voxel_stats,
vors_trackers_map_voxel_means, vors_voxel_means, the vors_tracker_* forms): per rank of the filtered list fixed-point sums of every
observation of its voxel, the sum of their greys, their number and the last segment that saw it; and their resolve into an averaged
list. GPU only; every comparison is on bits unless stated.

  1. the inputs reach the cases     2. device == vors_voxel_stats_host of the UNFILTERED run's list     3. the statistics only read
  4. independence: two runs, company, stream, table_slots, a crowded table     5. clipping by capacity     6. the resolve against its
  host twin, its bound     7. the renderer skips NaN rows     8. Tracker(map_voxel_stats=True) == sequence 0 of an N = 1 handle
  9. overflow: bounded, flagged, tracking untouched

Sequences, shapes, seeds, twists, voxel edges and table_slots are those of tests/test_gpu_trackers_map_voxels.py (its helpers are copied
here): six sequences x ten frames, 120x160 / 4 levels dense with 0.02 m voxels, 96x128 / 4 levels for the two sparse modes with 0.10 m.

Guard words: the statistics are the handle's own arrays, so nothing can be placed behind them. What stands in: a sequence's rows at or
beyond its clipped count must still hold init's zeros, a store past a sequence's rows would land in the next sequence's, which are
compared bit for bit, and the resolve writes caller arrays preset to a sentinel, which must survive at and beyond the clipped count.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V

BLOCKY = 1 << 63
N_SEQ, N_FRAMES = 6, 10
BASE = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001])
SPEED = np.array([4.0, 0.05, 9.0, 2.0, 6.0, 5.0])
FILTER = (0.02, 255, 1)
SHAPES = {V.CANDIDATES_DENSE: (120, 160, 4), V.CANDIDATES_COARSE_TO_FINE: (96, 128, 4), V.CANDIDATES_DSO: (96, 128, 4)}
MODES = pytest.mark.parametrize("mode", [V.CANDIDATES_DENSE, V.CANDIDATES_COARSE_TO_FINE, V.CANDIDATES_DSO], ids=["dense", "coarse_to_fine", "dso"])
ARITHS = pytest.mark.parametrize("arith", [V.ARITH_REFERENCE, V.ARITH_FUSED], ids=["reference", "fused"])
VARIANTS = {"plain": (None, 0), "filter2": (FILTER, 2)}
VARIANT = pytest.mark.parametrize("variant", list(VARIANTS))
MAX_KF = 16
VOXEL_M = {V.CANDIDATES_DENSE: 0.02, V.CANDIDATES_COARSE_TO_FINE: 0.10, V.CANDIDATES_DSO: 0.10}
SLOTS = 65536
NONE = np.uint64(V.VOXEL_NONE)
NAN_BITS = np.uint32(0x7FC00000)


def config(mode, arith):
    rows, cols, L = SHAPES[mode]
    intr = V.scaled_intrinsics(rows, cols)
    return V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, arithmetic=arith)


def large_capacity(mode):
    rows, cols, _ = SHAPES[mode]
    return rows * cols * N_FRAMES


@functools.lru_cache(maxsize=None)
def frames_of(mode):
    import torch
    rows, cols, _ = SHAPES[mode]
    intr = V.scaled_intrinsics(rows, cols)
    out = [V.synth_render_frames([(BLOCKY if mode == V.CANDIDATES_DSO else 0) | (1000 + s) for s in range(N_SEQ)], [k] * N_SEQ,
                                 [BASE * SPEED[s] * k for s in range(N_SEQ)], rows, cols, intr, invalid_percent=2) for k in range(N_FRAMES)]
    torch.cuda.synchronize()
    return out


def read_map(tr, voxels=False, stats=False):
    """Trackers.map() on the host; with `voxels` occupied / overflow, with `stats` sums (int64) and obs (u32) whole."""
    import torch
    m = tr.map()
    v = tr.map_voxels() if voxels else {}
    st = tr.map_voxel_stats() if stats else {}
    torch.cuda.synchronize()
    out = dict(xyz=m["xyz"].cpu().numpy(), pixel=m["pixel"].cpu().numpy().view(np.uint32), gray=m["gray"].cpu().numpy(),
               counts=m["counts"].cpu().numpy().view(np.uint32), n_segments=m["n_segments"].cpu().numpy().view(np.uint32),
               segments=V.decode_map_segments(m["segments"]))
    out.update({k: t.cpu().numpy().view(np.uint32) for k, t in v.items()})
    if stats:
        out["sums"], out["obs"] = st["sums"].cpu().numpy(), st["obs"].cpu().numpy().view(np.uint32)
    return out


def run(cfg, frames, rows, cols, map_args, depth_filter=None, seqs=None, voxels=None, stats=False, n_frames=None, keep=False):
    """A Trackers run -> (per frame a dict of host arrays, the map read after the last frame[, the handle])."""
    sel = (lambda t: t) if seqs is None else (lambda t: t[seqs].contiguous())
    n = N_SEQ if seqs is None else len(seqs)
    tr = V.Trackers(cfg, n, rows, cols)
    if depth_filter is not None:
        tr.enable_depth_filter(*depth_filter)
    tr.enable_map(*map_args)
    if voxels is not None:
        tr.enable_map_voxels(*voxels)
    if stats:
        tr.enable_map_voxel_stats()
    rec = []
    for k, (g, d) in enumerate(frames[:n_frames]):
        g, d = sel(g), sel(d)
        if k == 0:
            tr.init(g, d)
        else:
            tr.track(g, d)
        poses, status, kf = tr.current_frames()
        r = dict(poses=poses, status=status, kf=kf, stats=tr.stats().copy() if k else None)
        if depth_filter is not None:
            dd, ww = tr.keyframe_depth()
            r["depth"], r["weight"] = dd.cpu().numpy().view(np.uint16), ww.cpu().numpy()
        rec.append(r)
    out = rec, read_map(tr, voxels is not None, stats)
    return out + (tr,) if keep else out


@functools.lru_cache(maxsize=None)
def unfiltered_run(mode, arith, variant):
    rows, cols, _ = SHAPES[mode]
    depth_filter, min_weight = VARIANTS[variant]
    return run(config(mode, arith), frames_of(mode), rows, cols, (0, large_capacity(mode), MAX_KF, min_weight), depth_filter)


@functools.lru_cache(maxsize=None)
def voxel_run(mode, arith, variant, stats, voxel_m=None, slots=SLOTS):
    rows, cols, _ = SHAPES[mode]
    depth_filter, min_weight = VARIANTS[variant]
    return run(config(mode, arith), frames_of(mode), rows, cols, (0, large_capacity(mode), MAX_KF, min_weight), depth_filter,
               voxels=(VOXEL_M[mode] if voxel_m is None else voxel_m, slots), stats=stats)


def segment_of(m, s):
    """The segment index of every entry of sequence s's list."""
    out = np.zeros(int(m["counts"][s]), np.uint32)
    for j in range(int(m["n_segments"][s])):
        a = int(m["segments"][s, j]["first"])
        out[a:a + int(m["segments"][s, j]["count"])] = j
    return out


@functools.lru_cache(maxsize=None)
def host_stats(mode, arith, variant, voxel_m=None):
    """vors_voxel_stats_host of every sequence's unfiltered list, at a capacity that clips nothing."""
    _, m = unfiltered_run(mode, arith, variant)
    vm = VOXEL_M[mode] if voxel_m is None else voxel_m
    return [V.voxel_stats_host(m["xyz"][s, :int(m["counts"][s])], m["gray"][s, :int(m["counts"][s])], vm, large_capacity(mode), segment_of(m, s))
            for s in range(N_SEQ)]


def promotions(rec):
    return np.stack([rec[k]["kf"] != rec[k - 1]["kf"] for k in range(1, len(rec))])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def written_stats(m, s, capacity):
    k = min(int(m["counts"][s]), capacity)
    return {name: m[name][s, :k].tobytes() for name in ("xyz", "pixel", "gray", "sums", "obs")}


def check_rows_beyond_are_zero(m, capacity, where):
    for s in range(len(m["counts"])):
        k = min(int(m["counts"][s]), capacity)
        assert not m["sums"][s, k:].any() and not m["obs"][s, k:].any(), f"{where}: sequence {s} has statistics at or beyond rank {k}"


def check_device_equals_host(mode, arith, variant, voxel_m=None, slots=SLOTS):
    (_, u), (_, got), want = unfiltered_run(mode, arith, variant), voxel_run(mode, arith, variant, True, voxel_m, slots), \
        host_stats(mode, arith, variant, voxel_m)
    vm = VOXEL_M[mode] if voxel_m is None else voxel_m
    assert (got["overflow"] == 0).all()
    for s in range(N_SEQ):
        w, k = want[s], want[s]["total"]
        assert got["counts"][s] == k, f"sequence {s}: {got['counts'][s]} ranks against {k}"
        for name in ("xyz", "pixel", "gray"):
            assert same_bits(got[name][s, :k], u[name][s][w["first_index"]]), f"sequence {s}: {name} is not the first-occurrence filter"
        assert same_bits(got["sums"][s, :k], w["sums"]), f"sequence {s}: sums differ from the host twin"
        assert same_bits(got["obs"][s, :k], w["obs"]), f"sequence {s}: obs differ from the host twin"
        keyed = int((V.voxel_keys(vm, u["xyz"][s, :int(u["counts"][s])]) != NONE).sum())
        assert int(got["obs"][s, :k, 0].astype(np.int64).sum()) == keyed, f"sequence {s}: the counts do not add up to the keyed entries of U"
    check_rows_beyond_are_zero(got, large_capacity(mode), "full run")


# ------------------------------------------------------------------------------------------------------------ 1
@MODES
@ARITHS
def test_inputs_reach_the_cases(mode, arith):
    rec, u = unfiltered_run(mode, arith, "plain")
    assert (promotions(rec).sum(axis=0) == 0).any(), "every sequence promotes"
    twice = again = once = False
    for s in range(N_SEQ):
        keys, seg = V.voxel_keys(VOXEL_M[mode], u["xyz"][s, :int(u["counts"][s])]), segment_of(u, s)
        ok = keys != NONE
        uniq, inv, cnt = np.unique(keys[ok], return_inverse=True, return_counts=True)
        once |= bool((cnt == 1).any())
        lo, hi = np.full(len(uniq), 2 ** 31), np.zeros(len(uniq), np.int64)
        np.minimum.at(lo, inv, seg[ok])
        np.maximum.at(hi, inv, seg[ok])
        again |= bool((hi > lo).any())
        pair = np.unique(np.stack([inv, seg[ok].astype(np.int64)]), axis=1, return_counts=True)[1]
        twice |= bool((pair >= 2).any())
    assert twice, "no voxel has two points of one keyframe"
    assert again, "no voxel is seen again by a later keyframe"
    assert once, "no voxel is seen exactly once"


# ------------------------------------------------------------------------------------------------------------ 2
@MODES
@ARITHS
@VARIANT
def test_device_equals_host_bit_for_bit(mode, arith, variant):
    check_device_equals_host(mode, arith, variant)


# ------------------------------------------------------------------------------------------------------------ 3
@MODES
@ARITHS
def test_the_statistics_only_read(mode, arith):
    for variant in VARIANTS:
        (rec, m), (bare, b) = voxel_run(mode, arith, variant, True), voxel_run(mode, arith, variant, False)
        for k in range(N_FRAMES):
            for name in ("poses", "status", "kf") + (("stats",) if k else ()) + (("depth", "weight") if VARIANTS[variant][0] else ()):
                assert same_bits(rec[k][name], bare[k][name]), f"{variant} frame {k}: {name} depend on the statistics"
        for name in ("counts", "n_segments", "occupied", "overflow"):
            assert same_bits(m[name], b[name]), f"{variant}: {name} of the map depends on the statistics"
        for s in range(N_SEQ):   # (the written entries: what lies past the totals is not data)
            k, j = int(b["counts"][s]), int(b["n_segments"][s])
            assert same_bits(m["segments"][s, :j], b["segments"][s, :j]), f"{variant} sequence {s}: the segment records depend on the statistics"
            for name in ("xyz", "pixel", "gray"):
                assert same_bits(m[name][s, :k], b[name][s, :k]), f"{variant} sequence {s}: {name} of the map depends on the statistics"


# ------------------------------------------------------------------------------------------------------------ 4
@MODES
def test_independent_of_the_other_sequences_of_the_stream_and_of_the_run(mode):
    import torch
    arith = V.ARITH_FUSED
    rows, cols, _ = SHAPES[mode]
    (_, m), frames, cfg, cap = voxel_run(mode, arith, "filter2", True), frames_of(mode), config(mode, arith), large_capacity(mode)
    args, vox = (0, cap, MAX_KF, 2), (VOXEL_M[mode], SLOTS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for s, stream in ((0, None), (N_SEQ - 1, side)):
        if stream is None:
            _, alone = run(cfg, frames, rows, cols, args, FILTER, seqs=[s], voxels=vox, stats=True)
        else:
            with torch.cuda.stream(stream):
                _, alone = run(cfg, frames, rows, cols, args, FILTER, seqs=[s], voxels=vox, stats=True)
            stream.synchronize()
        assert alone["counts"][0] == m["counts"][s] > 0
        assert written_stats(alone, 0, cap) == written_stats(m, s, cap), f"sequence {s}: the statistics depend on the company or the stream"
    _, again = run(cfg, frames, rows, cols, args, FILTER, voxels=vox, stats=True)
    assert same_bits(again["sums"], m["sums"]) and same_bits(again["obs"], m["obs"]), "two runs differ"


@MODES
def test_independent_of_table_slots(mode):
    arith = V.ARITH_FUSED
    (_, a), (_, b) = voxel_run(mode, arith, "plain", True, None, 32768), voxel_run(mode, arith, "plain", True)
    assert (a["overflow"] == 0).all() and same_bits(a["counts"], b["counts"])
    assert same_bits(a["sums"], b["sums"]) and same_bits(a["obs"], b["obs"]), "table_slots shows in the statistics"


def test_a_crowded_table():
    """Dense, 0.05 m voxels in 4096 entries (a load of about 0.8): long probe runs, and still the host twin's bits."""
    _, got = voxel_run(V.CANDIDATES_DENSE, V.ARITH_FUSED, "plain", True, 0.05, 4096)
    assert got["occupied"].max() > 2048, "the table was meant to be crowded"
    check_device_equals_host(V.CANDIDATES_DENSE, V.ARITH_FUSED, "plain", 0.05, 4096)


# ------------------------------------------------------------------------------------------------------------ 5
@MODES
def test_clipping(mode):
    arith = V.ARITH_FUSED
    rows, cols, _ = SHAPES[mode]
    rec, full = voxel_run(mode, arith, "plain", True)
    s3 = int(np.argmax(promotions(rec).sum(axis=0)))
    seg = full["segments"][s3]
    cap = int(seg[1]["first"]) + int(seg[1]["count"]) // 2   # strictly inside keyframe 1's filtered segment
    assert seg[1]["first"] < cap < seg[1]["first"] + seg[1]["count"]
    _, clipped = run(config(mode, arith), frames_of(mode), rows, cols, (0, cap, MAX_KF, 0), voxels=(VOXEL_M[mode], SLOTS), stats=True)
    assert same_bits(clipped["counts"], full["counts"]) and clipped["counts"][s3] > cap and (clipped["overflow"] == 0).all()
    assert clipped["sums"].shape == (N_SEQ, cap, 4) and clipped["obs"].shape == (N_SEQ, cap, 2)
    for s in range(N_SEQ):
        k = min(int(full["counts"][s]), cap)
        assert same_bits(clipped["sums"][s, :k], full["sums"][s, :k]) and same_bits(clipped["obs"][s, :k], full["obs"][s, :k]), \
            f"sequence {s}: ranks below a capacity of {cap} differ from the unclipped run's"
    check_rows_beyond_are_zero(clipped, cap, "clipped run")


# ------------------------------------------------------------------------------------------------------------ 6
def first_segment_of_rank(m, s, capacity):
    out = np.zeros(capacity, np.uint32)
    for j in range(min(int(m["n_segments"][s]), MAX_KF)):
        a = int(m["segments"][s, j]["first"])
        out[a:a + int(m["segments"][s, j]["count"])] = j
    return out


@MODES
@ARITHS
def test_resolve_equals_its_host_twin(mode, arith):
    import torch
    rows, cols, _ = SHAPES[mode]
    cap, vm = large_capacity(mode), VOXEL_M[mode]
    _, m, tr = run(config(mode, arith), frames_of(mode), rows, cols, (0, cap, MAX_KF, 0), voxels=(vm, SLOTS), stats=True, keep=True)
    # The bound on mean - f: points of one voxel lie within one edge of each other, so the mean offset is at most voxel_m (1 + a few
    # 2^-24), and the f32 sum f + offset rounds by at most half an ulp of a coordinate, which is below 2^-11 voxel_m while the voxel
    # index |w / voxel_m| stays below 2^13. Asserted of the scenes below.
    dev_map, dev_stats = tr.map(copy=False), tr.map_voxel_stats(copy=False)
    fs = torch.from_numpy(np.stack([first_segment_of_rank(m, s, cap) for s in range(N_SEQ)]).view(np.int32)).cuda()
    rejected = {}
    for min_count, min_span in ((1, 0), (2, 0), (1, 1), (3, 2)):
        sentinel = torch.full((N_SEQ, cap, 3), -7.0, dtype=torch.float32, device="cuda")
        gsent = torch.full((N_SEQ, cap), 201, dtype=torch.uint8, device="cuda")
        own = tr.map_voxel_means(min_count, min_span, xyz_mean=sentinel, gray_mean=gsent)
        free = V.voxel_means(dev_map["xyz"], dev_map["counts"], dev_stats["sums"], dev_stats["obs"], vm, min_count, min_span,
                             first_segment_of_rank=fs)
        torch.cuda.synchronize()
        xm, gm, kept = own["xyz_mean"].cpu().numpy(), own["gray_mean"].cpu().numpy(), own["kept"].cpu().numpy()
        for s in range(N_SEQ):
            k = int(m["counts"][s])
            want = V.voxel_means_host(m["xyz"][s, :k], m["sums"][s, :k], m["obs"][s, :k], vm, min_count, min_span, first_segment_of_rank(m, s, cap)[:k])
            where = f"min_count {min_count} min_span {min_span} sequence {s}"
            assert same_bits(xm[s, :k].view(np.uint32), want["xyz_mean"].view(np.uint32)), f"{where}: centroids differ from the host twin"
            assert same_bits(gm[s, :k], want["gray_mean"]), f"{where}: mean grey differs from the host twin"
            assert same_bits(free["xyz_mean"][s, :k].cpu().numpy().view(np.uint32), want["xyz_mean"].view(np.uint32)), f"{where}: the handle-free pass"
            assert same_bits(free["gray_mean"][s, :k].cpu().numpy(), want["gray_mean"]) and int(free["kept"][s]) == want["kept"]
            finite = np.isfinite(xm[s, :k]).all(axis=1)
            assert (np.isfinite(xm[s, :k]).any(axis=1) == finite).all() and (xm[s, :k][~finite].view(np.uint32) == NAN_BITS).all()
            assert int(kept[s]) == want["kept"] == int(finite.sum()), f"{where}: kept"
            assert (gm[s, :k][~finite] == 0).all()
            assert (xm[s, k:] == -7.0).all() and (gm[s, k:] == 201).all(), f"{where}: the pass wrote at or beyond the clipped count"
            if (min_count, min_span) == (1, 0):
                assert finite.all(), f"{where}: a NaN row below the count"
                assert np.abs(m["xyz"][s, :k].astype(np.float64) / vm).max() < 2.0 ** 13, f"{where}: the scene leaves the range of the bound"
                q = np.abs(m["sums"][s, :k, :3].astype(np.float64) / m["obs"][s, :k, :1].astype(np.float64))
                assert q.max() <= 2.0 ** 20 * (1 + 2.0 ** -10), f"{where}: a mean offset of {q.max()} units"
                d = np.abs(xm[s, :k].astype(np.float64) - m["xyz"][s, :k].astype(np.float64))
                assert d.max() <= vm * (1 + 2.0 ** -10), f"{where}: a centroid {d.max()} m from its first point"
            else:
                a, b = rejected.get((min_count, min_span), (0, 0))
                rejected[(min_count, min_span)] = (a + int((~finite).sum()), b + int(finite.sum()))
    for key, (no, yes) in rejected.items():
        assert no > 0 and yes > 0, f"min_count, min_span {key}: the thresholds were meant to reject some ranks and keep some ({no} / {yes})"


# ------------------------------------------------------------------------------------------------------------ 7
@MODES
def test_the_renderer_skips_nan_rows(mode):
    import torch
    arith = V.ARITH_FUSED
    rows, cols, _ = SHAPES[mode]
    cap, vm = large_capacity(mode), VOXEL_M[mode]
    intr = V.scaled_intrinsics(rows, cols)
    _, m, tr = run(config(mode, arith), frames_of(mode), rows, cols, (0, cap, MAX_KF, 0), voxels=(vm, SLOTS), stats=True, keep=True)
    counts = tr.map(copy=False)["counts"]
    out = {}
    for min_count in (1, 2):
        means = tr.map_voxel_means(min_count, 0)
        r = V.render_points(means["xyz_mean"], means["gray_mean"], counts, intr, rows, cols, V.DEPTH_SCALE, counts=True, zkey=True)
        torch.cuda.synchronize()
        out[min_count] = (means["xyz_mean"].cpu().numpy(), means["gray_mean"].cpu().numpy(), r["counts"].cpu().numpy(),
                          r["zkey"].cpu().numpy().view(np.uint64))
    all_nan = 0
    for s in range(N_SEQ):
        k = int(m["counts"][s])
        nan_rows = int(np.isnan(out[2][0][s, :k, 0]).sum())
        all_nan += nan_rows
        assert out[1][2][s, 0] == out[2][2][s, 0] == k, "considered"
        assert out[1][2][s, 1] == k, "the scene was meant to lie in front of the first camera"
        assert out[2][2][s, 1] == k - nan_rows, f"sequence {s}: in_front {out[2][2][s, 1]} with {nan_rows} NaN rows of {k}"
        host = V.render_points_host(out[2][0][s], out[2][1][s], intr, rows, cols, V.DEPTH_SCALE, count=k)
        assert same_bits(out[2][3][s], host["zkey"]) and (out[2][2][s].view(np.uint32) == host["counts"]).all(), f"sequence {s}: device and host render"
    assert all_nan > 0, "min_count 2 was meant to reject some ranks"


# ------------------------------------------------------------------------------------------------------------ 8
@MODES
@ARITHS
def test_single_tracker_equals_one_sequence_handle(mode, arith):
    rows, cols, _ = SHAPES[mode]
    frames, cfg, s, cap, vox = frames_of(mode), config(mode, arith), 4, large_capacity(mode), (VOXEL_M[mode], SLOTS)
    many, m, tr = run(cfg, frames, rows, cols, (0, cap, MAX_KF, 0), seqs=[s], voxels=vox, stats=True, keep=True)
    host = [(g[s].cpu().numpy(), d[s].cpu().numpy().view(np.uint16)) for g, d in frames]
    one = V.Tracker(cfg, 0.0, host[0][1], 0.0, host[0][0], map=(0, cap, MAX_KF, 0), map_voxels=vox, map_voxel_stats=True)
    first = one.read_map_voxel_stats()   # keyframe 0 was emitted again by the switch: counted once
    assert len(first["obs"]) == m["segments"][0, 0]["count"] and int(first["obs"][:, 0].sum()) >= len(first["obs"]) > 0 and (first["obs"][:, 1] == 0).all()
    for k in range(1, N_FRAMES):
        assert one.track(float(k), host[k][1], float(k), host[k][0]) == many[k]["status"][0]
    total = int(m["counts"][0])
    got = one.read_map_voxel_stats()
    assert same_bits(got["sums"], m["sums"][0, :total]) and same_bits(got["obs"], m["obs"][0, :total])
    assert same_bits(one.read_map()["xyz"], m["xyz"][0, :total])
    for min_count, min_span in ((1, 0), (2, 1)):
        want = tr.map_voxel_means(min_count, min_span)
        mine = one.map_voxel_means(min_count, min_span)
        assert same_bits(mine["xyz_mean"].view(np.uint32), want["xyz_mean"][0, :total].cpu().numpy().view(np.uint32))
        assert same_bits(mine["gray_mean"], want["gray_mean"][0, :total].cpu().numpy()) and mine["kept"] == int(want["kept"][0])
    with pytest.raises(V.VorsError, match="already"):
        V._check(V.lib().vors_tracker_enable_map_voxel_stats(one._h))
    bare = V.Tracker(cfg, 0.0, host[0][1], 0.0, host[0][0], map=(0, cap, MAX_KF, 0), map_voxels=vox)
    with pytest.raises(V.VorsError, match="not enabled"):
        V._check(V.lib().vors_tracker_read_map_voxel_stats(bare._h, 0, None, None))
    bare.track(1.0, host[1][1], 1.0, host[1][0])
    with pytest.raises(V.VorsError, match="before the first"):
        V._check(V.lib().vors_tracker_enable_map_voxel_stats(bare._h))


# ------------------------------------------------------------------------------------------------------------ 9
def test_overflow_is_bounded_and_flagged():
    """Dense, 0.02 m, 64 entries: the init keyframe alone has thousands of voxels. The calls return, every sequence is flagged, tracking is
    bitwise that of the voxels-only run, and no statistics appear at or beyond a sequence's list."""
    import torch
    mode, arith, slots, n_frames = V.CANDIDATES_DENSE, V.ARITH_FUSED, 64, 4
    rows, cols, _ = SHAPES[mode]
    cap = large_capacity(mode)
    rec, m, tr = run(config(mode, arith), frames_of(mode), rows, cols, (0, cap, MAX_KF, 0), voxels=(0.02, slots), stats=True, n_frames=n_frames, keep=True)
    bare, b = run(config(mode, arith), frames_of(mode), rows, cols, (0, cap, MAX_KF, 0), voxels=(0.02, slots), n_frames=n_frames)
    assert (m["overflow"] != 0).all() and (m["occupied"] <= slots).all() and same_bits(m["n_segments"], b["n_segments"])
    for k in range(n_frames):
        for name in ("poses", "status", "kf") + (("stats",) if k else ()):
            assert same_bits(rec[k][name], bare[k][name]), f"frame {k}: {name} depend on the statistics of an overflowing table"
    check_rows_beyond_are_zero(m, cap, "overflowing run")
    means = tr.map_voxel_means(1, 0)   # the resolve of whatever is there returns, too
    torch.cuda.synchronize()
    assert means["kept"].shape == (N_SEQ,)


# ------------------------------------------------------------------------------------------------------------ contracts
def test_contracts():
    import torch
    mode = V.CANDIDATES_DSO
    rows, cols, _ = SHAPES[mode]
    cfg, frames = config(mode, V.ARITH_FUSED), frames_of(mode)
    t = V.Trackers(cfg, N_SEQ, rows, cols)
    cap, slots = 20000, 4096
    t.enable_map(0, cap, 8)
    with pytest.raises(V.VorsError, match="needs the voxel filter"):
        t.enable_map_voxel_stats()
    t.enable_map_voxels(VOXEL_M[mode], slots)
    before = t.workspace_bytes()
    with pytest.raises(V.VorsError, match="not enabled"):
        t.map_voxel_stats()
    with pytest.raises(V.VorsError, match="not enabled"):
        t.map_voxel_means()
    t.enable_map_voxel_stats()
    assert t.workspace_bytes() == before + N_SEQ * (4 * slots + 40 * cap)   # the header's figure
    with pytest.raises(V.VorsError, match="already"):
        t.enable_map_voxel_stats()
    with pytest.raises(V.VorsError, match="before vors_trackers_init"):
        t.map_voxel_means()
    t.init(*frames[0])
    for k in range(1, 3):
        t.track(*frames[k])
    assert t.workspace_bytes() == before + N_SEQ * (4 * slots + 40 * cap)   # no later call allocates
    with pytest.raises(V.VorsError, match="no output"):
        t.map_voxel_means(xyz_mean=False, gray_mean=False, kept=False)
    lib = V.lib()
    other = torch.empty(N_SEQ * 4 + 1, dtype=torch.uint8, device="cuda")
    assert lib.vors_trackers_map_voxel_means(t._h, 1, 0, None, None, other.data_ptr() + 1, None) == -1 and b"aligned" in lib.vors_last_error()
    st = t.map_voxel_stats()
    t.init(*frames[0])   # a second init zeroes the statistics: keyframe 0's again
    again = t.map_voxel_stats()
    torch.cuda.synchronize()
    assert int(again["obs"][..., 0].sum()) < int(st["obs"][..., 0].sum()) and int(again["obs"][..., 1].max()) == 0
    late = V.Trackers(cfg, N_SEQ, rows, cols)
    late.enable_map(0, cap, 8)
    late.enable_map_voxels(VOXEL_M[mode], slots)
    late.init(*frames[0])
    with pytest.raises(V.VorsError, match="before vors_trackers_init"):
        late.enable_map_voxel_stats()
    assert late.workspace_bytes() == before   # a handle that never enables the statistics pays nothing for them
