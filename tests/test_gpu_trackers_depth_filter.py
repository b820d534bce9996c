"""The recursive depth filter of the lock-step trackers (vors_trackers_enable_depth_filter, vors_trackers_keyframe_depth,
vors_tracker_enable_depth_filter): at a promotion the new keyframe is built on the depth fused from the old keyframe and the
measurement (vors_batch_fuse_depth's pass as masked launches), and a sequence that does not promote keeps its planes. GPU only.

  1. shadow fusion: every promoted plane equals a separate Batch's fuse_depth on (old keyframe, final model, measurement, old weight), bit for bit
  2. replay: a plain Trackers fed the recorded fused planes at the promotions reproduces poses, statuses, keyframes and stats bit for bit
  3. Tracker(depth_filter=...) on host buffers == sequence 0 of an N = 1 filtered Trackers
  4. it filters: RMS error of the fused depth below the measurement's at the pixels of weight >= 3
  5. independence of the other sequences and of the stream; two runs are bitwise equal
  6. contracts   7. hostile scenes, no faults
"""
import functools
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V

BLOCKY = 1 << 63
N_SEQ, N_FRAMES = 6, 10
# Twist per frame = BASE * SPEED[s]. Chosen with the oracle's tracker on the CPU (an unfiltered run): in every mode sequences 0 and 5
# promote, sequence 1 never does, at least one promotes every other frame, and most frames promote some sequences but not all.
BASE = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001])
SPEED = np.array([4.0, 0.05, 9.0, 2.0, 6.0, 5.0])
TOL_M, MAX_W, FILL = 0.02, 255, 1
SHAPES = {V.CANDIDATES_DENSE: (60, 80, 3), V.CANDIDATES_COARSE_TO_FINE: (96, 128, 4), V.CANDIDATES_DSO: (96, 128, 4)}
MODES = pytest.mark.parametrize("mode", [V.CANDIDATES_DENSE, V.CANDIDATES_COARSE_TO_FINE, V.CANDIDATES_DSO], ids=["dense", "coarse_to_fine", "dso"])
ARITHS = pytest.mark.parametrize("arith", [V.ARITH_REFERENCE, V.ARITH_FUSED], ids=["reference", "fused"])


def config(mode, arith, intr=None):
    rows, cols, L = SHAPES[mode]
    intr = intr or V.scaled_intrinsics(rows, cols)
    return V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, arithmetic=arith)


@functools.lru_cache(maxsize=None)
def frames_of(mode):
    """[N_FRAMES] of (gray [N_SEQ, rows, cols] u8, depth int16 holding u16) on the device: 2 % of the depth pixels are 0."""
    import torch
    rows, cols, _ = SHAPES[mode]
    intr = V.scaled_intrinsics(rows, cols)
    out = [V.synth_render_frames([(BLOCKY if mode == V.CANDIDATES_DSO else 0) | (1000 + s) for s in range(N_SEQ)], [k] * N_SEQ,
                                 [BASE * SPEED[s] * k for s in range(N_SEQ)], rows, cols, intr, invalid_percent=2) for k in range(N_FRAMES)]
    torch.cuda.synchronize()
    return out


def run(cfg, frames, rows, cols, depth_filter=(TOL_M, MAX_W, FILL), seqs=None):
    """A Trackers run over `frames` (of the sequences `seqs`) -> per frame k = 0 .. F-1 a dict of host arrays: poses, status, kf, stats (k >= 1),
    and with a filter depth, weight. The planes are read back after every frame."""
    sel = (lambda t: t) if seqs is None else (lambda t: t[seqs].contiguous())
    n = N_SEQ if seqs is None else len(seqs)
    tr = V.Trackers(cfg, n, rows, cols)
    if depth_filter is not None:
        tr.enable_depth_filter(*depth_filter)
    rec = []
    for k, (g, d) in enumerate(frames):
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
    return rec


@functools.lru_cache(maxsize=None)
def filtered_run(mode, arith):
    rows, cols, _ = SHAPES[mode]
    return run(config(mode, arith), frames_of(mode), rows, cols)


def promotions(rec):
    """[F-1, n] bool: sequence s promoted at frame k (the keyframe index moved)."""
    return np.stack([rec[k]["kf"] != rec[k - 1]["kf"] for k in range(1, len(rec))])


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------ the inputs reach the cases
@MODES
@ARITHS
def test_inputs_reach_the_cases(mode, arith):
    rec, frames = filtered_run(mode, arith), frames_of(mode)
    p = promotions(rec)
    per_frame = p.sum(axis=1)
    assert ((per_frame > 0) & (per_frame < N_SEQ)).any(), "no frame on which some but not all sequences promote"
    assert (p.sum(axis=0) >= 3).any(), "no sequence promotes three times"
    assert (p.sum(axis=0) == 0).any(), "every sequence promotes"
    assert p[:, 0].any() and p[:, N_SEQ - 1].any(), "the first and the last sequence must promote"
    zeros = np.mean([(d.cpu().numpy() == 0).mean() for _, d in frames])
    assert 0.01 < zeros < 0.03, f"{zeros:.4f} of the measured depth is 0"
    assert max(r["weight"].max() for r in rec) >= 3, "no weight of 3 anywhere"
    assert all((r["status"] == 0).all() for r in rec)
    # init: the measured depth, weight 1 where it is non-zero
    d0 = frames[0][1].cpu().numpy().view(np.uint16)
    assert same_bits(rec[0]["depth"], d0) and same_bits(rec[0]["weight"], (d0 != 0).astype(np.uint8))


# ------------------------------------------------------------------------------------------------------------ 1
@MODES
@ARITHS
def test_shadow_fusion_bit_for_bit(mode, arith):
    import torch
    rows, cols, _ = SHAPES[mode]
    rec, frames = filtered_run(mode, arith), frames_of(mode)
    shadow = V.Batch(config(mode, arith), N_SEQ, rows, cols)
    counts = np.zeros(6, np.int64)
    for k in range(1, N_FRAMES):
        before, after = rec[k - 1], rec[k]
        promoted = np.nonzero(after["kf"] != before["kf"])[0]
        kept = np.nonzero(after["kf"] == before["kf"])[0]
        assert (after["stats"]["change_keyframe"][promoted] == 1).all() and (after["stats"]["change_keyframe"][kept] == 0).all()
        for s in kept:
            assert same_bits(after["depth"][s], before["depth"][s]) and same_bits(after["weight"][s], before["weight"][s]), f"frame {k} sequence {s} moved"
        if len(promoted) == 0:
            continue
        kf_gray = torch.stack([frames[before["kf"][s]][0][s] for s in promoted]).contiguous()
        kf_depth = torch.from_numpy(before["depth"][promoted].view(np.int16)).cuda()
        kf_weight = torch.from_numpy(before["weight"][promoted]).cuda()
        models = torch.from_numpy(np.ascontiguousarray(after["stats"]["lm_model"][promoted])).cuda()
        shadow.prepare_keyframes(kf_gray, kf_depth)
        m = shadow.fuse_depth(models, frames[k][1][promoted].contiguous(), TOL_M, kf_weight=kf_weight, max_weight=MAX_W, fill_min_weight=FILL, counts=True)
        torch.cuda.synchronize()
        assert same_bits(m["depth"].cpu().numpy().view(np.uint16), after["depth"][promoted]), f"frame {k}: fused depth differs from the shadow batch"
        assert same_bits(m["weight"].cpu().numpy(), after["weight"][promoted]), f"frame {k}: fused weight differs from the shadow batch"
        counts += m["counts"].cpu().numpy().sum(axis=0)
    assert counts[0] > 0 and counts[3] > 0 and counts[4] > 0 and counts[5] > 0, f"agree / measured only / filled / empty must all occur: {counts}"


# ------------------------------------------------------------------------------------------------------------ 2
@MODES
@ARITHS
def test_replay_with_the_recorded_planes(mode, arith):
    import torch
    rows, cols, _ = SHAPES[mode]
    rec, frames = filtered_run(mode, arith), frames_of(mode)
    p = promotions(rec)
    replay = []
    for k, (g, d) in enumerate(frames):
        if k >= 1 and p[k - 1].any():
            d = d.clone()
            for s in np.nonzero(p[k - 1])[0]:
                d[s] = torch.from_numpy(rec[k]["depth"][s].view(np.int16)).cuda()
        replay.append((g, d))
    plain = run(config(mode, arith), replay, rows, cols, depth_filter=None)
    differs_from_measured = False
    for k in range(N_FRAMES):
        for name in ("poses", "status", "kf") + (("stats",) if k else ()):
            assert same_bits(plain[k][name], rec[k][name]), f"frame {k}: {name} of the replay differ"
        differs_from_measured |= k >= 1 and not same_bits(replay[k][1].cpu().numpy(), frames[k][1].cpu().numpy())
    assert differs_from_measured   # (the replay was fed something the sensor did not measure)


# ------------------------------------------------------------------------------------------------------------ 3
@MODES
@ARITHS
def test_single_tracker_equals_one_sequence_handle(mode, arith):
    rows, cols, _ = SHAPES[mode]
    frames, cfg, s = frames_of(mode), config(mode, arith), 4
    many = run(cfg, frames, rows, cols, seqs=[s])
    host = [(g[s].cpu().numpy(), d[s].cpu().numpy().view(np.uint16)) for g, d in frames]
    one = V.Tracker(cfg, 0.0, host[0][1], 0.0, host[0][0], depth_filter=(TOL_M, MAX_W, FILL))
    n_switch = 0
    for k in range(1, N_FRAMES):
        status = one.track(float(k), host[k][1], float(k), host[k][0])
        assert status == many[k]["status"][0], f"frame {k}: status"
        assert same_bits(one.current_frame()[1], many[k]["poses"][0]), f"frame {k}: pose bits differ"
        assert one.keyframe()[0] == float(many[k]["kf"][0]), f"frame {k}: keyframe index"
        n_switch += int(one.last_stats()["change_keyframe"])
    assert n_switch >= 3
    with pytest.raises(V.VorsError, match="before the first"):   # the switch is legal until the first track only
        V._check(V.lib().vors_tracker_enable_depth_filter(one._h, TOL_M, MAX_W, FILL))


# ------------------------------------------------------------------------------------------------------------ 4
def test_it_filters():
    """Fronto-parallel textured plane under lateral translation, dense mode; measured depth = truth + N(0, 20 depth units), rounded.
    Independent noise averaged over three measurements would give 1 / sqrt(3) = 0.58 of the measurement's RMS error; the condition is < 1.

    Where the plane stands. A prediction is the old depth carried through the tracked model, so it also carries the model's error: a
    rotation error theta about the vertical axis moves a point at lateral offset X by X theta along the optical axis. On this geometry
    lateral translation and that rotation are nearly indistinguishable at 80x60, and the ORACLE's tracker (CPU, no filter anywhere) is off
    by up to 0.0086 rad (quaternion y 0.0043) over one keyframe interval, whatever the distance of the plane when the images are kept the
    same. X reaches 0.6 Z0 at the image border, so the carried error is up to 0.6 Z0 x 0.0086 x 5000 = 26 Z0 depth units (Z0 in metres)
    against a sensor noise the issue fixes at 20 units: at 2 m it is 52 units at the border and buries the noise the filter is to
    average (measured there on an MI355X: RMS fused 20.48 against 19.94 measured, ratio 1.027; the planes were the bits of
    vors_batch_fuse_depth all the same, test_shadow_fusion_bit_for_bit). The test is about the filter, not about the conditioning of this
    scene, so the plane stands at 0.5 m, where the model carries at most 13 units at the border, 13 / sqrt(3) = 7.5 RMS over the image: well
    below the 20 of the noise. Step and texture are scaled with the distance, which keeps the images what they were."""
    import torch
    mode = V.CANDIDATES_DENSE
    rows, cols, _ = SHAPES[mode]
    cu, cv, fu, fv, _ = intr = V.scaled_intrinsics(rows, cols)
    # the keyframe test reads the flow at the coarsest level, where 1 px = 4 Z0 / fu = 0.031 m: a promotion every third frame (the oracle's
    # tracker on the unfiltered sequence promotes at frames 3, 6, 9 and 12)
    Z0, sigma, n_frames, step = 0.5, 20.0, 13, 0.0125
    truth = np.full((rows, cols), Z0 * V.DEPTH_SCALE, np.float64)
    rng = np.random.default_rng(20)
    waves = [(rng.uniform(32.0, 160.0), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi), rng.uniform(10.0, 25.0)) for _ in range(12)]
    y, x = np.mgrid[0:rows, 0:cols]
    frames, noisy = [], []
    for k in range(n_frames):
        p, q = (x - cu) / fu * Z0 + step * k, (y - cv) / fv * Z0   # the plane point a pixel sees from a camera at (step k, 0, 0)
        tex = 128.0 + sum(a * np.sin(f * (np.cos(th) * p + np.sin(th) * q) + ph) for f, th, ph, a in waves)
        gray = np.clip(np.floor(tex + 0.5), 0, 255).astype(np.uint8)
        depth = np.clip(np.round(truth + rng.normal(0.0, sigma, truth.shape)), 1, 65535).astype(np.uint16)
        noisy.append(depth)
        frames.append((torch.from_numpy(gray[None]).cuda(), torch.from_numpy(depth.view(np.int16)[None]).cuda()))
    tol_m = 12 * sigma / V.DEPTH_SCALE   # 12 sigma, in metres: well above 3 sigma
    tr = V.Trackers(config(mode, V.ARITH_FUSED, intr), 1, rows, cols)
    tr.enable_depth_filter(tol_m)
    tr.init(*frames[0])
    last_kf = 0
    for k in range(1, n_frames):
        tr.track(*frames[k])
        last_kf = int(tr.current_frames()[2][0])
    depth, weight = (t.cpu().numpy()[0] for t in tr.keyframe_depth())
    depth = depth.view(np.uint16)
    sel = weight >= 3
    assert last_kf >= 3 and sel.any() and sel.mean() > 0.25, f"last keyframe {last_kf}, weight >= 3 on {sel.mean():.3f} of the image"
    rms = lambda a: float(np.sqrt(np.mean((a[sel].astype(np.float64) - truth[sel]) ** 2)))
    rms_fused, rms_measured = rms(depth), rms(noisy[last_kf])
    print(f"depth filter: keyframe {last_kf}, weight >= 3 on {sel.mean():.3f} of the image, RMS fused {rms_fused:.2f} / measured {rms_measured:.2f} "
          f"= {rms_fused / rms_measured:.3f} (independent noise, three measurements: 0.577)")
    assert rms_fused < rms_measured


# ------------------------------------------------------------------------------------------------------------ 5
@MODES
def test_independent_of_the_other_sequences_and_of_the_stream(mode):
    import torch
    arith = V.ARITH_FUSED
    rows, cols, _ = SHAPES[mode]
    rec, frames, cfg = filtered_run(mode, arith), frames_of(mode), config(mode, arith)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for s, stream in ((0, None), (N_SEQ - 1, side)):
        if stream is None:
            alone = run(cfg, frames, rows, cols, seqs=[s])
        else:
            with torch.cuda.stream(stream):
                alone = run(cfg, frames, rows, cols, seqs=[s])
        for k in range(N_FRAMES):
            for name in ("poses", "status", "kf", "depth", "weight"):
                assert same_bits(alone[k][name][0], rec[k][name][s]), f"sequence {s} frame {k}: {name} depend on the company"
    again = run(cfg, frames, rows, cols)
    for k in range(N_FRAMES):
        for name in ("poses", "status", "kf", "depth", "weight"):
            assert same_bits(again[k][name], rec[k][name]), f"frame {k}: {name} differ between two identical runs"


# ------------------------------------------------------------------------------------------------------------ 6
def test_contracts():
    import torch
    mode = V.CANDIDATES_COARSE_TO_FINE
    rows, cols, _ = SHAPES[mode]
    cfg, frames = config(mode, V.ARITH_FUSED), frames_of(mode)
    plain, batch = V.Trackers(cfg, N_SEQ, rows, cols), V.Batch(cfg, N_SEQ, rows, cols)
    assert plain.workspace_bytes() == batch.workspace_bytes()   # a handle that never enables the filter pays nothing
    with pytest.raises(V.VorsError, match="not enabled"):
        plain.keyframe_depth()
    t = V.Trackers(cfg, N_SEQ, rows, cols)
    before = t.workspace_bytes()
    for bad, word in (((-1e-3, 255, 0), "tol_m"), ((float("nan"), 255, 0), "tol_m"), ((0.01, 0, 0), "max_weight"), ((0.01, 256, 0), "max_weight"),
                      ((0.01, 255, -1), "fill_min_weight"), ((0.01, 255, 256), "fill_min_weight")):
        with pytest.raises(V.VorsError, match=word):
            t.enable_depth_filter(*bad)
    assert t.workspace_bytes() == before   # a refused call allocates nothing
    t.enable_depth_filter(TOL_M)
    enabled = t.workspace_bytes()
    assert enabled == before + N_SEQ * rows * cols * (8 + 2 + 1 + 1)   # key plane, depth, weight, staged weight
    with pytest.raises(V.VorsError, match="already"):
        t.enable_depth_filter(TOL_M)
    t.init(*frames[0])
    for k in range(1, 4):
        t.track(*frames[k])
    t.keyframe_depth()
    assert t.workspace_bytes() == enabled   # no later call allocates
    plain.init(*frames[0])
    with pytest.raises(V.VorsError, match="before vors_trackers_init"):
        plain.enable_depth_filter(TOL_M)
    plain.track(*frames[1])
    torch.cuda.synchronize()
    assert plain.workspace_bytes() == batch.workspace_bytes()
    lib = V.lib()
    assert lib.vors_trackers_enable_depth_filter(None, 0.01, 255, 0) == -1 and lib.vors_trackers_keyframe_depth(None, None, None) == -1
    assert lib.vors_trackers_keyframe_depth(t._h, None, None) == 0   # either output may be NULL


# ------------------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("name", sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "adversarial", "*.npz"))))
def test_hostile_scenes(name):
    import torch
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "adversarial", name + ".npz"))
    L, mode, rows, cols, intr = int(g["L"]), int(g["mode"]), int(g["rows"]), int(g["cols"]), tuple(float(x) for x in g["intr"])
    kg, cg = (torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("kf_gray", "cur_gray"))
    kd = torch.from_numpy(np.ascontiguousarray(g["kf_depth"]).view(np.int16)).cuda()   # (stands in for the current depth as well)
    n = kg.shape[0]
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, huber_delta=float(g["huber"]),
                   arithmetic=V.ARITH_FUSED)
    out = []
    for filtered in (True, False):
        tr = V.Trackers(cfg, n, rows, cols)   # every pair of the scene is one two-frame sequence
        if filtered:
            tr.enable_depth_filter(TOL_M, MAX_W, FILL)
        tr.init(kg, kd)
        tr.track(cg, kd)
        out.append(tr.current_frames())
        if filtered:
            depth, weight = (t.cpu().numpy() for t in tr.keyframe_depth())
            assert ((depth == 0) == (weight == 0)).all(), "depth 0 and weight 0 must coincide"
    assert (out[0][1] == out[1][1]).all(), "statuses of the first frame must not depend on the filter"
    assert same_bits(out[0][0], out[1][0]) and (out[0][2] == out[1][2]).all()   # (nor do its poses: no fused map has been used yet)
