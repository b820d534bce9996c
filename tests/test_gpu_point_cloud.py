"""Point clouds of a prepared batch (vors_batch_point_cloud): ordered, deterministic stream compaction of a level's usable points,
back-projected and carried to the world frame. GPU only.

  1. against the oracle (levels 0 and L - 1): the pixels are oracle.Tracker's points, the counts are equal, the grey levels are the oracle's level
     image, xyz has the BITS of vors_camera_back_project (one text on host and device) and is within 1e-5 relative of the float64 value;
  2. order: dense = strictly increasing raster index; lists = Batch.points' order;
  3. mask: a random keep = the unmasked result filtered, in order, bit for bit (also from a misaligned mask: the byte path of the quad
     source); an all-zero keep = count 0 and nothing written;
  4. capacity: the count stays the total, the first `capacity` entries are the untruncated run's, nothing is written from `capacity` on;
  5. independence of the batch, the run, the pose stride and the outputs requested; legal before any track_current; tracking afterwards
     gives the bits of tracking without the pass; the workspace grows once, at the first call;
  6. composition with vors_batch_residual_maps; 7. argument checks on a live handle.

Shapes are those tests/test_gpu_residual_maps.py derives (the smallest at which each path can go wrong): 120x160 / 4 levels in the three
candidate modes (dense level 0 = 19200 pixels = two chunks: the cross-chunk base; DSO on the piecewise-constant texture its selector needs),
240x320 / 5 levels coarse-to-fine (4800 slots > 4096: the list is cut), 122x162 / 3 levels dense (the one-pixel source, odd halving).

invalid_percent = 80, so that four pixels in five of a dense level 0 are holes to compact. It is the largest value of 2, 30, 50, 60, 70, 80,
90, 95 at which the oracle's tracker still tracks these scenes on the CPU, by this criterion, fixed beforehand: every pair's status is OK
and the largest pose error against the ground truth is at most 1.5 x that at the default 2 (at 90 the DSO scenes reach 1.7 x). With this seed
the oracle alone gives at least 215 points for every (pair, level) used and 15278 holes in every dense level 0; the tests assert >= 16 and >= 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from oracle import oracle as O
from depth_scales import requantise_tensor

N = 4
SEED = 0x5EEDC10D
BLOCKY = 1 << 63   # seeds with the top bit set render the piecewise-constant texture the DSO selector needs
INVALID_PERCENT = 80
ARITHS = {"reference": V.ARITH_REFERENCE, "fused": V.ARITH_FUSED}
CONFIGS = [((120, 160, 4), m) for m in (0, 1, 2)] + [((240, 320, 5), 0), ((122, 162, 3), 1)]
PARAMS = [(s, m, a) for s, m in CONFIGS for a in ARITHS]
SENT_F, SENT_I, SENT_B = -12345.5, -77, 0xA5
# most chunks a level of the handle is cut into (engine.h eval_pairs_chunks): one integer per pair and chunk is the pass's whole workspace
WS_CHUNKS = {(120, 160, 0): 1, (120, 160, 1): 2, (120, 160, 2): 2, (240, 320, 0): 2, (122, 162, 1): 2}
_oracle_cache = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def quat_to_mat(q):
    i, j, k, w = (float(v) for v in q)
    return np.array([[1 - 2 * (j * j + k * k), 2 * (i * j - k * w), 2 * (i * k + j * w)],
                     [2 * (i * j + k * w), 1 - 2 * (i * i + k * k), 2 * (j * k - i * w)],
                     [2 * (i * k - j * w), 2 * (j * k + i * w), 1 - 2 * (i * i + j * j)]])


def world_poses():
    """One camera -> world pose per pair: 0.4 rad about a random axis, 1 m away (unit quaternions up to float32 rounding)."""
    rng = np.random.default_rng(5)
    out = np.empty((N, 7), np.float32)
    for p in range(N):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        t = rng.normal(size=3)
        out[p, :3] = t / np.linalg.norm(t)
        out[p, 3:6] = np.sin(0.2) * axis
        out[p, 6] = np.cos(0.2)
    return out


def sentinels(n, cap, pad=0, dev="cuda"):
    import torch
    return dict(xyz=torch.full((n * cap * 3 + pad,), SENT_F, dtype=torch.float32, device=dev),
                pixel=torch.full((n * cap + pad,), SENT_I, dtype=torch.int32, device=dev),
                gray=torch.full((n * cap + pad,), SENT_B, dtype=torch.uint8, device=dev),
                counts=torch.full((n + pad,), SENT_I, dtype=torch.int32, device=dev))


class Scene:
    """4 rendered pairs on a handle that has only prepared its keyframes; the full clouds of levels 0 and L - 1 are read back once.
    scale, idepth_variance: the handle's; the rendered depth maps (quantised at V.DEPTH_SCALE) are re-quantised at another scale."""

    def __init__(self, shape, mode, arith, scale=V.DEPTH_SCALE, idepth_variance=1e-4):
        import torch
        self.rows, self.cols, self.L = shape
        self.mode, self.arith = mode, ARITHS[arith]
        self.scale, self.idepth_variance = scale, idepth_variance
        self.intr = V.scaled_intrinsics(self.rows, self.cols)
        seed = SEED | (BLOCKY if mode == V.CANDIDATES_DSO else 0)
        self.kg, self.kd, self.cg, _, _ = V.synth_render_pairs(seed, N, self.rows, self.cols, self.intr, invalid_percent=INVALID_PERCENT)
        if scale != V.DEPTH_SCALE:
            self.kd = requantise_tensor(self.kd, scale)
        self.cfg = V.Config(nb_levels=self.L, intrinsics=V.Intrinsics(self.intr[:2], self.intr[2:4], self.intr[4]), candidates_mode=mode,
                            depth_scale=scale, idepth_variance=idepth_variance, arithmetic=self.arith)
        self.b = V.Batch(self.cfg, N, self.rows, self.cols)
        self.b.prepare_keyframes(self.kg, self.kd)
        self.poses = world_poses()
        self.d_poses = torch.from_numpy(self.poses).cuda()
        self.ws_before = self.b.workspace_bytes()
        self.levels = (0, self.L - 1)
        self.full = {lvl: self.run(lvl) for lvl in self.levels}   # the first calls on the handle: before any track_current
        self.ws_after_first = self.b.workspace_bytes()
        self.stats = None

    def shape(self, lvl):
        return self.rows >> lvl, self.cols >> lvl

    def run(self, lvl, **kw):
        """Batch.point_cloud with every output unless told otherwise -> dict of numpy arrays (synchronises)."""
        import torch
        args = dict(poses=self.d_poses, xyz=True, pixel=True, gray=True, counts=True)
        args.update(kw)
        out = self.b.point_cloud(lvl, **args)
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in out.items()}

    def oracle(self):
        """Per pair and level of self.levels: the oracle's points (xy, idepth), level image and level intrinsics. Shared by the handles of a scene."""
        key = (self.rows, self.cols, self.L, self.mode, self.scale, self.idepth_variance)
        if key not in _oracle_cache:
            kg, kd = self.kg.cpu().numpy(), self.kd.cpu().numpy().view(np.uint16)
            per_pair = []
            for p in range(N):
                tr = O.Tracker(O.make_config(self.L, self.intr, depth_scale=self.scale, idepth_variance=self.idepth_variance, candidates_mode=self.mode),
                               0.0, kd[p], 0.0, kg[p])
                per_pair.append({lvl: (tr.points(lvl)[0], tr.points(lvl)[1], tr.image(lvl), tr.level(lvl)[3]) for lvl in self.levels})
            _oracle_cache[key] = per_pair
        return _oracle_cache[key]

    def ensure_tracked(self):
        import torch
        if self.stats is None:
            self.track_poses = torch.zeros((N, 7), dtype=torch.float32, device="cuda")
            self.track_status = torch.zeros(N, dtype=torch.int32, device="cuda")
            self.stats = V.stats_tensor(N)
            self.b.track_current(self.cg, self.track_poses, self.track_status, self.stats)
            torch.cuda.synchronize()
        return self.stats


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: f"{p[0][1]}x{p[0][0]}L{p[0][2]}-{('c2f', 'dense', 'dso')[p[1]]}-{p[2]}")
def scene(request):
    return Scene(*request.param)


def unpack(pix):
    pix = pix.view(np.uint32)
    return (pix & 0xffff).astype(np.int64), (pix >> 16).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ 1
def test_clouds_equal_the_oracle(scene):
    check_clouds_equal_the_oracle(scene)


def check_clouds_equal_the_oracle(sc):
    for p in range(N):
        for lvl in sc.levels:
            rows, cols = sc.shape(lvl)
            xy_o, iz_o, img, k5 = sc.oracle()[p][lvl]
            m = sc.full[lvl]
            cnt = int(m["counts"][p])
            assert len(xy_o) >= 16, ("too few points for the case to mean anything", p, lvl, len(xy_o))
            if sc.mode == V.CANDIDATES_DENSE and lvl == 0:
                assert len(xy_o) < rows * cols, "dense level 0 without a hole: nothing to compact"
            assert cnt == len(xy_o), (p, lvl)
            x, y = unpack(m["pixel"][p, :cnt])
            assert (x < cols).all() and (y < rows).all()
            mine, theirs = np.argsort(y * cols + x, kind="stable"), np.argsort(xy_o[:, 1].astype(np.int64) * cols + xy_o[:, 0], kind="stable")
            assert ((y * cols + x)[mine] == (xy_o[:, 1].astype(np.int64) * cols + xy_o[:, 0])[theirs]).all(), (p, lvl)
            assert (m["gray"][p, :cnt] == img[y, x]).all(), (p, lvl)
            xy_s, iz_s = xy_o[theirs].astype(np.float32), iz_o[theirs]
            host = V.camera_back_project(k5, sc.poses[p], xy_s, np.float32(1.0) / iz_s)
            got = m["xyz"][p, :cnt][mine]
            assert (bits(got) == bits(host)).all(), (p, lvl, int((bits(got) != bits(host)).any(axis=1).sum()))
            # float64, from first principles: camera.rs:135-140 and R P + t
            k = k5.astype(np.float64)
            z = 1.0 / iz_s.astype(np.float64)
            Y = (xy_s[:, 1] - k[1]) * z / k[3]
            X = ((xy_s[:, 0] - k[0]) * z - k[4] * Y) / k[2]
            W = np.stack([X, Y, z], axis=1) @ quat_to_mat(sc.poses[p, 3:]).T + sc.poses[p, :3].astype(np.float64)
            rel = np.linalg.norm(got.astype(np.float64) - W, axis=1) / np.linalg.norm(W, axis=1)
            print(f"pair {p} level {lvl}: {cnt} points of {rows * cols} pixels, max relative |xyz - xyz64| = {rel.max():.3e}")
            assert rel.max() <= 1e-5, (p, lvl)


# ------------------------------------------------------------------------------------------------------------ 2
def test_order_is_the_slot_order_of_the_source(scene):
    sc = scene
    for lvl in sc.levels:
        rows, cols = sc.shape(lvl)
        m = sc.full[lvl]
        for p in range(N):
            cnt = int(m["counts"][p])
            x, y = unpack(m["pixel"][p, :cnt])
            if sc.mode == V.CANDIDATES_DENSE:
                assert (np.diff(y * cols + x) > 0).all(), (p, lvl)
            else:
                xy, _, _, tm = sc.b.points(p, lvl)
                assert len(xy) == cnt and (xy[:, 0] == x).all() and (xy[:, 1] == y).all(), (p, lvl)
                assert (tm == m["gray"][p, :cnt]).all(), (p, lvl)


# ------------------------------------------------------------------------------------------------------------ 3
def filtered(full, p, keep_p):
    cnt = int(full["counts"][p])
    x, y = unpack(full["pixel"][p, :cnt])
    sel = keep_p[y, x] != 0
    return {k: full[k][p, :cnt][sel] for k in ("xyz", "pixel", "gray")}, int(sel.sum())


def test_mask_filters_in_order_bit_for_bit(scene):
    import torch
    sc = scene
    rng = np.random.default_rng(21)
    for lvl in sc.levels:
        rows, cols = sc.shape(lvl)
        full = sc.full[lvl]
        keep = (rng.integers(0, 2, (N, rows, cols)) * rng.integers(1, 256, (N, rows, cols))).astype(np.uint8)   # about half ones, any non-zero byte
        d_keep = torch.from_numpy(keep).cuda()
        shifted = torch.zeros(keep.size + 1, dtype=torch.uint8, device="cuda")   # the same mask one byte off any alignment
        shifted[1:] = d_keep.reshape(-1)
        for name, k in (("aligned", d_keep), ("misaligned", shifted[1:].view(N, rows, cols))):
            m = sc.run(lvl, keep=k)
            for p in range(N):
                want, n_want = filtered(full, p, keep[p])
                assert 0 < n_want < int(full["counts"][p]), "the mask must remove some points and keep some"
                assert int(m["counts"][p]) == n_want, (name, p, lvl)
                assert (bits(m["xyz"][p, :n_want]) == bits(want["xyz"])).all(), (name, p, lvl)
                assert (m["pixel"][p, :n_want] == want["pixel"]).all() and (m["gray"][p, :n_want] == want["gray"]).all(), (name, p, lvl)
        cap = rows * cols
        s = sentinels(N, cap)
        out = sc.b.point_cloud(lvl, poses=sc.d_poses, keep=torch.zeros((N, rows, cols), dtype=torch.uint8, device="cuda"),
                               xyz=s["xyz"].view(N, cap, 3), pixel=s["pixel"].view(N, cap), gray=s["gray"].view(N, cap), counts=s["counts"])
        torch.cuda.synchronize()
        assert (out["counts"].cpu().numpy() == 0).all(), lvl
        assert (s["xyz"] == SENT_F).all() and (s["pixel"] == SENT_I).all() and (s["gray"] == SENT_B).all(), lvl


# ------------------------------------------------------------------------------------------------------------ 4
def test_capacity_truncates_and_writes_nothing_beyond(scene):
    import torch
    sc, lib = scene, V.lib()
    for lvl in sc.levels:
        full = sc.full[lvl]
        counts = full["counts"].astype(np.int64)
        # the untruncated run itself: entries from a pair's count on were never written
        cap_full = sc.shape(lvl)[0] * sc.shape(lvl)[1]
        s = sentinels(N, cap_full)
        sc.b.point_cloud(lvl, poses=sc.d_poses, xyz=s["xyz"].view(N, cap_full, 3), pixel=s["pixel"].view(N, cap_full),
                         gray=s["gray"].view(N, cap_full), counts=s["counts"])
        torch.cuda.synchronize()
        for p in range(N):
            c = int(counts[p])
            assert (s["xyz"].view(N, cap_full, 3)[p, c:] == SENT_F).all() and (s["pixel"].view(N, cap_full)[p, c:] == SENT_I).all()
            assert (s["gray"].view(N, cap_full)[p, c:] == SENT_B).all()
            assert (bits(s["xyz"].view(N, cap_full, 3)[p, :c].cpu().numpy()) == bits(full["xyz"][p, :c])).all()
        for cap in (int(counts.min()) // 2, 1):
            assert 1 <= cap < counts.min()
            pad = 64   # sentinel entries past the last pair's list: an overrun of the last list would land here
            s = sentinels(N, cap, pad)
            st = lib.vors_batch_point_cloud(sc.b._h, N, lvl, sc.b._dp(sc.d_poses), 0, None, cap, sc.b._dp(s["xyz"]), sc.b._dp(s["pixel"]),
                                            sc.b._dp(s["gray"]), sc.b._dp(s["counts"]), sc.b._stream())
            assert st == 0, lib.vors_last_error()
            torch.cuda.synchronize()
            assert (s["counts"][:N].cpu().numpy() == counts).all(), (lvl, cap)
            assert (s["counts"][N:] == SENT_I).all()
            xyz, pix, gray = s["xyz"].cpu().numpy(), s["pixel"].cpu().numpy(), s["gray"].cpu().numpy()
            # every pair has more points than `cap`: each list is full, the next pair's starts right behind it, the pad follows the last
            assert (bits(xyz[:N * cap * 3].reshape(N, cap, 3)) == bits(full["xyz"][:, :cap])).all(), (lvl, cap)
            assert (pix[:N * cap].reshape(N, cap) == full["pixel"][:, :cap]).all() and (gray[:N * cap].reshape(N, cap) == full["gray"][:, :cap]).all()
            assert (xyz[N * cap * 3:] == np.float32(SENT_F)).all() and (pix[N * cap:] == SENT_I).all() and (gray[N * cap:] == SENT_B).all(), (lvl, cap)


# ------------------------------------------------------------------------------------------------------------ 5
def test_results_do_not_depend_on_the_batch_the_run_the_stride_or_the_outputs(scene):
    import torch
    sc, b = scene, scene.b
    item = V.PAIR_STATS_DTYPE.itemsize
    as_stats = np.zeros(N, V.PAIR_STATS_DTYPE)   # the poses in records of sizeof(vors_pair_stats) bytes, lm_model first
    as_stats["lm_model"] = sc.poses
    assert V.PAIR_STATS_DTYPE.fields["lm_model"][1] == 0
    d_stats = torch.from_numpy(np.frombuffer(as_stats.tobytes(), np.uint8).copy()).cuda()
    assert d_stats.numel() == N * item
    for lvl in sc.levels:
        full = sc.full[lvl]
        counts = full["counts"]
        again = sc.run(lvl)
        three = sc.run(lvl, n_pairs=3)
        strided = sc.run(lvl, poses=d_stats)
        subsets = [sc.run(lvl, **kw) for kw in (dict(pixel=False, gray=False), dict(xyz=False, gray=False), dict(xyz=False, pixel=False),
                                                dict(counts=False), dict(xyz=False, pixel=False, gray=False))]
        assert [sorted(s) for s in subsets] == [["counts", "xyz"], ["counts", "pixel"], ["counts", "gray"], ["gray", "pixel", "xyz"], ["counts"]]
        assert three["counts"].shape == (3,) and (three["counts"] == counts[:3]).all()
        for p in range(N):
            c = int(counts[p])
            for run in [again, strided] + subsets + ([three] if p < 3 else []):
                for name in ("xyz", "pixel", "gray"):
                    if name in run:
                        assert (run[name][p, :c].view(np.uint8) == full[name][p, :c].view(np.uint8)).all(), (lvl, p, name)
                if "counts" in run:
                    assert int(run["counts"][p]) == c, (lvl, p)
        # no pose = the camera frame: the bits of the host entry without a pose
        cam = sc.run(lvl, poses=None, n_pairs=N)
        for p in range(N):
            c = int(counts[p])
            xy_o, iz_o, _, k5 = sc.oracle()[p][lvl]
            x, y = unpack(cam["pixel"][p, :c])
            key_o = xy_o[:, 1].astype(np.int64) * 65536 + xy_o[:, 0]
            order = np.argsort(key_o)
            idx = order[np.searchsorted(key_o[order], y * 65536 + x)]
            assert (key_o[idx] == y * 65536 + x).all()
            host = V.camera_back_project(k5, None, np.stack([x, y], axis=1).astype(np.float32), np.float32(1.0) / iz_o[idx])
            assert (bits(cam["xyz"][p, :c]) == bits(host)).all(), (lvl, p)
    # the workspace was created by the first call (the fixture's, before any track_current) and never again
    assert sc.ws_after_first - sc.ws_before == N * WS_CHUNKS[sc.rows, sc.cols, sc.mode] * 4, (sc.ws_before, sc.ws_after_first)
    assert b.workspace_bytes() == sc.ws_after_first
    # tracking after the passes = tracking on a handle that never ran one, bit for bit
    sc.ensure_tracked()
    fresh = V.Batch(sc.cfg, N, sc.rows, sc.cols)
    poses = torch.zeros((N, 7), dtype=torch.float32, device="cuda")
    status = torch.zeros(N, dtype=torch.int32, device="cuda")
    fresh.track_pairs(sc.kg, sc.kd, sc.cg, poses, status)
    torch.cuda.synchronize()
    assert (bits(sc.track_poses.cpu().numpy()) == bits(poses.cpu().numpy())).all()
    assert (sc.track_status.cpu().numpy() == status.cpu().numpy()).all()
    after_track = sc.run(0)
    assert (after_track["counts"] == sc.full[0]["counts"]).all()
    for p in range(N):   # (the entries beyond a pair's count were never written: they are not compared)
        c = int(sc.full[0]["counts"][p])
        assert all((after_track[k][p, :c].view(np.uint8) == sc.full[0][k][p, :c].view(np.uint8)).all() for k in ("xyz", "pixel", "gray")), p
    assert b.workspace_bytes() == sc.ws_after_first


# ------------------------------------------------------------------------------------------------------------ 6
def test_a_mask_from_the_residual_maps_composes(scene):
    import torch
    sc = scene
    stats = sc.ensure_tracked()
    for lvl in sc.levels:
        res = sc.b.residual_maps(lvl, stats, residuals=True)["residuals"]
        keep = (torch.isfinite(res) & (res.abs() <= 20)).to(torch.uint8)
        m = sc.run(lvl, keep=keep)
        keep_h = keep.cpu().numpy()
        for p in range(N):
            c = int(m["counts"][p])
            x, y = unpack(m["pixel"][p, :c])
            assert (keep_h[p][y, x] != 0).all(), (lvl, p)
            assert c == int(keep_h[p].sum()), (lvl, p)   # a finite residual belongs to a usable point


# ------------------------------------------------------------------------------------------------------------ 7
def test_argument_validation_on_a_live_handle():
    import torch
    rows, cols, L = 120, 160, 4
    intr = V.scaled_intrinsics(rows, cols)
    kg, kd, _, _, _ = V.synth_render_pairs(SEED, N, rows, cols, intr, invalid_percent=INVALID_PERCENT)
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), arithmetic=V.ARITH_FUSED)
    b = V.Batch(cfg, 8, rows, cols)
    lib, s = V.lib(), b._stream()
    cap = 64
    o = sentinels(8, cap)

    def call(n=N, lvl=0, capacity=cap, stride=0, stream=s, **kw):
        t = {**o, **kw}
        return lib.vors_batch_point_cloud(b._h, n, lvl, None, stride, None, capacity, b._dp(t["xyz"]), b._dp(t["pixel"]), b._dp(t["gray"]),
                                          b._dp(t["counts"]), stream)

    assert call() == -1 and b"prepare_keyframes" in lib.vors_last_error()
    with pytest.raises(V.VorsError):
        b.point_cloud(0)
    b.prepare_keyframes(kg, kd)
    before = b.workspace_bytes()
    bad = [(dict(xyz=None, pixel=None, gray=None, counts=None), "every output"), (dict(lvl=L), "level"), (dict(lvl=-1), "level"),
           (dict(capacity=-1), "capacity"), (dict(capacity=0), "capacity"), (dict(n=N + 1), "n_pairs"), (dict(n=0), "n_pairs"),
           (dict(stride=30), "stride"), (dict(stride=24), "stride")]
    if torch.cuda.device_count() >= 2:
        other = torch.cuda.Stream(device=1)
        bad.append((dict(stream=V.C.c_void_p(other.cuda_stream)), "stream"))
    for kw, word in bad:
        assert call(**kw) == -1, kw
        assert word.encode() in lib.vors_last_error(), (kw, lib.vors_last_error())
    torch.cuda.synchronize()
    assert b.workspace_bytes() == before   # a refused call enqueues and allocates nothing
    assert (o["xyz"] == SENT_F).all() and (o["pixel"] == SENT_I).all() and (o["gray"] == SENT_B).all() and (o["counts"] == SENT_I).all()
    assert call(xyz=None, pixel=None, gray=None, capacity=0) == 0   # d_counts alone: capacity 0 is legal
    assert call() == 0
    torch.cuda.synchronize()
    assert (o["counts"][:N] > cap).all() and (o["counts"][N:] == SENT_I).all()
    assert (o["pixel"][:N * cap] != SENT_I).all() and (o["pixel"][N * cap:] == SENT_I).all()
    with pytest.raises(V.VorsError):
        b.point_cloud(0, xyz=False, pixel=False, gray=False, counts=False)
    with pytest.raises(V.VorsError):
        b.point_cloud(0, keep=torch.zeros((N, rows, cols), dtype=torch.float32, device="cuda"))
