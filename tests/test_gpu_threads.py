"""include/vors_hip.h on threads: "distinct handles are independent", vors_last_error() is "the last error on the calling thread", and
every entry of a handle "restores the caller's current device". Here distinct handles of every kind — creation and destruction
included — are used from distinct host threads at the same time, and every result must equal, bit for bit, the result of the same work
done by one thread. GPU only.

vors_amd loads the library with ctypes.CDLL (vors_amd.lib()), so every call drops the GIL and the threads' calls really overlap; the
first test pins that, because behind a PyDLL this file would test nothing.

A JOB is a function job(ctx) -> nested dicts / lists of host arrays. It passes ctx.sync() before its first library call and again before
each of its STEPS steps, creates its handles after the first sync, makes every library call through ctx.call(), which then checks that
torch.cuda.current_device() is what it was, and works on the calling thread's current stream. run_serial() runs the jobs one after
another on the default stream (sync is nothing): the expected values. run_threads() runs them in one daemon thread each, on a
torch.cuda.Stream of its own, behind one threading.Barrier. Jobs get different seeds, so a thread that read a neighbour's buffers
would produce other bits. No comparison has a tolerance: same() compares dtype, shape and bytes.

  1. Batch handles of one kind on 4 threads, three candidate modes x {REFERENCE, FUSED}; REFERENCE also against the oracle
  2. 8 threads, modes and arithmetics mixed, two of them on a ragged feed
  3. 4 Trackers handles with depth filter, map, voxels, voxel statistics and map normals; every thread promotes keyframes
  4. 4 single trackers (host buffers), REFERENCE, against the serial run and the oracle's tracker
  5. every kind at once: Batch, Pipeline of depth 3, Trackers with the map ICP correction, a handle-free worker
  6. two threads create, step and destroy handles while two long-lived handles step
  7. the process's first calls from 4 threads at once, in a fresh process, with and without VORS_PYRAMID_FUSED=0
  8. vors_last_error() is per thread     9. the current device is restored (one device: see the test)
 10. two dense FUSED handles of 2048 pairs, which own a side-lane stream    11. vors_lm_solve from eight std::threads

At 8 pairs no dense handle owns a side-lane stream (batch.cpp plan_split: from 2048 pairs, two levels of >= 64 Ki pixels): in cases 1
to 9 the handles with streams of their own are the Trackers (two each) and the Pipeline's slots; case 10 is there for the side lane.
"""
import hashlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "visual-odometry-rs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import vors_amd as V
from oracle import oracle as O

pytestmark = pytest.mark.gpu

BLOCKY = 1 << 63
STEPS = 6
N = 8                                   # pairs per batch, sequences per Trackers handle
SHAPES = [(60, 80, 3), (120, 160, 4)]
JOIN_TIMEOUT_S = 120
MODES = {V.CANDIDATES_COARSE_TO_FINE: "coarse_to_fine", V.CANDIDATES_DENSE: "dense", V.CANDIDATES_DSO: "dso"}
BASE = np.array([0.012, -0.006, 0.004, 0.002, -0.003, 0.001])
SPEED = np.array([4.0, 0.05, 9.0, 2.0, 6.0, 5.0, 7.0, 3.0])   # tests/test_gpu_trackers_map.py's six and two more: most sequences promote
FILTER, NORMALS, VOXEL_M, SLOTS, MAX_KF = (0.02, 255, 1), (2, 0.05), 0.02, 1 << 16, 16
ICP = dict(dist_m=0.05, iters=6, min_cos=0.9, huber_m=0.002, min_match_ratio=0.1, max_rms=0.02, max_trans_m=0.05, max_rot_rad=0.05)


# ------------------------------------------------------------------------------------------------------------ harness
class Ctx:
    """What a job sees of the run it is part of."""

    def __init__(self, barrier=None):
        import torch
        self.barrier = barrier
        self.device = torch.cuda.current_device()
        self.device_checks = 0
        self.inputs = []          # host copies of a job's inputs, kept by the serial run for the oracle

    @property
    def serial(self):
        return self.barrier is None

    def sync(self):
        if self.barrier is not None:
            self.barrier.wait(timeout=JOIN_TIMEOUT_S)

    def call(self, fn, *args, **kwargs):
        import torch
        out = fn(*args, **kwargs)
        assert torch.cuda.current_device() == self.device, f"{getattr(fn, '__name__', fn)} left another current device behind"
        self.device_checks += 1
        return out


def stop_the_session(why):
    pytest.exit(f"{why}: nothing more is started on the GPU", returncode=3)


def run_serial(jobs):
    import torch
    out = []
    for job in jobs:
        ctx = Ctx()
        out.append((job(ctx), ctx))
        torch.cuda.synchronize()
    return out


def run_threads(jobs):
    """One daemon thread per job behind one barrier -> [(result, ctx)]. An exception of a thread is raised here; a thread that does not
    come back within JOIN_TIMEOUT_S is a hang: the session ends."""
    import torch
    assert len(jobs) <= 8, "a command has 16 CPUs: never more than 8 threads"
    barrier = threading.Barrier(len(jobs))
    results, errors = [None] * len(jobs), [None] * len(jobs)

    def body(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                ctx = Ctx(barrier)
                results[i] = (jobs[i](ctx), ctx)
                torch.cuda.current_stream().synchronize()
        except BaseException as e:   # noqa: B036 — handed to the main thread
            errors[i] = e
            barrier.abort()

    threads = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_TIMEOUT_S)
        if t.is_alive():
            stop_the_session(f"a thread of {len(jobs)} did not finish within {JOIN_TIMEOUT_S} s")
    torch.cuda.synchronize()
    first = [e for e in errors if e is not None and not isinstance(e, threading.BrokenBarrierError)] or [e for e in errors if e is not None]
    if first:
        if "illegal memory access" in str(first[0]) or "hipError" in str(first[0]):
            stop_the_session(f"a thread met a HIP error ({first[0]})")
        raise first[0]
    return results


def same(a, b, where="result"):
    """Equality of bits, recursively -> None, or the path of the first difference."""
    if isinstance(a, dict):
        if not isinstance(b, dict) or a.keys() != b.keys():
            return where + ": keys"
        for k in a:
            d = same(a[k], b[k], f"{where}[{k!r}]")
            if d:
                return d
        return None
    if isinstance(a, (list, tuple)):
        if not isinstance(b, (list, tuple)) or len(a) != len(b):
            return where + ": length"
        for k, (x, y) in enumerate(zip(a, b)):
            d = same(x, y, f"{where}[{k}]")
            if d:
                return d
        return None
    if isinstance(a, np.ndarray):
        ok = isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        return None if ok else where
    return None if type(a) is type(b) and a == b else where


def assert_threads_equal_serial(jobs):
    want = run_serial(jobs)
    got = run_threads(jobs)
    for i, ((w, _), (g, ctx)) in enumerate(zip(want, got)):
        d = same(w, g, f"thread {i}")
        assert d is None, f"{d} differs from the serial run"
        assert ctx.device_checks > 0
    return want, got


def host(t):
    """A device tensor on the host, after the calling thread's stream alone (no device-wide synchronisation: the neighbours keep going)."""
    import torch
    torch.cuda.current_stream().synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def config(mode, arith, rows, cols, L):
    intr = O.scaled_intrinsics(rows, cols)
    return V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=mode, arithmetic=arith), intr


def outputs(m):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    return (torch.zeros((m, 7), dtype=torch.float32, device=dev), torch.full((m,), -9, dtype=torch.int32, device=dev), V.stats_tensor(m, device=dev))


def step_result(poses, status, stats):
    """poses, statuses and the whole vors_pair_stats records (lm_model, optical_flow, nb_iter and the rest) as bytes."""
    return dict(poses=host(poses).view(np.uint32), status=host(status), stats=host(stats))


def pairs_of(ctx, seed, mode, m, rows, cols, intr, keep=True):
    kg, kd, cg, _, _ = ctx.call(V.synth_render_pairs, (BLOCKY if mode == V.CANDIDATES_DSO else 0) | seed, m, rows, cols, intr)
    if ctx.serial and keep:
        ctx.inputs.append((host(kg), host(kd), host(cg)))
    return kg, kd, cg


# ------------------------------------------------------------------------------------------------------------ jobs
def batch_job(mode, arith, shape, seed, ragged=False, n=N, steps=STEPS):
    """A V.Batch created behind the barrier, `steps` track_pairs steps on fresh pairs, destroyed at the end."""
    rows, cols, L = shape
    cfg, intr = config(mode, arith, rows, cols, L)

    def job(ctx):
        ctx.sync()
        b = ctx.call(V.Batch, cfg, n, rows, cols)
        out = dict(workspace=[ctx.call(b.workspace_bytes)], steps=[])
        for k in range(steps):
            ctx.sync()
            m = n - 3 * (k % 3) if ragged else n   # tests/test_gpu_pipeline.py's ragged feed
            kg, kd, cg = pairs_of(ctx, seed + 97 * k, mode, m, rows, cols, intr, keep=arith == V.ARITH_REFERENCE)
            poses, status, stats = outputs(m)
            ctx.call(b.track_pairs, kg, kd, cg, poses, status, stats)
            out["steps"].append(step_result(poses, status, stats))
            out["workspace"].append(ctx.call(b.workspace_bytes))
        ctx.call(b.__del__)
        return out
    job.oracle = (mode, arith, shape)
    return job


def pipeline_job(mode, arith, shape, seed, depth=3, ragged=False):
    """A V.Pipeline of `depth` slots: a submit per step, a stream-ordered wait two steps behind, a drain at the end."""
    rows, cols, L = shape
    cfg, intr = config(mode, arith, rows, cols, L)

    def job(ctx):
        ctx.sync()
        pipe = ctx.call(V.Pipeline, cfg, N, rows, cols, depth=depth)
        bufs, tickets = [], []
        for k in range(STEPS):
            ctx.sync()
            m = N - 3 * (k % 3) if ragged else N
            kg, kd, cg = pairs_of(ctx, seed + 97 * k, mode, m, rows, cols, intr)
            bufs.append(outputs(m))
            tickets.append(ctx.call(pipe.submit, kg, kd, cg, *bufs[-1]))
            if k >= 2:
                ctx.call(pipe.wait, tickets[k - 2])
        ctx.call(pipe.drain)
        out = dict(tickets=tickets, steps=[step_result(*b) for b in bufs])
        ctx.call(pipe.__del__)
        return out
    job.oracle = (mode, arith, shape)
    return job


def trackers_job(arith, shape, seed, icp=False):
    """A V.Trackers of N dense sequences with depth filter, map, voxels, voxel statistics and map normals (icp: and the map ICP
    correction): init and STEPS - 1 frames, everything read back after each frame and the map at the end."""
    rows, cols, L = shape
    mode = V.CANDIDATES_DENSE
    cfg, intr = config(mode, arith, rows, cols, L)
    cap = rows * cols * STEPS

    def job(ctx):
        ctx.sync()
        tr = ctx.call(V.Trackers, cfg, N, rows, cols)
        ctx.call(tr.enable_depth_filter, *FILTER)
        ctx.call(tr.enable_map, 0, cap, MAX_KF, 0)
        ctx.call(tr.enable_map_voxels, VOXEL_M, SLOTS)
        ctx.call(tr.enable_map_voxel_stats)
        ctx.call(tr.enable_map_normals, *NORMALS)
        if icp:
            ctx.call(tr.enable_map_icp, **ICP)
        frames = []
        for k in range(STEPS):
            ctx.sync()
            g, d = ctx.call(V.synth_render_frames, [seed + s for s in range(N)], [k] * N, [BASE * SPEED[s] * k for s in range(N)], rows, cols, intr)
            ctx.call(tr.track if k else tr.init, g, d)
            poses, status, kf = ctx.call(tr.current_frames)
            r = dict(poses=poses.view(np.uint32), status=status, kf=kf, stats=ctx.call(tr.stats).copy() if k else None)
            r["depth"], r["weight"] = [host(t) for t in ctx.call(tr.keyframe_depth)]
            if icp and k:
                rec = ctx.call(tr.map_icp)
                r["icp_records"], r["icp_totals"] = host(rec["records"]), host(rec["totals"])
            frames.append(r)
        m, st, vox = ctx.call(tr.map), ctx.call(tr.map_voxel_stats), ctx.call(tr.map_voxels)
        normals = host(ctx.call(tr.map_normals))
        counts, n_seg = host(m["counts"]).view(np.uint32), host(m["n_segments"]).view(np.uint32)
        xyz, pixel, gray, seg = host(m["xyz"]), host(m["pixel"]), host(m["gray"]), host(m["segments"])
        sums, obs = host(st["sums"]), host(st["obs"])
        lists = []   # entries past a list's total are not data
        for s in range(N):
            c, j = min(int(counts[s]), cap), min(int(n_seg[s]), MAX_KF)
            lists.append(dict(xyz=xyz[s, :c].view(np.uint32), pixel=pixel[s, :c], gray=gray[s, :c], segments=seg[s, :j], sums=sums[s, :c],
                              obs=obs[s, :c], normals=normals[s, :c].view(np.uint32)))
        out = dict(frames=frames, counts=counts, n_segments=n_seg, lists=lists, occupied=host(vox["occupied"]), overflow=host(vox["overflow"]),
                   workspace=ctx.call(tr.workspace_bytes))
        ctx.call(tr.__del__)
        return out
    return job


def promotions(result):
    kf = np.stack([f["kf"] for f in result["frames"]])
    return int((kf[1:] != kf[:-1]).sum())


def tracker_frames(seed, shape, mode):
    rows, cols, L = shape
    intr = O.scaled_intrinsics(rows, cols)
    speed = 2.0 + (seed % 4)
    return [O.synth_frame((BLOCKY if mode == V.CANDIDATES_DSO else 0) | seed, BASE * speed * k, rows, cols, intr, frame_salt=k) for k in range(STEPS)]


def single_tracker_job(shape, seed):
    """A vors_tracker (host buffers; each call synchronises its own stream), REFERENCE arithmetic, coarse-to-fine."""
    rows, cols, L = shape
    mode = V.CANDIDATES_COARSE_TO_FINE
    cfg, _ = config(mode, V.ARITH_REFERENCE, rows, cols, L)
    frames = tracker_frames(seed, shape, mode)

    def job(ctx):
        ctx.sync()
        t = ctx.call(cfg.init, 0.0, frames[0][1], 0.0, frames[0][0])
        out = []
        ctx.sync()
        for k in range(1, STEPS):
            ctx.sync()
            g, d = frames[k]
            status = ctx.call(t.track, 0.1 * k, d, 0.1 * k + 0.01, g)
            stamp, pose = ctx.call(t.current_frame)
            out.append(dict(status=status, stamp=stamp, pose=pose.view(np.uint32), keyframe=ctx.call(t.keyframe)[1].view(np.uint32),
                            stats=np.array([ctx.call(t.last_stats)])))
        ctx.call(t.__del__)
        return out
    job.frames = frames
    return job


def handle_free_job(shape, seed):
    """vors_render_points, vors_depth_normals and vors_icp_points_robust on lists, planes and a workspace of the thread's own."""
    rows, cols, L = shape
    intr = O.scaled_intrinsics(rows, cols)
    cam = np.array(intr, np.float32)
    n = 2

    def job(ctx):
        import torch
        ctx.sync()
        dev = torch.device("cuda", torch.cuda.current_device())
        g0, d0 = ctx.call(V.synth_render_frames, [seed, seed + 1], [0, 0], [BASE * 0.0, BASE * 0.0], rows, cols, intr)
        z = host(d0).astype(np.float32) / np.float32(V.DEPTH_SCALE)
        v, u = np.meshgrid(np.arange(rows, dtype=np.float32), np.arange(cols, dtype=np.float32), indexing="ij")
        py = (v - cam[1]) / cam[3]
        px = ((u - cam[0]) - cam[4] * py) / cam[2]
        xyz = torch.from_numpy(np.ascontiguousarray(np.stack([px * z, py * z, z], axis=-1).reshape(n, rows * cols, 3).astype(np.float32))).to(dev)
        normals = ctx.call(V.depth_normals, d0, cam, V.DEPTH_SCALE, *NORMALS)["normals"].reshape(n, rows * cols, 3).contiguous()
        gray = g0.reshape(n, rows * cols).contiguous()
        counts = torch.full((n,), rows * cols, dtype=torch.int32, device=dev)
        poses = torch.tensor([[0, 0, 0, 0, 0, 0, 1.0]] * n, dtype=torch.float32, device=dev)
        ws = torch.empty(V.icp_workspace_bytes(n, rows * cols), dtype=torch.uint8, device=dev)
        out = []
        for k in range(STEPS):
            ctx.sync()
            _, d = ctx.call(V.synth_render_frames, [seed, seed + 1], [k, k], [BASE * 0.5 * k, BASE * -0.5 * k], rows, cols, intr)
            r = ctx.call(V.render_points, xyz, gray, counts, cam, rows, cols, V.DEPTH_SCALE, poses=poses, footprint=1 + k % 3, counts=True, zkey=True)
            fn = ctx.call(V.depth_normals, d, cam, V.DEPTH_SCALE, *NORMALS, counts=True)
            i = ctx.call(V.icp_points_robust, xyz, normals, counts, d, cam, V.DEPTH_SCALE, poses, 0.05, iters=4, frame_normals=fn["normals"],
                         min_cos=0.9, huber_m=0.002, workspace=ws, sums29=True, gate_counts=True)
            step = {"render_" + name: host(t) for name, t in r.items()}
            step.update({"normals_" + name: host(t).view(np.uint32) if name == "normals" else host(t) for name, t in fn.items()})
            step.update({"icp_" + name: host(t).view(np.uint32) if t.dtype == torch.float32 else host(t) for name, t in i.items()})
            out.append(step)
        return out
    return job


def churn_job(shape, seed, first_kind):
    """Create, step once and destroy, STEPS times, alternating between a dense Batch and a Pipeline."""
    rows, cols, L = shape
    mode = V.CANDIDATES_DENSE
    cfg, intr = config(mode, V.ARITH_FUSED, rows, cols, L)

    def job(ctx):
        ctx.sync()
        out = []
        for k in range(STEPS):
            ctx.sync()
            kg, kd, cg = pairs_of(ctx, seed + 97 * k, mode, N, rows, cols, intr)
            bufs = outputs(N)
            if (k + first_kind) % 2 == 0:
                h = ctx.call(V.Batch, cfg, N, rows, cols)
                ctx.call(h.track_pairs, kg, kd, cg, *bufs)
            else:
                h = ctx.call(V.Pipeline, cfg, N, rows, cols, depth=2)
                ctx.call(h.wait, ctx.call(h.submit, kg, kd, cg, *bufs))
            out.append(step_result(*bufs))   # (synchronises the thread's stream: the step is over before its handle goes)
            ctx.call(h.__del__)
        return out
    return job


def assert_reference_jobs_equal_the_oracle(jobs, serial):
    """The anchor is the oracle, not only this build: the serial results of every REFERENCE Batch / Pipeline job, step for step."""
    checked = 0
    for job, (res, ctx) in zip(jobs, serial):
        mode, arith, (rows, cols, L) = getattr(job, "oracle", (None, None, (0, 0, 0)))
        if arith != V.ARITH_REFERENCE:
            continue
        ocfg = O.make_config(L, O.scaled_intrinsics(rows, cols), candidates_mode=mode)
        for k, (step, (kg, kd, cg)) in enumerate(zip(res["steps"], ctx.inputs)):
            ref = O.track_pairs(ocfg, kg, kd, cg, n_threads=16)
            stats = np.frombuffer(step["stats"].tobytes(), V.PAIR_STATS_DTYPE)
            what = f"{MODES[mode]} {cols}x{rows} step {k}"
            assert (step["status"] == ref["status"]).all(), what
            assert (step["poses"] == ref["poses"].view(np.uint32)).all(), what + ": poses differ from the oracle's bits"
            assert (stats["lm_model"].view(np.uint32) == ref["models"].view(np.uint32)).all(), what
            assert (stats["nb_iter"][:, :L] == ref["nb_iter"]).all(), what
            assert (stats["optical_flow"].view(np.uint32) == ref["flow"].view(np.uint32)).all(), what
            checked += 1
    return checked


# ------------------------------------------------------------------------------------------------------------ 0
def test_the_library_is_a_cdll_so_calls_drop_the_gil():
    import ctypes
    assert type(V.lib()) is ctypes.CDLL and not isinstance(V.lib(), ctypes.PyDLL)


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("arith", [V.ARITH_REFERENCE, V.ARITH_FUSED], ids=["reference", "fused"])
@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES.values()))
def test_batch_handles_of_one_kind_on_four_threads(mode, arith):
    jobs = [batch_job(mode, arith, SHAPES[t % 2], 0x7EAD1000 + 0x100 * t + 16 * mode + arith) for t in range(4)]
    serial, _ = assert_threads_equal_serial(jobs)
    for res, _ in serial:
        assert len(set(res["workspace"])) == 1, "a step allocated"
    assert same(serial[0][0]["steps"], serial[2][0]["steps"]) is not None, "the seeds do not tell the threads apart"
    if arith == V.ARITH_REFERENCE:
        assert assert_reference_jobs_equal_the_oracle(jobs, serial) == 4 * STEPS


# ------------------------------------------------------------------------------------------------------------ 2
def test_mixed_batch_handles_on_eight_threads():
    kinds = [(0, V.ARITH_REFERENCE), (1, V.ARITH_FUSED), (2, V.ARITH_FUSED), (1, V.ARITH_REFERENCE), (0, V.ARITH_FUSED), (2, V.ARITH_REFERENCE),
             (1, V.ARITH_EXACT), (0, V.ARITH_EXACT)]
    jobs = [batch_job(mode, arith, SHAPES[(t // 2) % 2], 0x7EAD2000 + 0x100 * t, ragged=t in (2, 5)) for t, (mode, arith) in enumerate(kinds)]
    serial, _ = assert_threads_equal_serial(jobs)
    assert assert_reference_jobs_equal_the_oracle(jobs, serial) == 3 * STEPS


# ------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("arith", [V.ARITH_REFERENCE, V.ARITH_FUSED], ids=["reference", "fused"])
def test_trackers_with_map_voxels_statistics_and_normals_on_four_threads(arith):
    jobs = [trackers_job(arith, SHAPES[t % 2], 2000 + 100 * t) for t in range(4)]
    serial, _ = assert_threads_equal_serial(jobs)
    for t, (res, _) in enumerate(serial):
        assert promotions(res) >= 1, f"thread {t}: no sequence promotes a keyframe"
        assert (res["counts"] > 0).all() and (res["n_segments"] >= 1).all() and (res["overflow"] == 0).all()
        assert any(l["obs"][:, 0].max() >= 2 for l in res["lists"]), f"thread {t}: no voxel was seen twice"
        assert any(l["normals"].any() for l in res["lists"])


# ------------------------------------------------------------------------------------------------------------ 4
def test_single_trackers_on_four_threads_equal_the_oracle_tracker():
    jobs = [single_tracker_job(SHAPES[1], 77 + t) for t in range(4)]
    serial, _ = assert_threads_equal_serial(jobs)
    rows, cols, L = SHAPES[1]
    for job, (res, _) in zip(jobs, serial):
        f = job.frames
        ot = O.Tracker(O.make_config(L, O.scaled_intrinsics(rows, cols)), 0.0, f[0][1], 0.0, f[0][0])
        for k in range(1, STEPS):
            assert ot.track(0.1 * k, f[k][1], 0.1 * k + 0.01, f[k][0]) == res[k - 1]["status"]
            stamp, pose = ot.current_frame()
            assert stamp == res[k - 1]["stamp"] and (pose.view(np.uint32) == res[k - 1]["pose"]).all(), f"frame {k}"
            assert (ot.keyframe_pose()[1].view(np.uint32) == res[k - 1]["keyframe"]).all()


# ------------------------------------------------------------------------------------------------------------ 5
def test_every_handle_kind_at_once():
    jobs = [batch_job(V.CANDIDATES_DENSE, V.ARITH_FUSED, SHAPES[1], 0x7EAD5000),
            pipeline_job(V.CANDIDATES_COARSE_TO_FINE, V.ARITH_REFERENCE, SHAPES[1], 0x7EAD5100, depth=3),
            trackers_job(V.ARITH_FUSED, SHAPES[0], 5000, icp=True),
            handle_free_job(SHAPES[0], 5500)]
    serial, _ = assert_threads_equal_serial(jobs)
    assert assert_reference_jobs_equal_the_oracle(jobs, serial) == STEPS
    tracked = serial[2][0]
    assert promotions(tracked) >= 1 and tracked["frames"][-1]["icp_totals"][:, 0].sum() >= 1, "the correction was never attempted"
    free = serial[3][0]
    assert all(s["render_counts"][:, 2].min() > 0 for s in free) and any(np.ascontiguousarray(s["icp_stats"]).view(V.ICP_STATS_DTYPE)["matched"].min() > 0 for s in free)


# ------------------------------------------------------------------------------------------------------------ 6
def test_create_and_destroy_under_load():
    jobs = [batch_job(V.CANDIDATES_DENSE, V.ARITH_FUSED, SHAPES[1], 0x7EAD6000), batch_job(V.CANDIDATES_DSO, V.ARITH_REFERENCE, SHAPES[0], 0x7EAD6100),
            churn_job(SHAPES[0], 0x7EAD6200, 0), churn_job(SHAPES[1], 0x7EAD6300, 1)]
    serial, threaded = assert_threads_equal_serial(jobs)
    for (res, _), (got, _) in zip(serial[:2], threaded[:2]):
        assert len(set(got["workspace"])) == 1 and got["workspace"] == res["workspace"], "a long-lived handle's workspace changed"
    assert assert_reference_jobs_equal_the_oracle(jobs, serial) == STEPS


# ------------------------------------------------------------------------------------------------------------ 7
def first_use_child(how):
    """(this file run as a program) The process's first track_pairs: two coarse-to-fine and two DSO batches through vors_track_pairs,
    from four threads behind a barrier (`threads`) or one after another (`serial`); prints a hash of every output."""
    rows, cols, L = SHAPES[1]
    intr = O.scaled_intrinsics(rows, cols)
    work = []
    for t, mode in enumerate([V.CANDIDATES_COARSE_TO_FINE, V.CANDIDATES_DSO, V.CANDIDATES_COARSE_TO_FINE, V.CANDIDATES_DSO]):
        kg, kd, cg, _, _ = O.synth_batch(N, rows, cols, seed0=(BLOCKY if mode == V.CANDIDATES_DSO else 0) | (0x7EAD7000 + 0x100 * t), intr=intr)
        cfg, _ = config(mode, V.ARITH_FUSED if t < 2 else V.ARITH_REFERENCE, rows, cols, L)
        work.append((cfg, kg, kd, cg))
    V.lib()   # loaded by one thread; no entry of it has run yet
    out, errors = [None] * 4, []
    barrier = threading.Barrier(4)

    def body(i):
        try:
            if how == "threads":
                barrier.wait(timeout=JOIN_TIMEOUT_S)
            poses, status, stats = V.track_pairs(*work[i])
            out[i] = poses.tobytes() + status.tobytes() + stats.tobytes()
        except BaseException as e:   # noqa: B036
            errors.append(e)
            barrier.abort()

    if how == "threads":
        threads = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(JOIN_TIMEOUT_S)
            if t.is_alive():
                print("HUNG", flush=True)
                os._exit(4)
    else:
        for i in range(4):
            body(i)
    if errors:
        raise errors[0]
    assert (np.frombuffer(out[0], np.uint8).size == np.frombuffer(out[2], np.uint8).size) and out[0] != out[2]
    print("FIRST-USE " + hashlib.sha256(b"".join(out)).hexdigest(), flush=True)


@pytest.mark.parametrize("pyramid_fused", [None, "0"], ids=["environment_as_it_is", "VORS_PYRAMID_FUSED=0"])
def test_first_use_in_a_fresh_process_from_four_threads(pyramid_fused):
    env = dict(os.environ)
    if pyramid_fused is not None:
        env["VORS_PYRAMID_FUSED"] = pyramid_fused
    hashes = {}
    for how in ("serial", "threads"):
        try:   # a new process each time: nothing replaces the program of a process that has opened the GPU
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--first-use", how], env=env, capture_output=True, text=True,
                                   timeout=JOIN_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            stop_the_session(f"the first-use child ({how}) did not finish within {JOIN_TIMEOUT_S} s")
        if child.returncode < 0 or child.returncode in (4, 134, 139):
            stop_the_session(f"the first-use child ({how}) ended with status {child.returncode}: {child.stderr[-2000:]}")
        assert child.returncode == 0, child.stdout + child.stderr
        lines = [l for l in child.stdout.splitlines() if l.startswith("FIRST-USE ")]
        assert len(lines) == 1, child.stdout + child.stderr
        hashes[how] = lines[0]
    assert hashes["threads"] == hashes["serial"]


# ------------------------------------------------------------------------------------------------------------ 8
def refused_job(kind, shape, seed, calls_per_step=40):
    """A live handle and the same refused call over and over, nothing enqueued: `batch` = track_current with more pairs than were
    prepared, `pipeline` = a wait on a ticket that does not exist -> every (status, vors_last_error()) the thread saw."""
    rows, cols, L = shape
    mode = V.CANDIDATES_COARSE_TO_FINE
    cfg, intr = config(mode, V.ARITH_FUSED, rows, cols, L)

    def job(ctx):
        lib = V.lib()
        ctx.sync()
        kg, kd, cg = pairs_of(ctx, seed, mode, N, rows, cols, intr)
        poses, status, _ = outputs(N)
        if kind == "batch":
            h = ctx.call(V.Batch, cfg, N, rows, cols)
            ctx.call(h.prepare_keyframes, kg[:4], kd[:4])
            refused = lambda: lib.vors_batch_track_current(h._h, N, V.Batch._dp(cg), None, V.Batch._dp(poses), V.Batch._dp(status), None, V.Batch._stream())
        else:
            h = ctx.call(V.Pipeline, cfg, N, rows, cols, depth=2)
            refused = lambda: lib.vors_pipeline_wait(h._h, 99, V.Batch._stream(), 0)
        seen = set()
        for k in range(STEPS):
            ctx.sync()
            for _ in range(calls_per_step):
                st = ctx.call(refused)
                seen.add((st, lib.vors_last_error()))
        out = dict(seen=sorted(seen), untouched=host(status))
        ctx.call(h.__del__)
        return out
    return job


def test_last_error_is_per_thread():
    jobs = [refused_job("batch", SHAPES[0], 0x7EAD8000), refused_job("pipeline", SHAPES[0], 0x7EAD8100),
            batch_job(V.CANDIDATES_DENSE, V.ARITH_FUSED, SHAPES[0], 0x7EAD8200), batch_job(V.CANDIDATES_COARSE_TO_FINE, V.ARITH_REFERENCE, SHAPES[1], 0x7EAD8300)]
    serial, threaded = assert_threads_equal_serial(jobs)
    (a, _), (b, _) = threaded[0], threaded[1]
    assert len(a["seen"]) == 1 and len(b["seen"]) == 1, f"a thread saw more than its own message: {a['seen']} {b['seen']}"
    (st_a, msg_a), (st_b, msg_b) = a["seen"][0], b["seen"][0]
    assert st_a == st_b == -1 and msg_a and msg_b and msg_a != msg_b   # VORS_ERR_INVALID_ARGUMENT, two different sentences
    assert (a["untouched"] == -9).all(), "a refused call wrote"
    assert assert_reference_jobs_equal_the_oracle(jobs, serial) == STEPS


# ------------------------------------------------------------------------------------------------------------ 9
def test_current_device_is_unchanged_after_every_call():
    """Ctx.call asserts it after every library call of every job above; here once more by name, for one job of each kind, with the number
    of checks. With one GPU this only pins "restores the caller's current device": the handle's device IS the caller's. The
    cross-device half — a handle of device 1 called while device 0 is current — needs a second GPU; tests/test_gpu_multi.py keeps it."""
    import torch
    jobs = [batch_job(V.CANDIDATES_DSO, V.ARITH_FUSED, SHAPES[0], 0x7EAD9000), pipeline_job(V.CANDIDATES_DENSE, V.ARITH_FUSED, SHAPES[0], 0x7EAD9100),
            trackers_job(V.ARITH_FUSED, SHAPES[0], 9000), single_tracker_job(SHAPES[0], 91)]
    before = torch.cuda.current_device()
    got = run_threads(jobs)
    assert torch.cuda.current_device() == before
    for (_, ctx), least in zip(got, (2 + 3 * STEPS, 2 + 2 * STEPS, 6 + 4 * STEPS, 1 + 4 * (STEPS - 1))):
        assert ctx.device == before and ctx.device_checks >= least


# ------------------------------------------------------------------------------------------------------------ 10
def test_dense_fused_handles_with_a_side_lane_on_two_threads():
    """Beyond the 8 pairs of the cases above, because at 8 pairs the case they were meant for does not exist: a dense handle owns a side-lane
    stream and its two events only from 2048 pairs on, with two levels of >= 64 Ki pixels (batch.cpp plan_split: 512x512 has levels 0 and
    1). Two such handles are created, step twice and are destroyed side by side, next to a small neighbour of the same kind."""
    big = (512, 512, 5)
    jobs = [batch_job(V.CANDIDATES_DENSE, V.ARITH_FUSED, big, 0x7EADA000, n=2048, steps=2),
            batch_job(V.CANDIDATES_DENSE, V.ARITH_FUSED, big, 0x7EADA100, n=2048, steps=2),
            batch_job(V.CANDIDATES_DENSE, V.ARITH_FUSED, SHAPES[1], 0x7EADA200, steps=2)]
    serial, _ = assert_threads_equal_serial(jobs)
    for res, _ in serial:
        assert len(set(res["workspace"])) == 1
    assert same(serial[0][0]["steps"], serial[1][0]["steps"]) is not None, "the seeds do not tell the threads apart"


# ------------------------------------------------------------------------------------------------------------ 11
def test_lm_solve_from_eight_threads_on_the_device():
    """csrc/host_threads_check without --host-only: vors_lm_solve of a valid observation from eight std::threads, every output byte and
    every vors_last_error() equal to the serial calls. tests/test_threads_host.py runs the same program on the CPU, host entries only."""
    csrc = os.path.join(ROOT, "visual-odometry-rs_amd", "csrc")
    program = os.path.join(csrc, "host_threads_check")
    if not os.path.exists(program):   # (a prebuilt one is used as it is, like the libraries)
        subprocess.check_call(["make", "-C", csrc, "-s", "host_threads_check"])
    try:
        out = subprocess.run([program], capture_output=True, text=True, timeout=JOIN_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        stop_the_session(f"host_threads_check did not finish within {JOIN_TIMEOUT_S} s")
    if out.returncode < 0 or out.returncode in (134, 139):
        stop_the_session(f"host_threads_check ended with status {out.returncode}: {out.stderr[-2000:]}")
    assert out.returncode == 0 and "vors_lm_solve included" in out.stdout, out.stdout + out.stderr


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--first-use" and sys.argv[2] in ("serial", "threads")
    first_use_child(sys.argv[2])
