"""Development aid (GPU): record tests/golden/tap_sharing/sums.npz — for every case of tests/test_gpu_tap_sharing.py the model and the 29
FUSED sums, for every tracked shape the hostile initial models and what vors_batch_track_pairs returns from them — as THIS build computes
them, and print how far each evaluation is from the EXACT arithmetic.
Run it on the commit whose results are to be pinned (the parent of a change that must not move them).
usage: python tools/make_tap_sharing_golden.py [OUT.npz]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "visual-odometry-rs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import vors_amd as V
import test_gpu_tap_sharing as T

out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
data = {}
handles = T.Handles()
for case in T.CASES:
    model = T.model_of(handles, case)
    fused, exact = T.sums29(handles, case, model, V.ARITH_FUSED), T.sums29(handles, case, model, V.ARITH_EXACT)
    again = T.sums29(handles, case, model, V.ARITH_FUSED)
    assert (fused.view(np.uint32) == again.view(np.uint32)).all(), "not reproducible"
    rel = lambda a, b: float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-30))
    print(f"{T.case_id(case):44s} n_inside {int(fused[1]):6d} / {int(exact[1]):6d} exact; vs exact: e {rel(fused[0:1], exact[0:1]):.2e} "
          f"g {rel(fused[2:8], exact[2:8]):.2e} H {rel(fused[8:], exact[8:]):.2e}")
    data["model__" + T.case_id(case)] = model
    data["sums__" + T.case_id(case)] = fused
handles.h.clear()
for shape in T.TRACKED:
    b, frames, gt = T.render(shape)
    prev = T.hostile_priors(gt)
    poses, status, stats = T.track(b, frames, prev)
    again = T.track(b, frames, prev)
    assert (poses.view(np.uint32) == again[0].view(np.uint32)).all() and (stats == again[2]).all(), "not reproducible"
    L = T.SHAPES[shape][2]
    st = np.frombuffer(stats.tobytes(), V.PAIR_STATS_DTYPE)
    print(f"{shape}: status {status.tolist()} iterations per level {st['nb_iter'][:, :L].tolist()} evaluations {st['nb_grad_evals'][:, :L].tolist()}")
    data.update({"prev__" + shape: prev, "poses__" + shape: poses, "status__" + shape: status, "stats__" + shape: stats})
np.savez(out, **data)
print(f"wrote {out}: {len(T.CASES)} evaluations, {len(T.TRACKED)} tracked batches, {os.path.getsize(out)} bytes")
