"""Generates tests/golden/adversarial/*.npz: one small batch per scene family of tests/adversarial.py with the ORACLE's results —
statuses, poses, final models, iteration and point counts, per-level energies, optical flow — and the outcome flags of its replay.
(A subdirectory: the fixtures of make_golden.py, golden/*.npz, have other keys.) Run from the repo root:
    python tests/golden/make_adversarial.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
from oracle import oracle as O  # noqa: E402

import adversarial as A  # noqa: E402

ROWS, COLS, L, N = 96, 128, 3, 6
INTR = O.scaled_intrinsics(ROWS, COLS)
# family -> (candidates mode, Huber delta): each family where it bites (brightness jumps in dense mode, occluders with Huber)
SETTINGS = {"depth_step": (0, 0.0), "invalid_blobs": (0, 0.0), "occluder": (0, 10.0), "large_motion": (0, 0.0),
            "brightness_jump": (1, 0.0), "saturated": (0, 0.0), "mid_pyramid": (1, 0.0), "rank_deficient": (0, 0.0)}
SEED0 = 0xADD5000
OUTCOME_POOL = 48  # rank-deficient pairs searched for outcomes 1, 2 and 3 (the fixture keeps the pairs that reach one)


def scene(family, seed, n, mode):
    if family == "rank_deficient":
        return A.rank_deficient(seed, n, ROWS, COLS, INTR, mode=mode, L=L)
    return A.FAMILIES[family](seed, n, ROWS, COLS, INTR)


def make(name, family, seed, n, mode, huber, pick=None):
    kg, kd, cg, init = scene(family, seed, n, mode)
    cfg = O.make_config(L, INTR, candidates_mode=mode, huber_delta=huber)
    if pick is not None:  # keep the pairs the replay classifies as the targeted outcomes
        cls = A.classify(cfg, kg, kd, cg, init)
        keep = np.flatnonzero(pick(cls))
        kg, kd, cg = kg[keep], kd[keep], cg[keep]
        init = None if init is None else init[keep]
    else:
        keep = np.arange(n)
    ref = O.track_pairs(cfg, kg, kd, cg, init_poses7=init)
    cls = A.classify(cfg, kg, kd, cg, init)
    A.check_replay(ref, cls)
    out = dict(family=family, seed=np.uint64(seed), n_generated=n, picked=keep.astype(np.int32), rows=ROWS, cols=COLS, L=L, mode=mode,
               huber=np.float32(huber), intr=np.asarray(INTR, np.float64), kf_gray=kg, kf_depth=kd, cur_gray=cg,
               init=np.tile(A.identity7(), (len(kg), 1)) if init is None else init, has_init=init is not None,
               status=ref["status"], poses=ref["poses"], models=ref["models"], nb_iter=ref["nb_iter"], n_points=ref["n_points"],
               flow=ref["flow"], energy=cls["energy"], o1=cls["o1"], o2=cls["o2"], o3=cls["o3"])
    os.makedirs(os.path.join(HERE, "adversarial"), exist_ok=True)
    path = os.path.join(HERE, "adversarial", name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(kg)} pairs, failed {int(ref['status'].sum())}, outcomes 1/2/3: {int(cls['o1'].sum())} / {int(cls['o2'].sum())} / "
          f"{int(cls['o3'].sum())}, {os.path.getsize(path) // 1024} KiB")


if __name__ == "__main__":
    for k, (family, (mode, huber)) in enumerate(SETTINGS.items()):
        make(family, family, SEED0 + 0x100 * k, N, mode, huber)
    make("outcomes", "rank_deficient", SEED0 + 0x1000, OUTCOME_POOL, 0, 0.0, pick=lambda c: c["o1"] | c["o2"] | c["o3"])
