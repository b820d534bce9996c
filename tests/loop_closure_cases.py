"""What tests/test_loop_closure_host.py and tests/test_gpu_loop_closure.py share: numpy restatements of the loop-closure definitions
(include/vors_hip.h 2h) and the test data. Signatures and dot products are exact integers (int64 here); the score is one float64 divide
of an exact numerator by the product of two float64 roots, cast to float32 — IEEE sqrt, multiply and divide are correctly rounded in numpy
as in the library, so the comparison is one of bits."""
import numpy as np

import pose_graph_cases as P

EMPTY = 0xFFFFFFFF
SHAPES = [(60, 80, 8, 8), (61, 83, 12, 16), (64, 64, 32, 32), (8, 8, 8, 8)]  # rows, cols, tr, tc


def signature(gray, tr, tc):
    """-> (sig int8 [tr * tc], sum, sumsq)"""
    rows, cols = gray.shape
    s = np.zeros(tr * tc, np.int64)
    for cy in range(tr):
        for cx in range(tc):
            cell = gray[cy * rows // tr:(cy + 1) * rows // tr, cx * cols // tc:(cx + 1) * cols // tc]
            total, cnt = int(cell.astype(np.uint64).sum()), cell.size
            s[cy * tc + cx] = (2 * total + cnt) // (2 * cnt) - 128
    return s.astype(np.int8), int(s.sum()), int((s * s).sum())


def planes(rows, cols, seed=0):
    rng = np.random.default_rng(seed)
    return [np.zeros((rows, cols), np.uint8), np.full((rows, cols), 255, np.uint8), rng.integers(0, 256, (rows, cols), dtype=np.uint8),
            (rng.integers(0, 40, (rows, cols)) + np.linspace(0, 200, cols)[None, :]).astype(np.uint8)]


def meta_of(sig):
    s = np.asarray(sig, np.int64)
    return np.stack([s.sum(-1), (s * s).sum(-1)], axis=-1).astype(np.int32)


def pose_gate(pi, pj, max_dist_m, min_qdot):
    """float32, in the written order; a half whose parameter is 0 is off."""
    pi, pj = np.asarray(pi, np.float32), np.asarray(pj, np.float32)
    ok = True
    with np.errstate(all="ignore"):
        if max_dist_m > 0:
            d = pi[:3] - pj[:3]
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            ok = bool(d2 <= np.float32(max_dist_m) * np.float32(max_dist_m))
        if min_qdot > 0:
            qd = np.abs(((pi[3] * pj[3] + pi[4] * pj[4]) + pi[5] * pj[5]) + pi[6] * pj[6])
            ok = ok and bool(np.isfinite(qd)) and bool(qd >= np.float32(min_qdot))
    return ok


def candidates(sig, min_gap, k, min_score, poses=None, max_dist_m=0.0, min_qdot=0.0, query_first=0, count=None):
    """The brute force -> (cand_i uint32 [capacity, k], cand_score float32 [capacity, k], cand_counts uint32 [capacity], counts [5]);
    queries outside [query_first, count) keep unused slots and a count of 0."""
    s = np.asarray(sig, np.int64)
    cap, d = s.shape
    n = cap if count is None else min(count, cap)
    sm, sq = s.sum(1), (s * s).sum(1)
    va = d * sq - sm * sm
    root = np.sqrt(va.astype(np.float64))
    num = d * (s @ s.T) - np.outer(sm, sm)
    with np.errstate(all="ignore"):
        score = (num.astype(np.float64) / (root[:, None] * root[None, :])).astype(np.float32)
    ci, cs = np.full((cap, k), EMPTY, np.uint32), np.zeros((cap, k), np.float32)
    cc, counts = np.zeros(cap, np.uint32), np.zeros(5, np.uint64)
    for j in range(query_first, n):
        keep = []
        for i in range(0, j - min_gap + 1):
            counts[0] += 1
            if va[i] == 0 or va[j] == 0:
                counts[1] += 1
            elif poses is not None and not pose_gate(poses[i], poses[j], max_dist_m, min_qdot):
                counts[2] += 1
            elif not score[i, j] >= np.float32(min_score):
                counts[3] += 1
            else:
                counts[4] += 1
                keep.append((-float(score[i, j]), i))
        keep.sort()
        for p, (_, i) in enumerate(keep[:k]):
            ci[j, p], cs[j, p] = i, score[i, j]
        cc[j] = min(k, len(keep))
    return ci, cs, cc, counts.astype(np.uint32)


def random_signatures(count, d, seed):
    return np.random.default_rng(seed).integers(-128, 128, (count, d)).astype(np.int8)


def asymmetric_signatures(count, d):
    """signature r holds ((r * 7 + c * 13) % 255) - 127 at cell c: a swapped row / column C-write or a mismatched k-map cannot pass"""
    r, c = np.arange(count)[:, None], np.arange(d)[None, :]
    return (((r * 7 + c * 13) % 255) - 127).astype(np.int8)


def special_signatures(d=64, seed=3):
    """24 signatures: 6 and 7 identical (equal scores order by index), 11 flat, 15 the negative image of 2"""
    s = np.random.default_rng(seed).integers(-127, 128, (24, d)).astype(np.int8)
    s[7] = s[6]
    s[11] = 5
    s[15] = -s[2]
    return s


def line_poses(count, step=0.1):
    p = np.zeros((count, 7), np.float32)
    p[:, 0] = step * np.arange(count)
    p[:, 6] = 1.0
    return p


def f32(pose):
    return np.asarray(pose, np.float64).astype(np.float32)


def verify_cases(m, seed, nodes=16):
    """m tracked candidates over `nodes` random poses with a random mix of defects (kind: 0 none, 1 forward status, 2 index, 3 not finite,
    4 cycle translation, 5 cycle rotation, 6 prior translation, 7 prior rotation, 8 backward status); consistent ones are exact up to
    float32 rounding, defects are 0.2 m / 0.2 rad against bounds of 0.01."""
    rng = np.random.default_rng(seed)
    poses = np.array([P.random_pose(rng, 1.0, 1.0) for _ in range(nodes)])
    kind = rng.integers(0, 9, m)
    kind[0] = 0
    pairs = np.zeros((m, 2), np.uint32)
    fwd, bwd = np.zeros((m, 7), np.float32), np.zeros((m, 7), np.float32)
    sf, sb = np.zeros(m, np.int32), np.zeros(m, np.int32)
    info = np.zeros((m, 36), np.float32)
    off_t, off_r = P.se3_exp([0.2, 0, 0, 0, 0, 0]), P.se3_exp([0, 0, 0, 0, 0.2, 0])
    for e in range(m):
        i = int(rng.integers(0, nodes))
        j = int((i + 1 + rng.integers(0, nodes - 1)) % nodes)
        model = P.iso_mul(P.iso_inv(poses[j]), poses[i])
        back = P.iso_inv(model)
        if kind[e] == 4:
            back = P.iso_mul(off_t, back)
        if kind[e] == 5:
            back = P.iso_mul(off_r, back)
        if kind[e] in (6, 7):
            model = P.iso_mul(model, off_t if kind[e] == 6 else off_r)
            back = P.iso_inv(model)
        if kind[e] == 2:
            j = i if e % 2 else nodes + e % 3
        pairs[e], fwd[e], bwd[e] = (i, j), f32(model), f32(back)
        sf[e], sb[e] = int(kind[e] == 1), int(kind[e] == 8)
        info[e] = (np.diag(rng.uniform(1.0, 9.0, 6)) + 0.1 * np.ones((6, 6))).reshape(36)
        if kind[e] == 3:
            (fwd[e], bwd[e], info[e])[e % 3][e % 7] = (np.nan, np.inf)[e % 2]
    return dict(pairs=pairs, model_fwd=fwd, model_bwd=bwd, status_fwd=sf, status_bwd=sb, info=info, poses=f32(poses)), kind


VERIFY_BOUNDS = dict(max_cycle_trans=0.01, max_cycle_rot=0.01, max_prior_trans=0.01, max_prior_rot=0.01)
EXPECTED_VERDICT = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7, 8: 1}  # kind -> VORS_LOOP_* while the list has room
