"""The robust point-to-plane ICP on the host (vors_icp_points_robust_host; needs no GPU): lie.h icp_row_robust / icp_products_robust in the
loop and the order of sums of vors_icp_points_host.

The scene is tests/test_icp_host.py's corner of three planes in a 48x64 depth map at scale 5000 (the generator is restated here); the
model is its back-projection through P_TRUE with depth_normals_host's normals. FRAMES are that depth map with a rectangular patch
replaced by a foreign surface that stays inside DIST_M: "step" — the patch pushed back along the view rays, fronto-parallel to the
surface it replaces (for Huber); "ramp" — a saw-tooth of ramps across the patch whose normals differ from the model's by more than
acos(MIN_COS) (for the normal gate); "both" — the two side by side (for the gate counts). The frame normals are depth_normals_host's of
the frame itself, without a pose.

`robust64()` is ONE float64 numpy statement of the rule (landing, the three gates, the Huber weight); `irls64()` the loop around it.

Measured here (and recorded in DESIGN.md 7m):
  evaluator (MIN_COS 0.9, HUBER_M 2 mm, distance gate 50 mm, frame "both"): gate counts of 2988 considered, per pose:
      [2976, 2746, 2261, 2139], [2976, 2626, 2261, 2039], [2976, 2626, 2261, 690]; largest |s32 - s64| over the 28 sums in units of
      eps x magnitude (test_icp_host.py's model, extended by the weight: see magnitudes()): 0.0418, 0.149, 0.122 — asserted at
      test_icp_host.py's bound, 4 x 0.794.
  it helps: errors against P_TRUE after ITERS = 10 rounds from START (translation / rotation), DIST_M 0.1:
      step: plain 9.22 mm / 1.44 deg, robust (Huber 2 mm) 0.933 mm / 0.16 deg: ratios 9.88 / 8.99, the float64 restatement the same
      ramp: plain 3.19 mm / 0.246 deg, robust (normal gate 0.9) 0.055 mm / 0.00276 deg: ratios 58 / 89, the float64 restatement the same
  the robust loop against irls64(): |pose32 - pose64| over the 7 numbers: step 1.97e-08, ramp 4.18e-08.
      MEASURED_POSE_DIFF = 4.2e-08; asserted at 4 x that.
"""
import numpy as np
import pytest

import vors_amd as V

SCALE = 5000.0
ROWS, COLS = 48, 64
CAM = np.array([31.5, 23.5, 60.0, 61.0, 0.0], np.float32)
DIST_M = 0.1
MIN_COS = 0.9
HUBER_M = 0.002
PLANES = (((0.5, 0.0, 1.0), 2.0), ((-0.5, 0.1, 1.0), 2.0), ((0.0, -0.6, 1.0), 2.2))
SUM_REL_BOUND = 4 * 0.794  # tests/test_icp_host.py's: 4 x its measured 0.794, in eps x magnitude
MEASURED_POSE_DIFF = 4.2e-08  # the docstring
POSE_DIFF_BOUND = 4 * MEASURED_POSE_DIFF
COUNTS = [1, 1023, 1024, 1025, 2500]


# ------------------------------------------------------------------------------------------------------------ the scene
def corner_z(rows=ROWS, cols=COLS, cam=CAM):
    cu, cv, fu, fv, skew = [float(v) for v in cam]
    x, y = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    ry = (y - cv) / fv
    rx = ((x - cu) - skew * ry) / fu
    return np.min([dist / (n[0] * rx + n[1] * ry + n[2]) for n, dist in PLANES], axis=0)


def to_depth(z):
    d = np.rint(z * SCALE)
    assert d.min() >= 1 and d.max() <= 65535
    d = d.astype(np.uint16)
    d.reshape(-1)[::37] = 0  # some pixels without depth
    return d


def patched(kind):
    """The corner with a foreign patch, every pixel of which stays within DIST_M of the surface it replaces along its view ray."""
    z = corner_z()
    x = np.arange(COLS, dtype=np.float64)[None, :]
    if kind in ("step", "both"):
        z[8:30, 6:26] *= 1.02  # ~ 40 mm behind, parallel to the surface it replaces as seen from the camera
    if kind in ("ramp", "both"):
        saw = ((x - 36) % 4 - 1.5) / 1.5  # -1 .. 1 across every 4 columns
        z[10:40, 36:60] *= (1.0 + 0.03 * saw)[:, 36:60]
    assert np.abs(z - corner_z()).max() * 1.2 < DIST_M  # (|ray| / z < 1.2 in this camera)
    return to_depth(z)


def pose_from_xi(xi):
    out = np.zeros(7, np.float32)
    V.lib().vors_se3_exp(V._ptr(np.ascontiguousarray(xi, np.float32)), V._ptr(out))
    return out


P_TRUE = pose_from_xi([0.3, -0.2, 0.1, 0.05, -0.1, 0.08])


def frame_normals_of(depth):
    return np.ascontiguousarray(V.depth_normals_host(depth, CAM, SCALE, 2, 0.05)["normals"], np.float32)


@pytest.fixture(scope="module")
def model():
    """The list of the clean corner's pixels with depth, in the world frame of P_TRUE: (xyz [m, 3], normals [m, 3])."""
    depth = to_depth(corner_z())
    ys, xs = np.nonzero(depth)
    xy = np.stack([xs, ys], -1).astype(np.float32)
    z = (np.float32(1.0) / (np.float32(SCALE) / depth[ys, xs].astype(np.float32))).astype(np.float32)
    xyz = V.camera_back_project(CAM, P_TRUE, xy, z)
    nrm = V.depth_normals_host(depth, CAM, SCALE, 2, 0.05, pose7=P_TRUE)["normals"][ys, xs]
    assert len(xyz) > 2600 and (np.abs(nrm).sum(-1) > 0).mean() > 0.9
    return np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(nrm, np.float32)


@pytest.fixture(scope="module")
def frames():
    out = {}
    for kind in ("clean", "step", "ramp", "both"):
        depth = patched(kind)
        out[kind] = (depth, frame_normals_of(depth))
    return out


# ------------------------------------------------------------------------------------------------------------ the rule in float64
def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def products(a, w=None, wr=None, e=None):
    """The 28 products of rows a [m, 7]: icp_products, or icp_products_robust with the weights given."""
    w = np.ones(len(a), a.dtype) if w is None else w
    wr = a[:, 0] if wr is None else wr
    e = a[:, 0] * a[:, 0] if e is None else e
    cols = [e] + [a[:, i] * wr for i in range(1, 7)]
    cols += [w * (a[:, i] * a[:, j]) for i in range(1, 7) for j in range(i, 7)]
    return np.stack(cols, -1)


def robust64(xyz, nrm, pose, depth, fn, min_cos, huber_m, dist_m=DIST_M):
    """The rule of vors_icp_points_robust for every point of a list at `pose` in float64 (fn None: no normal gate; huber_m 0: no weight)
    -> the gates passed, the rows, the weights, the distances of every quantity from its decision, the magnitudes of the sums' errors."""
    f = np.float64
    w, nw = xyz.astype(f), nrm.astype(f)
    t, q = pose[:3].astype(f), pose[3:].astype(f)
    cu, cv, fu, fv, skew = [f(v) for v in CAM]
    rows, cols = depth.shape

    def rotate_conj(p):  # quat_rotate(conj(q), p)
        qv = np.broadcast_to(-q[:3], p.shape)
        tt = cross(qv, p) * 2.0
        return (tt * q[3] + cross(qv, tt)) + p

    with np.errstate(all="ignore"):
        c = rotate_conj(w - t)
        u = ((fu * c[:, 0] + skew * c[:, 1]) + cu * c[:, 2]) / c[:, 2]
        v = (fv * c[:, 1] + cv * c[:, 2]) / c[:, 2]
        x0, y0 = np.floor(u + 0.5), np.floor(v + 0.5)
        lands = (c[:, 2] > 0) & (x0 >= 0) & (x0 < cols) & (y0 >= 0) & (y0 < rows)
        xi, yi = np.where(lands, x0, 0).astype(np.int64), np.where(lands, y0, 0).astype(np.int64)
        d = depth[yi, xi]
        with_depth = lands & ~((nw == 0).all(-1)) & (d != 0)
        z = 1.0 / (f(SCALE) / np.where(with_depth, d, 1).astype(f))
        qy = (yi.astype(f) - cv) * z / fv
        qx = ((xi.astype(f) - cu) * z - skew * qy) / fu
        qq = np.stack([qx, qy, z], -1)
        e = qq - c
        dist = np.sqrt(dot3(e, e))
        within = with_depth & (dist <= dist_m)
        n = rotate_conj(nw)
        matched = within
        cosine = np.ones(len(w))
        if fn is not None:
            nf = fn[yi, xi].astype(f)
            cosine = dot3(n, nf)
            matched = within & ~((nf == 0).all(-1)) & (cosine >= min_cos)
        r = np.where(matched, dot3(n, e), 0.0)
        J = np.where(matched[:, None], np.concatenate([n, cross(qq, n)], -1), 0.0)
        frac_u, frac_v = (u + 0.5) - x0, (v + 0.5) - y0
        edge = np.where(c[:, 2] > 0, np.minimum(np.minimum(frac_u, 1 - frac_u), np.minimum(frac_v, 1 - frac_v)), 1.0)
    ar = np.abs(r)
    lin = ar <= huber_m if huber_m > 0 else np.ones(len(r), bool)
    wgt = np.where(lin, 1.0, huber_m / np.where(lin, 1.0, ar))
    loss = np.where(lin, r * r, huber_m * (2.0 * ar - huber_m))
    # no point within 1e-4 (relative) of a decision: the pixel it lands in, the distance gate, min_cos, |r| against huber_m
    doubtful = (edge < 1e-4) | (with_depth & (np.abs(dist / dist_m - 1.0) < 1e-4))
    if fn is not None:
        doubtful |= within & (np.abs(cosine - min_cos) < 1e-4)
    if huber_m > 0:
        doubtful |= matched & (np.abs(ar / huber_m - 1.0) < 1e-4)
    rows7 = np.concatenate([r[:, None], J], -1)
    return dict(with_depth=with_depth, within=within, matched=matched, linear=matched & ~lin, doubtful=doubtful, rows=rows7, w=wgt,
                terms=products(rows7, wgt, wgt * r, loss), q_norm=np.where(matched, np.sqrt(dot3(qq, qq)), 0.0), loss=loss, lin=lin)


def magnitudes(o, huber_m):
    """What a forward error of the 28 sums is measured against, in units of the float32 epsilon: tests/test_icp_host.py's model — every
    product a relative eps, r = n . (q - c) an ABSOLUTE eps |q| — extended by the weight. On the quadratic branch w = 1 exactly and the
    model is unchanged. On the linear branch w = huber_m / |r| carries the division's relative eps and r's own error eps |q| / |r|,
    i.e. an absolute eps w (1 + |q| / |r|); so per point: w J_i J_j: w |J_i J_j| (2 + |q| / |r|); J_i (w r): |J_i| w (|r| + |q|) twice,
    once for r and once for w; the loss huber_m (2 |r| - huber_m): two more roundings of its own size and 2 huber_m eps |q| from r."""
    eps = float(np.finfo(np.float32).eps)
    a, qn, w = np.abs(o["rows"]), o["q_norm"], o["w"]
    nonlin = ~o["lin"]
    ar = np.where(nonlin, a[:, 0], 1.0)
    jj = products(a)[:, 7:] * (w * np.where(nonlin, 2.0 + qn / ar, 1.0))[:, None]
    jr = a[:, 1:] * (w * (a[:, 0] + qn) * np.where(nonlin, 2.0, 1.0))[:, None]
    e0 = np.where(nonlin, 2.0 * np.abs(o["loss"]) + 2.0 * huber_m * qn, a[:, 0] ** 2 + 2 * a[:, 0] * qn + eps * qn * qn)
    return eps * np.concatenate([e0[:, None], jr, jj], -1).sum(0)


def tree32(terms, count):
    """The order of the sums in float32 for per-point products [count, 28]."""
    total = None
    for base in range(0, count, 1024):
        v = np.zeros((1024, 28), np.float32)
        part = terms[base:min(base + 1024, count)]
        v[:len(part)] = part
        w = 512
        while w >= 1:
            v[:w] = v[:w] + v[w:2 * w]
            w //= 2
        total = v[0].copy() if total is None else total + v[0]
    return np.zeros(28, np.float32) if total is None else total


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ 1. the neutral case
OFF = pose_from_xi([0.01, -0.015, 0.02, 0.01, 0.005, -0.012])


@pytest.mark.parametrize("ranged", [False, True])
@pytest.mark.parametrize("count", COUNTS)
def test_neutral_case_is_the_plain_pass(model, frames, count, ranged):
    xyz, nrm = model
    depth = frames["both"][0]
    start = V.iso_mul(P_TRUE, OFF)
    rng = (3, max(1, count - 5)) if ranged else None
    for iters in (0, 3):
        kw = dict(iters=iters, count=count, range2=rng)
        plain = V.icp_points_host(xyz, nrm, depth, CAM, SCALE, start, DIST_M, residuals=np.full(len(xyz), 42.0, np.float32), **kw)
        robust = V.icp_points_robust_host(xyz, nrm, depth, CAM, SCALE, start, DIST_M, residuals=np.full(len(xyz), 42.0, np.float32), **kw)
        for key in ("pose", "sums29", "residuals"):
            assert np.array_equal(bits(robust[key]), bits(plain[key])), key
        assert robust["stats"].tobytes() == plain["stats"].tobytes()
        g = robust["gate_counts"]
        assert g[2] == plain["stats"]["matched"] == g[1] and g[3] == 0 and g[0] >= g[1]


# ------------------------------------------------------------------------------------------------------------ 2. the gates against float64
EVAL_POSES = [V.iso_mul(P_TRUE, pose_from_xi(xi)) for xi in
              ([0.0002, 0.009, -0.0071, 0.0072, -0.003, -0.0012], [-0.0059, -0.0048, 0.005, -0.0035, -0.0002, 0.0077], [0.002, -0.0005, 0.0003, -0.0019, 0.001, 0.0002])]
GATE_DIST_M = 0.05  # (inside the ramp's +- 60 mm, so that the distance gate rejects a part of it and the normal gate the rest)


@pytest.mark.parametrize("k", range(len(EVAL_POSES)))
def test_gates_against_float64(model, frames, k):
    xyz, nrm = model
    depth, fn = frames["both"]
    pose = EVAL_POSES[k]
    ref = robust64(xyz, nrm, pose, depth, fn, MIN_COS, HUBER_M, GATE_DIST_M)
    assert int(ref["doubtful"].sum()) == 0, "choose another pose: the float64 side itself has points at a decision"
    out = V.icp_points_robust_host(xyz, nrm, depth, CAM, SCALE, pose, GATE_DIST_M, iters=0, frame_normals=fn, min_cos=MIN_COS, huber_m=HUBER_M)
    got = ~np.isnan(out["residuals"])
    want = [int(ref[key].sum()) for key in ("with_depth", "within", "matched", "linear")]
    print(f"pose {k}: considered {len(xyz)}, gate counts {out['gate_counts'].tolist()}")
    assert np.array_equal(got, ref["matched"])  # NaN exactly off the matched set
    assert out["gate_counts"].tolist() == want and out["stats"]["matched"] == want[2] and out["sums29"][1] == float(want[2])
    assert len(xyz) > want[0] > want[1] > want[2] > want[3] > 0  # every gate rejects something the one before let through
    s64 = ref["terms"].sum(0)
    mag = magnitudes(ref, HUBER_M)
    s32 = np.delete(out["sums29"], 1).astype(np.float64)
    rel = np.abs(s32 - s64) / np.where(mag > 0, mag, 1.0)
    print(f"pose {k}: largest |s32 - s64| / magnitude = {rel.max():.3g}")
    assert rel.max() <= SUM_REL_BOUND
    assert np.abs(out["residuals"][got] - ref["rows"][got, 0]).max() < 1e-5  # the raw r, unweighted
    assert np.isclose(out["stats"]["rms"], np.sqrt(ref["loss"][ref["matched"]].sum() / want[2]), rtol=1e-5)  # the Huber loss


# ------------------------------------------------------------------------------------------------------------ 3. the tree
def rows32(xyz, nrm, pose, residuals):
    """The entry's own rows in float32: its residuals and the Jacobian rows of the rule with lie.h's operand order."""
    f = np.float32
    t, q = pose[:3].astype(f), pose[3:].astype(f)
    cu, cv, fu, fv, skew = [f(v) for v in CAM]

    def rotate_conj(p):
        qv = np.broadcast_to(-q[:3], p.shape)
        tt = cross(qv, p) * f(2.0)
        return (tt * q[3] + cross(qv, tt)) + p

    with np.errstate(all="ignore"):
        c = rotate_conj(xyz + -t)
        pu = (fu * c[:, 0] + skew * c[:, 1]) + cu * c[:, 2]
        pv = fv * c[:, 1] + cv * c[:, 2]
        x0, y0 = np.floor(pu / c[:, 2] + f(0.5)), np.floor(pv / c[:, 2] + f(0.5))
    m = ~np.isnan(residuals)
    return m, x0, y0, rotate_conj(nrm)


@pytest.mark.parametrize("count", COUNTS)
def test_order_of_the_sums(model, frames, count):
    xyz, nrm = model
    depth, fn = frames["both"]
    pose = EVAL_POSES[2]
    f = np.float32
    out = V.icp_points_robust_host(xyz, nrm, depth, CAM, SCALE, pose, DIST_M, iters=0, count=count, frame_normals=fn, min_cos=MIN_COS,
                                   huber_m=HUBER_M)
    res = out["residuals"][:count]
    m, x0, y0, n = rows32(xyz[:count], nrm[:count], pose, res)
    cu, cv, fu, fv, skew = [f(v) for v in CAM]
    xi, yi = np.where(m, x0, 0).astype(np.int64), np.where(m, y0, 0).astype(np.int64)
    z = f(1.0) / (f(SCALE) / np.where(m, depth[yi, xi], 1).astype(f))
    qy = (yi.astype(f) - cv) * z / fv
    qx = ((xi.astype(f) - cu) * z - skew * qy) / fu
    J = np.concatenate([n, cross(np.stack([qx, qy, z], -1), n)], -1)
    a = np.where(m[:, None], np.concatenate([res[:, None], J], -1), f(0.0)).astype(f)
    r = a[:, 0]
    ar = np.abs(r)
    lin = ar <= f(HUBER_M)
    with np.errstate(all="ignore"):
        w = np.where(lin, f(1.0), f(HUBER_M) / ar).astype(f)
    e = np.where(lin, r * r, f(HUBER_M) * (f(2.0) * ar - f(HUBER_M))).astype(f)
    want = tree32(products(a, w, w * r, e).astype(f), count)
    assert np.array_equal(bits(np.delete(out["sums29"], 1)), bits(want))
    assert np.isnan(out["residuals"][count:]).all() and out["gate_counts"][3] == int((~lin).sum())


# ------------------------------------------------------------------------------------------------------------ 4. it helps
def exp64(xi):
    v, w = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K, v.copy()
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th**2 * K @ K
    Vm = np.eye(3) + (1 - np.cos(th)) / th**2 * K + (th - np.sin(th)) / th**3 * K @ K
    return R, Vm @ v


def rot_of(q):
    i, j, k, w = [float(x) for x in q / np.linalg.norm(q)]
    return np.array([[1 - 2 * (j * j + k * k), 2 * (i * j - k * w), 2 * (i * k + j * w)],
                     [2 * (i * j + k * w), 1 - 2 * (i * i + k * k), 2 * (j * k - i * w)],
                     [2 * (i * k - j * w), 2 * (j * k + i * w), 1 - 2 * (i * i + j * j)]])


def quat_of(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2  # (rotations far from pi only)
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def irls64(xyz, nrm, pose, depth, fn, min_cos, huber_m, iters):
    """The loop of vors_icp_points_robust in float64: evaluate, solve the weighted normal equations, T <- T * exp(delta)^-1."""
    R, t = rot_of(pose[3:].astype(np.float64)), pose[:3].astype(np.float64)
    for _ in range(iters):
        o = robust64(xyz, nrm, np.concatenate([t, quat_of(R)]), depth, fn, min_cos, huber_m)
        a, w = o["rows"], o["w"]
        H, g = (a[:, 1:] * w[:, None]).T @ a[:, 1:], a[:, 1:].T @ (w * a[:, 0])
        Rd, td = exp64(np.linalg.solve(H, g))
        R, t = R @ Rd.T, t - R @ Rd.T @ td  # T * (Rd, td)^-1
    return np.concatenate([t, quat_of(R)])


def pose_errors(pose, truth):
    dt = np.linalg.norm(pose[:3].astype(np.float64) - truth[:3])
    Rrel = rot_of(pose[3:].astype(np.float64)).T @ rot_of(truth[3:].astype(np.float64))
    return dt, np.degrees(np.arccos(np.clip((np.trace(Rrel) - 1) / 2, -1, 1)))


START = pose_from_xi([0.004, -0.003, 0.005, 0.004, -0.005, 0.003])  # a few millimetres and tenths of a degree
ITERS = 10
REMEDY = {"step": dict(frame_normals=False, huber_m=HUBER_M), "ramp": dict(frame_normals=True, huber_m=0.0)}


@pytest.mark.parametrize("kind", list(REMEDY))
def test_it_helps(model, frames, kind):
    xyz, nrm = model
    depth, normals = frames[kind]
    fn = normals if REMEDY[kind]["frame_normals"] else None
    huber_m = REMEDY[kind]["huber_m"]
    start = V.iso_mul(P_TRUE, START)
    kw = dict(iters=ITERS, step_eps=0.0)
    plain = V.icp_points_host(xyz, nrm, depth, CAM, SCALE, start, DIST_M, **kw)
    robust = V.icp_points_robust_host(xyz, nrm, depth, CAM, SCALE, start, DIST_M, frame_normals=fn, min_cos=MIN_COS, huber_m=huber_m, **kw)
    assert plain["stats"]["iterations"] == robust["stats"]["iterations"] == ITERS
    tp, rp = pose_errors(plain["pose"], P_TRUE)
    tr, rr = pose_errors(robust["pose"], P_TRUE)
    # the condition on the scene, in float64 on both sides: the remedy is worth a factor of 4 at least
    p64 = irls64(xyz, nrm, start, depth, None, 0.0, 0.0, ITERS)
    r64 = irls64(xyz, nrm, start, depth, fn, MIN_COS, huber_m, ITERS)
    tp64, rp64 = pose_errors(p64, P_TRUE)
    tr64, rr64 = pose_errors(r64, P_TRUE)
    r64 = r64 if r64[6] * robust["pose"][6] >= 0 else np.concatenate([r64[:3], -r64[3:]])
    diff = np.abs(robust["pose"].astype(np.float64) - r64).max()
    print(f"{kind}: plain {tp:.3g} m / {rp:.3g} deg, robust {tr:.3g} m / {rr:.3g} deg: ratios {tp / tr:.3g} / {rp / rr:.3g}; float64 "
          f"{tp64 / tr64:.3g} / {rp64 / rr64:.3g}; gate counts {robust['gate_counts'].tolist()}; |pose32 - pose64| = {diff:.3g}")
    assert tp64 >= 4 * tr64 and rp64 >= 4 * rr64, "the scene does not show the remedy"
    assert tr < 0.5 * tp and rr < 0.5 * rp
    assert diff <= POSE_DIFF_BOUND
    g = robust["gate_counts"]
    assert (g[2] < g[1]) if fn is not None else (0 < g[3] < g[2])  # the remedy under test is the one at work
