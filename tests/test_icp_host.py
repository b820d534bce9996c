"""Point-to-plane ICP on the host (vors_icp_points_host; needs no GPU): lie.h icp_landing / icp_row / icp_products / icp_round and the
fixed order of the sums, the texts the kernels run.

The scene is a corner: three mutually non-parallel planes seen in one 48x64 depth map at scale 5000, with some zeros; the model is its
back-projection through a pose P (camera_back_project), the normals are depth_normals_host's with the same pose.

`rule(dtype)` below is ONE numpy statement of the per-point rule with the operand order of lie.h: in float64 it is the reference the
evaluator is held against, in float32 it reproduces the host entry's Jacobian rows bit for bit (numpy rounds every operation to the
array's type and fuses nothing).

Measured here (recorded in profiles/icp_summary.md as well):

  evaluator: the 28 sums against float64 with plain np.sum, in units of the float32 epsilon times the magnitudes eval64() states (every
      product a relative eps; r = n . (q - c) an ABSOLUTE eps |q|, being a difference of vectors of length |q|: relative to the sums
      themselves there is no bound, g cancels to nothing at the solution). Largest over the sums, per pose: 0.761, 0.483, 0.638, 0.793.
      MEASURED_SUM_ERR = 0.794; asserted at 4 x that.
  convergence: |pose32 - pose64| over the 7 numbers, per start: 4.11e-08 5.57e-08 2.58e-08 5.57e-08 4.25e-08 5.57e-08 2.58e-08 2.58e-08.
      MEASURED_POSE_DIFF = 5.6e-08; asserted at 4 x that.
  errors against P at the end (printed by test_convergence, NOT bounded). The frame aligned against is the map the model was made from,
      so the residual at P is zero and the depth quantisation leaves nothing: every start ends within what a float32 pose resolves,
      translation 0 .. 6.2e-08 m, rotation 0 .. 1.8e-06 degrees, after 2 or 3 updates (starts: 20 mm or 1 degree, two mixed).
"""
import numpy as np
import pytest

import vors_amd as V

SCALE = 5000.0
ROWS, COLS = 48, 64
CAM = np.array([31.5, 23.5, 60.0, 61.0, 0.0], np.float32)
DIST_M = 0.1
MEASURED_SUM_ERR = 0.794  # in eps x magnitude: the docstring
SUM_REL_BOUND = 4 * MEASURED_SUM_ERR
MEASURED_POSE_DIFF = 5.6e-08
POSE_DIFF_BOUND = 4 * MEASURED_POSE_DIFF
PLANES = (((0.5, 0.0, 1.0), 2.0), ((-0.5, 0.1, 1.0), 2.0), ((0.0, -0.6, 1.0), 2.2))


def corner_depth(rows=ROWS, cols=COLS, cam=CAM, scale=SCALE):
    cu, cv, fu, fv, skew = [float(v) for v in cam]
    x, y = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    ry = (y - cv) / fv
    rx = ((x - cu) - skew * ry) / fu
    z = np.min([dist / (n[0] * rx + n[1] * ry + n[2]) for n, dist in PLANES], axis=0)
    d = np.rint(z * scale)
    assert d.min() >= 1 and d.max() <= 65535
    d = d.astype(np.uint16)
    d.reshape(-1)[::37] = 0  # some pixels without depth
    return d


def pose_from_xi(xi):
    out = np.zeros(7, np.float32)
    V.lib().vors_se3_exp(V._ptr(np.ascontiguousarray(xi, np.float32)), V._ptr(out))
    return out


def model_of(depth, pose, cam=CAM, scale=SCALE):
    """The list of a depth map's pixels with depth, in the world frame of `pose`: (xyz [m, 3], normals [m, 3])."""
    rows, cols = depth.shape
    ys, xs = np.nonzero(depth)
    xy = np.stack([xs, ys], -1).astype(np.float32)
    z = (np.float32(1.0) / (np.float32(scale) / depth[ys, xs].astype(np.float32))).astype(np.float32)
    xyz = V.camera_back_project(cam, pose, xy, z)
    nrm = V.depth_normals_host(depth, cam, scale, 2, 0.05, pose7=pose)["normals"][ys, xs]
    return np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(nrm, np.float32)


P_TRUE = pose_from_xi([0.3, -0.2, 0.1, 0.05, -0.1, 0.08])


@pytest.fixture(scope="module")
def scene():
    depth = corner_depth()
    xyz, nrm = model_of(depth, P_TRUE)
    assert len(xyz) > 2600 and (np.abs(nrm).sum(-1) > 0).mean() > 0.9
    return depth, xyz, nrm


def icp(scene, pose, **kw):
    depth, xyz, nrm = scene
    kw.setdefault("iters", 0)
    return V.icp_points_host(xyz, nrm, depth, CAM, SCALE, pose, DIST_M, **kw)


# ------------------------------------------------------------------------------------------------------------ the rule, once, for two types
def rule(dtype, xyz, nrm, pose, depth, cam=CAM, scale=SCALE):
    """lie.h icp_landing + icp_row without the distance gate, operand order kept -> dict of per-point arrays."""
    f = dtype
    w, nw = xyz.astype(f), nrm.astype(f)
    t, q = pose[:3].astype(f), pose[3:].astype(f)
    cu, cv, fu, fv, skew = [f(v) for v in cam]
    rows, cols = depth.shape

    def cross(a, b):
        return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                         a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)

    def dot3(a, b):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]

    def rotate_conj(p):  # quat_rotate(conj(q), p)
        qv = np.broadcast_to(-q[:3], p.shape)
        tt = cross(qv, p) * f(2.0)
        return (tt * q[3] + cross(qv, tt)) + p

    with np.errstate(all="ignore"):
        c = rotate_conj(w + -t)
        pu = (fu * c[:, 0] + skew * c[:, 1]) + cu * c[:, 2]
        pv = fv * c[:, 1] + cv * c[:, 2]
        u, v = pu / c[:, 2], pv / c[:, 2]
        x0, y0 = np.floor(u + f(0.5)), np.floor(v + f(0.5))
        lands = (c[:, 2] > 0) & (x0 >= 0) & (x0 < cols) & (y0 >= 0) & (y0 < rows)
        xi, yi = np.where(lands, x0, 0).astype(np.int64), np.where(lands, y0, 0).astype(np.int64)
        d = depth[yi, xi]
        has_normal = ~((nw == 0).all(-1))
        usable = lands & has_normal & (d != 0)
        z = f(1.0) / (f(scale) / np.where(usable, d, 1).astype(f))
        qy = (yi.astype(f) - cv) * z / fv
        qx = ((xi.astype(f) - cu) * z - skew * qy) / fu
        qq = np.stack([qx, qy, z], -1)
        e = qq - c
        n = rotate_conj(nw)
        J = np.concatenate([n, cross(qq, n)], -1)
        frac_u, frac_v = (u + f(0.5)) - x0, (v + f(0.5)) - y0
        edge = np.minimum(np.minimum(frac_u, 1 - frac_u), np.minimum(frac_v, 1 - frac_v))
    return dict(usable=usable, dist2=dot3(e, e), r=dot3(n, e), J=J, edge=np.where(c[:, 2] > 0, edge, 1.0), q_norm=np.sqrt(dot3(qq, qq)))


def products(a):
    """lie.h icp_products for rows a [m, 7] -> [m, 28]."""
    cols = [a[:, 0] * a[:, 0]] + [a[:, i] * a[:, 0] for i in range(1, 7)]
    cols += [a[:, i] * a[:, j] for i in range(1, 7) for j in range(i, 7)]
    return np.stack(cols, -1)


def eval64(scene, pose, first=0, count=None):
    depth, xyz, nrm = scene
    last = len(xyz) if count is None else first + count
    o = rule(np.float64, xyz[first:last], nrm[first:last], pose, depth)
    dist = np.sqrt(o["dist2"])
    matched = o["usable"] & (dist <= DIST_M)
    doubtful = (o["edge"] < 1e-4) | (o["usable"] & (np.abs(dist - DIST_M) < 1e-4))
    rows7 = np.where(matched[:, None], np.concatenate([o["r"][:, None], o["J"]], -1), 0.0)
    # What a forward error of the sums is measured against, in units of the float32 epsilon: every product carries a relative error of
    # the order of eps, and r = n . (q - c) is a difference of vectors of length |q|, so it carries an ABSOLUTE error of the order of
    # eps |q| however small it is itself. Per point: |J_i J_j|; |J_i| (|r| + |q|); r r + 2 |r| |q| + eps |q|^2.
    eps = float(np.finfo(np.float32).eps)
    mags = np.abs(rows7)
    qn = np.where(matched, o["q_norm"], 0.0)
    mags[:, 0] += qn
    magnitude = products(mags).sum(0)
    magnitude[0] = (rows7[:, 0] ** 2 + 2 * np.abs(rows7[:, 0]) * qn + eps * qn * qn).sum()
    magnitude *= eps
    return dict(matched=matched, doubtful=doubtful, rows=rows7, terms=products(rows7), magnitude=magnitude)


EVAL_POSES = [P_TRUE] + [V.iso_mul(P_TRUE, pose_from_xi(xi)) for xi in
                         ([0.02, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0.0175, 0], [0.01, -0.015, 0.02, 0.01, 0.005, -0.012])]


def test_jacobian_rule():
    """J = (n, cross(q, n)) is the derivative of n . (exp(xi) q - c) at xi = 0 in se3_exp's order, by central differences in float64."""
    rng = np.random.default_rng(5)
    n, q, c = rng.normal(size=3), rng.normal(size=3) + [0, 0, 2], rng.normal(size=3)
    J = np.concatenate([n, np.cross(q, n)])

    def moved(xi):
        v, w = xi[:3], xi[3:]
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th**2 * K @ K if th > 0 else np.eye(3)
        Vm = np.eye(3) + (1 - np.cos(th)) / th**2 * K + (th - np.sin(th)) / th**3 * K @ K if th > 0 else np.eye(3)
        return n @ (R @ q + Vm @ v - c)

    h = 1e-6
    num = np.array([(moved(h * np.eye(6)[i]) - moved(-h * np.eye(6)[i])) / (2 * h) for i in range(6)])
    assert np.abs(num - J).max() < 1e-8
    # ... and se3_exp reads (v, w) in that order: its translation for a pure v is v
    assert np.allclose(pose_from_xi([0.1, 0.2, 0.3, 0, 0, 0])[:3], [0.1, 0.2, 0.3])


@pytest.mark.parametrize("k", range(len(EVAL_POSES)))
def test_evaluator_against_float64(scene, k):
    pose = EVAL_POSES[k]
    ref = eval64(scene, pose)
    assert int(ref["doubtful"].sum()) == 0, "choose another pose: the float64 side itself has points at a decision"
    out = icp(scene, pose)
    got = ~np.isnan(out["residuals"])
    assert int(out["stats"]["matched"]) == int(ref["matched"].sum()) == int(got.sum()) and int(ref["matched"].sum()) > 2000
    assert np.array_equal(got, ref["matched"])  # NaN exactly off the matched set
    assert int(out["stats"]["considered"]) == len(ref["matched"]) and out["sums29"][1] == float(got.sum())
    s64 = ref["terms"].sum(0)
    mag = ref["magnitude"]
    s32 = np.delete(out["sums29"], 1).astype(np.float64)
    rel = np.abs(s32 - s64) / np.where(mag > 0, mag, 1.0)
    print(f"pose {k}: matched {got.sum()}, largest |s32 - s64| / magnitude = {rel.max():.3g}")
    assert rel.max() <= SUM_REL_BOUND
    assert np.abs(out["residuals"][got] - ref["rows"][got, 0]).max() < 1e-5
    assert out["stats"]["status"] == V.ICP_ITERATIONS and out["stats"]["iterations"] == 0
    assert np.array_equal(out["pose"].view(np.uint32), pose.view(np.uint32))


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


def rows32(scene, pose, residuals, first, last):
    depth, xyz, nrm = scene
    o = rule(np.float32, xyz[first:last], nrm[first:last], pose, depth)
    res = residuals[first:last]
    m = ~np.isnan(res)
    a = np.concatenate([res[:, None], o["J"]], -1).astype(np.float32)
    return np.where(m[:, None], a, np.float32(0.0)).astype(np.float32)


@pytest.mark.parametrize("count", [1, 1023, 1024, 1025, 2500])
def test_order_of_the_sums(scene, count):
    depth, xyz, nrm = scene
    pose = EVAL_POSES[3]
    out = icp(scene, pose, count=count)
    a = rows32(scene, pose, out["residuals"], 0, count)
    want = tree32(products(a), count)
    assert np.array_equal(np.delete(out["sums29"], 1).view(np.uint32), want.view(np.uint32))
    assert np.isnan(out["residuals"][count:]).all()
    # another capacity: the same bits
    cap = count + 77
    big = V.icp_points_host(np.concatenate([xyz[:count], np.ones((77, 3), np.float32)]), np.concatenate([nrm[:count], np.ones((77, 3), np.float32)]),
                            depth, CAM, SCALE, pose, DIST_M, iters=0, count=count)
    assert len(big["residuals"]) == cap
    assert np.array_equal(big["sums29"].view(np.uint32), out["sums29"].view(np.uint32))
    assert big["stats"] == out["stats"]


def test_a_range_is_the_list_of_its_points(scene):
    depth, xyz, nrm = scene
    pose = EVAL_POSES[3]
    sentinel = np.full(len(xyz), 42.0, np.float32)
    ranged = icp(scene, pose, range2=(7, 1500), residuals=sentinel, iters=3)
    own = V.icp_points_host(xyz[7:1507], nrm[7:1507], depth, CAM, SCALE, pose, DIST_M, iters=3)
    for key in ("pose", "sums29"):
        assert np.array_equal(ranged[key].view(np.uint32), own[key].view(np.uint32)), key
    assert ranged["stats"] == own["stats"] and ranged["stats"]["considered"] == 1500
    assert np.array_equal(ranged["residuals"][7:1507].view(np.uint32), own["residuals"].view(np.uint32))
    assert (ranged["residuals"][:7] == 42.0).all() and (ranged["residuals"][1507:] == 42.0).all()  # exactly the ranks of the range


# ------------------------------------------------------------------------------------------------------------ convergence
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


def gauss_newton64(scene, pose, step_eps, iters):
    """The loop of vors_icp_points in float64: evaluate, solve, T <- T * exp(delta)^-1."""
    R, t = rot_of(pose[3:].astype(np.float64)), pose[:3].astype(np.float64)
    for _ in range(iters):
        ref = eval64(scene, np.concatenate([t, quat_of(R)]))
        a = ref["rows"]
        H, g = a[:, 1:].T @ a[:, 1:], a[:, 1:].T @ a[:, 0]
        delta = np.linalg.solve(H, g)
        Rd, td = exp64(delta)
        R, t = R @ Rd.T, t - R @ Rd.T @ td  # T * (Rd, td)^-1
        if delta @ delta <= step_eps * step_eps:
            break
    return np.concatenate([t, quat_of(R)])


def pose_errors(pose, truth):
    dt = np.linalg.norm(pose[:3].astype(np.float64) - truth[:3])
    Rrel = rot_of(pose[3:].astype(np.float64)).T @ rot_of(truth[3:].astype(np.float64))
    return dt, np.degrees(np.arccos(np.clip((np.trace(Rrel) - 1) / 2, -1, 1)))


STARTS = [np.eye(6)[i] * (0.02 if i < 3 else np.radians(1.0)) for i in range(6)] + [np.array([0.012, -0.01, 0.015, 0.008, -0.01, 0.006]),
                                                                                   np.array([-0.015, 0.01, 0.008, -0.006, 0.012, 0.01])]
STEP_EPS, ITERS = 2e-5, 40
T_RES, R_RES = 1e-6, 1e-4  # metres, degrees: a few units in the last place of |t| = 0.4 and of a unit quaternion's components


@pytest.mark.parametrize("k", range(len(STARTS)))
def test_convergence(scene, k):
    start = V.iso_mul(P_TRUE, pose_from_xi(STARTS[k]))
    out = icp(scene, start, iters=ITERS, step_eps=STEP_EPS)
    st = out["stats"]
    assert st["status"] == V.ICP_CONVERGED and 0 < st["iterations"] <= ITERS and st["last_step_norm"] <= STEP_EPS
    t0, r0 = pose_errors(start, P_TRUE)
    t1, r1 = pose_errors(out["pose"], P_TRUE)
    want = gauss_newton64(scene, start, STEP_EPS, ITERS)
    want = want if want[6] * out["pose"][6] >= 0 else np.concatenate([want[:3], -want[3:]])
    diff = np.abs(out["pose"].astype(np.float64) - want).max()
    print(f"start {k}: {st['iterations']} updates, rms {st['rms']:.3g} m; translation {t0:.3g} -> {t1:.3g} m, rotation {r0:.3g} -> "
          f"{r1:.3g} deg; |pose32 - pose64| = {diff:.3g}")
    # each error strictly below the start's; a single-axis start has NO error in its other component (below T_RES / R_RES, what a
    # float32 pose of this size resolves), which can then only be held to that resolution
    assert t1 < t0 if t0 > T_RES else t1 <= T_RES
    assert r1 < r0 if r0 > R_RES else r1 <= R_RES
    assert diff <= POSE_DIFF_BOUND
    # the sums of the final evaluation give the information matrix unchanged
    info, cov, sigma2, flag = V.pose_information_from_sums(out["sums29"])
    assert np.isfinite(cov).all() and flag == 0 and info[0, 0] == out["sums29"][8]


# ------------------------------------------------------------------------------------------------------------ failure paths
def frontal_plane():
    depth = np.full((ROWS, COLS), 7500, np.uint16)
    ys, xs = np.nonzero(depth)
    xyz = V.camera_back_project(CAM, None, np.stack([xs, ys], -1).astype(np.float32), np.full(len(xs), np.float32(1.0) / (np.float32(SCALE) / np.float32(7500))))
    nrm = np.zeros_like(xyz)
    nrm[:, 2] = -1.0
    return depth, np.ascontiguousarray(xyz, np.float32), nrm


IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1], np.float32)


def test_singular_keeps_the_pose():
    depth, xyz, nrm = frontal_plane()
    out = V.icp_points_host(xyz, nrm, depth, CAM, SCALE, IDENTITY, DIST_M, iters=5)
    st = out["stats"]
    assert st["matched"] == ROWS * COLS and out["sums29"][8] == 0.0  # H[0][0]: a sum of exact zeros
    assert st["status"] == V.ICP_SINGULAR and st["iterations"] == 0 and st["last_step_norm"] == 0.0
    assert np.array_equal(out["pose"].view(np.uint32), IDENTITY.view(np.uint32))


def test_too_few_keeps_the_pose(scene):
    pose = EVAL_POSES[3]
    matched = int(icp(scene, pose)["stats"]["matched"])
    out = icp(scene, pose, iters=5, min_points=matched + 1)
    assert out["stats"]["status"] == V.ICP_TOO_FEW and out["stats"]["iterations"] == 0 and out["stats"]["matched"] == matched
    assert np.array_equal(out["pose"].view(np.uint32), pose.view(np.uint32))
    assert icp(scene, pose, iters=1, min_points=matched)["stats"]["iterations"] == 1


def test_no_normals_and_empty_lists_match_nothing(scene):
    depth, xyz, nrm = scene
    for out in (V.icp_points_host(xyz, np.zeros_like(nrm), depth, CAM, SCALE, P_TRUE, DIST_M, iters=2), icp(scene, P_TRUE, count=0, iters=2)):
        st = out["stats"]
        assert st["matched"] == 0 and st["status"] == V.ICP_TOO_FEW and np.isnan(st["rms"]) and np.isnan(out["residuals"]).all()
        assert np.array_equal(out["sums29"].view(np.uint32), np.zeros(29, np.float32).view(np.uint32))  # +0.0f everywhere
        assert np.array_equal(out["pose"].view(np.uint32), P_TRUE.view(np.uint32))
    assert icp(scene, P_TRUE, count=0)["stats"]["considered"] == 0
