"""The joint point-to-plane and photometric ICP on the host (vors_icp_points_joint_host; needs no GPU): lie.h icp_photo_footprint /
icp_row_photo beside icp_row_robust, in the loop and the order of sums of vors_icp_points_host.

Scenes, 48x64 at scale 5000 with tests/test_icp_robust_host.py's camera and P_TRUE:
  "plane"  ONE tilted plane (PLANES[0] alone) — the degenerate geometry of DESIGN.md 7n: point-to-plane rows leave the translation inside
           the plane and the rotation about its normal free — under a smooth texture (three sines of periods 16, 13 and 23 pixels, none
           below 10 pixels in either image direction), rounded to u8. The model is the back-projection of the clean frame through
           P_TRUE with depth_normals_host's normals and the frame's grey at each pixel.
  "corner" test_icp_robust_host.py's corner with its "both" patches, the same texture as its grey plane: the order-of-sums cases.

`joint64()` is ONE float64 numpy statement of the rule on top of test_icp_robust_host.robust64(); `loop64()` the loop around it. The Rust
reference has no ICP: that restatement is the yardstick.

PHOTO_SCALE_M = 0.5 mm per grey level: depth noise over grey noise, about 1 mm per 2 grey levels. The choice is NOT measured on real data.

Measured here (and recorded in DESIGN.md 7o):
  evaluator (corner, frame "both", MIN_COS 0.9, HUBER_M 2 mm, distance gate 50 mm, photo Huber 1.5 grey levels): photo counts per pose
      [2162, 1622], [2135, 1381], [2156, 1306] of 2261 matched; largest |s32 - s64| over the 28 sums in units of eps x magnitude
      (magnitudes() extended by the photometric products: photo_magnitudes()): 0.0258, 0.119, 0.105 — under test_icp_host.py's bound,
      4 x 0.794, which is therefore reused.
  it does what 7n lacked (plane, a start 10 mm inside the plane = 0.3 pixel, ITERS = 10, no Huber, no normal gate); the translation error
      against P_TRUE split into (along the plane's normal, inside the plane):
      start (0, 10 mm); the robust pass alone: its first update slides 6.45 m inside the plane (the system is singular up to rounding:
      point-to-plane rows of one plane hold three of the six directions), then nothing matches and the list freezes as TOO_FEW — the
      in-plane error is not reduced; joint pass, f32 twin (1.4e-05 mm, 3.0e-05 mm); float64 loop (3.2e-05 mm, 5.7e-05 mm) — both at the
      resolution of the float32 model, since the frame is the model's own. The photometric term removes the in-plane slide of 7n on the
      single-plane scene. |pose32 - pose64| over the 7 numbers: 6.44e-08; MEASURED_POSE_DIFF = 6.5e-08, asserted at 4 x that.
      IN_PLANE_BOUND_M = 0.1 mm: half the depth quantum of the frame (0.2 mm at scale 5000) and a hundredth of the start's offset — not
      taken from the code under test; the float64 loop meets it with a factor of 1700 to spare.
  photo Huber (plane, the frame's grey with a 14 x 18 patch raised by 70 grey levels, the same start): in-plane error after ITERS rounds
      without the weight 4.38 mm, with photo_huber_grey = 10: 0.836 mm; photo_counts (2462 used, 245 on the linear branch) equal the
      float64 counts.
"""
import numpy as np
import pytest

import vors_amd as V
from test_icp_robust_host import (CAM, COLS, COUNTS, DIST_M, EVAL_POSES, GATE_DIST_M, HUBER_M, MIN_COS, PLANES, P_TRUE, ROWS, SCALE, SUM_REL_BOUND,
                                  bits, corner_z, cross, dot3, exp64, frame_normals_of, magnitudes, patched, pose_from_xi, products, quat_of,
                                  robust64, rot_of, to_depth, tree32)

PHOTO_SCALE_M = 0.0005
PHOTO_HUBER_GREY = 10.0
EVAL_PHOTO_HUBER_GREY = 1.5  # (the evaluator cases: low enough for both branches of the weight at every pose, the closest included)
MEASURED_POSE_DIFF = 6.5e-08  # the docstring
POSE_DIFF_BOUND = 4 * MEASURED_POSE_DIFF
IN_PLANE_BOUND_M = 1e-4  # half the frame's depth quantum, a hundredth of the start's offset (the docstring)
ITERS = 10


# ------------------------------------------------------------------------------------------------------------ the scenes
def texture(rows=ROWS, cols=COLS):
    x, y = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    g = 128 + 50 * np.sin(2 * np.pi * x / 16 + 0.3) + 40 * np.sin(2 * np.pi * y / 13 + 1.1) + 25 * np.sin(2 * np.pi * (x + y) / 23)
    return np.rint(g).astype(np.uint8)


def plane_z():
    cu, cv, fu, fv, skew = [float(v) for v in CAM]
    x, y = np.meshgrid(np.arange(COLS, dtype=np.float64), np.arange(ROWS, dtype=np.float64))
    ry = (y - cv) / fv
    rx = ((x - cu) - skew * ry) / fu
    n, dist = PLANES[0]
    return dist / (n[0] * rx + n[1] * ry + n[2])


def model_of(depth, gray):
    """The list of the frame's pixels with depth in the world frame of P_TRUE: (xyz, normals, grey)."""
    ys, xs = np.nonzero(depth)
    xy = np.stack([xs, ys], -1).astype(np.float32)
    z = (np.float32(1.0) / (np.float32(SCALE) / depth[ys, xs].astype(np.float32))).astype(np.float32)
    xyz = V.camera_back_project(CAM, P_TRUE, xy, z)
    nrm = V.depth_normals_host(depth, CAM, SCALE, 2, 0.05, pose7=P_TRUE)["normals"][ys, xs]
    return np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(nrm, np.float32), np.ascontiguousarray(gray[ys, xs])


@pytest.fixture(scope="module")
def plane():
    depth, gray = to_depth(plane_z()), texture()
    xyz, nrm, g = model_of(depth, gray)
    assert len(xyz) > 2900 and (np.abs(nrm).sum(-1) > 0).mean() > 0.8
    return dict(xyz=xyz, nrm=nrm, gray=g, depth=depth, frame_gray=gray)


@pytest.fixture(scope="module")
def corner():
    gray = texture()
    xyz, nrm, g = model_of(to_depth(corner_z()), gray)
    depth = patched("both")
    return dict(xyz=xyz, nrm=nrm, gray=g, depth=depth, frame_gray=gray, fn=frame_normals_of(depth))


def joint_host(s, pose, dist_m=DIST_M, **kw):
    return V.icp_points_joint_host(s["xyz"], s["nrm"], s["gray"], s["depth"], s["frame_gray"], CAM, SCALE, pose, dist_m, **kw)


# ------------------------------------------------------------------------------------------------------------ the rule in float64
def camera_points64(xyz, pose):
    f = np.float64
    t, q = pose[:3].astype(f), pose[3:].astype(f)
    p = xyz.astype(f) - t
    qv = np.broadcast_to(-q[:3], p.shape)
    tt = cross(qv, p) * 2.0
    return (tt * q[3] + cross(qv, tt)) + p


def photo_rows64(c, gray_w, G, scale):
    """The photometric rule for camera-frame points c [m, 3] in float64 -> inside, rows [m, 7], d = I - grey, and what the error model
    needs. Points whose footprint is not inside have rows of zeros."""
    f = np.float64
    cu, cv, fu, fv, skew = [f(v) for v in CAM]
    rows, cols = G.shape
    with np.errstate(all="ignore"):
        x, y, z = c[:, 0], c[:, 1], c[:, 2]
        u = ((fu * x + skew * y) + cu * z) / z
        v = (fv * y + cv * z) / z
        x0, y0 = np.floor(u), np.floor(v)
        inside = (x0 >= 0) & (x0 + 1 <= cols - 1) & (y0 >= 0) & (y0 + 1 <= rows - 1)
        xi, yi = np.where(inside, x0, 0).astype(np.int64), np.where(inside, y0, 0).astype(np.int64)
        fx, fy = np.where(inside, u - x0, 0.0), np.where(inside, v - y0, 0.0)
        i00, i10, i01, i11 = [G[np.minimum(yi + dy, rows - 1), np.minimum(xi + dx, cols - 1)].astype(f) for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1))]
        top, bot = i00 + fx * (i10 - i00), i01 + fx * (i11 - i01)
        im = top + fy * (bot - top)
        gx = (1 - fy) * (i10 - i00) + fy * (i11 - i01)
        gy = (1 - fx) * (i01 - i00) + fx * (i11 - i10)
        d = im - gray_w.astype(f)
        iz = 1.0 / np.where(inside, z, 1.0)
        du = np.stack([fu * iz, skew * iz, -(fu * x + skew * y) * iz * iz], -1)
        dv = np.stack([np.zeros_like(iz), fv * iz, -(fv * y) * iz * iz], -1)
        a = scale * (gx[:, None] * du + gy[:, None] * dv)
        row = np.concatenate([(scale * d)[:, None], -a, cross(a, c)], -1)
        # the distance of (u, v) from the decision "the footprint is inside", in pixels (a point with z <= 0 is never matched)
        border = np.minimum(np.minimum(np.abs(u), np.abs(u - (cols - 1))), np.minimum(np.abs(v), np.abs(v - (rows - 1))))
        # the absolute error of r_p in units of eps: the roundings of I and grey, and (u, v)'s own error through the gradient
        r_err = scale * (np.abs(im) + gray_w.astype(f) + 4.0 * (np.abs(gx) * np.abs(u) + np.abs(gy) * np.abs(v)))
    return dict(inside=inside, rows=np.where(inside[:, None], row, 0.0), d=d, border=border, r_err=np.where(inside, r_err, 0.0))


def joint64(s, pose, fn, min_cos, huber_m, scale, photo_huber_grey, dist_m=DIST_M):
    """The rule of vors_icp_points_joint for every point of a scene's list at `pose` in float64: robust64()'s dict, and photo, photo_linear,
    the photometric rows and weights, the 28 products per point (geometric + photometric) and `doubtful` extended by the new decisions."""
    o = robust64(s["xyz"], s["nrm"], pose, s["depth"], fn, min_cos, huber_m, dist_m)
    ph = photo_rows64(camera_points64(s["xyz"], pose), s["gray"], s["frame_gray"], scale)
    photo = o["matched"] & ph["inside"] & (scale > 0)
    a = np.where(photo[:, None], ph["rows"], 0.0)
    hub = scale * photo_huber_grey
    r = a[:, 0]
    ar = np.abs(r)
    lin = ar <= hub if hub > 0 else np.ones(len(r), bool)
    w = np.where(lin, 1.0, hub / np.where(lin, 1.0, ar))
    loss = np.where(lin, r * r, hub * (2.0 * ar - hub))
    doubtful = o["doubtful"] | (o["matched"] & (ph["border"] < 1e-4))
    if hub > 0:
        doubtful |= photo & (np.abs(ar / hub - 1.0) < 1e-4)
    o.update(photo=photo, photo_linear=photo & ~lin, photo_rows=a, photo_w=w, photo_loss=loss, photo_lin=lin, doubtful=doubtful,
             photo_d=np.where(photo, ph["d"], np.nan), photo_r_err=np.where(photo, ph["r_err"], 0.0),
             joint_terms=o["terms"] + np.where(photo[:, None], products(a, w, w * r, loss), 0.0))
    return o


def photo_magnitudes(o, hub):
    """test_icp_robust_host.magnitudes() for the photometric products: the same model with r_p's absolute error (photo_rows64's r_err, in
    units of eps) in |q|'s place — r_p = s (I - grey) carries the roundings of I and of the grey level and the error of (u, v) through the
    gradient, as r = n . (q - c) carries |q|'s."""
    return magnitudes(dict(rows=o["photo_rows"], q_norm=o["photo_r_err"], w=o["photo_w"], lin=o["photo_lin"], loss=o["photo_loss"]), hub)


def loop64(s, pose, fn, min_cos, huber_m, scale, photo_huber_grey, iters):
    """The loop of vors_icp_points_joint in float64: evaluate, solve the weighted normal equations of both rows, T <- T * exp(delta)^-1."""
    R, t = rot_of(pose[3:].astype(np.float64)), pose[:3].astype(np.float64)
    for _ in range(iters):
        o = joint64(s, np.concatenate([t, quat_of(R)]), fn, min_cos, huber_m, scale, photo_huber_grey)
        H, g = np.zeros((6, 6)), np.zeros(6)
        for a, w in ((o["rows"], o["w"]), (o["photo_rows"], o["photo_w"])):
            H += (a[:, 1:] * w[:, None]).T @ a[:, 1:]
            g += a[:, 1:].T @ (w * a[:, 0])
        Rd, td = exp64(np.linalg.solve(H, g))
        R, t = R @ Rd.T, t - R @ Rd.T @ td  # T * (Rd, td)^-1
    return np.concatenate([t, quat_of(R)])


def plane_normal_world():
    n = np.array(PLANES[0][0], np.float64)
    return rot_of(P_TRUE[3:].astype(np.float64)) @ (n / np.linalg.norm(n))


def split_error(pose):
    """The translation error against P_TRUE -> (along the plane's normal, inside the plane), metres."""
    dt = pose[:3].astype(np.float64) - P_TRUE[:3].astype(np.float64)
    n = plane_normal_world()
    along = dt @ n
    return abs(along), np.linalg.norm(dt - along * n)


def in_plane_start(metres=0.010):
    """P_TRUE composed with a translation inside the plane (camera frame: perpendicular to the plane's normal)."""
    n = np.array(PLANES[0][0], np.float64)
    n /= np.linalg.norm(n)
    e1 = np.array([0.0, 1.0, 0.0])  # (the normal has no y component)
    e2 = np.cross(n, e1)
    d = 0.6 * e1 + 0.8 * e2
    assert abs(d @ n) < 1e-12 and abs(np.linalg.norm(d) - 1) < 1e-12
    return V.iso_mul(P_TRUE, pose_from_xi(np.concatenate([metres * d, np.zeros(3)])))


# ------------------------------------------------------------------------------------------------------------ 1. the Jacobian rule
def test_jacobian_rule():
    """J_p = (-a, cross(a, c)) with a = s (gx du/dc + gy dv/dc) is the derivative of s (I(project(exp(xi)^-1 c)) - grey) at xi = 0 in
    se3_exp's order — the camera moves to T exp(xi) —, by central differences in float64 through the bilinear interpolant itself."""
    G = texture()
    cu, cv, fu, fv, skew = [float(v) for v in CAM]
    skew = 0.7  # (the rule's skew terms too)
    s, grey = 0.0005, 97.0
    c = np.array([0.21, -0.13, 1.9])

    def value(p):
        u = ((fu * p[0] + skew * p[1]) + cu * p[2]) / p[2]
        v = (fv * p[1] + cv * p[2]) / p[2]
        x0, y0 = int(np.floor(u)), int(np.floor(v))
        fx, fy = u - x0, v - y0
        i00, i10, i01, i11 = [float(G[y0 + dy, x0 + dx]) for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1))]
        top, bot = i00 + fx * (i10 - i00), i01 + fx * (i11 - i01)
        gx = (1 - fy) * (i10 - i00) + fy * (i11 - i01)
        gy = (1 - fx) * (i01 - i00) + fx * (i11 - i10)
        return s * (top + fy * (bot - top) - grey), gx, gy, (fx, fy)

    _, gx, gy, frac = value(c)
    assert min(frac) > 0.05 and max(frac) < 0.95 and abs(gx) > 1 and abs(gy) > 1  # (well inside one cell, a real gradient)
    x, y, z = c
    du = np.array([fu / z, skew / z, -(fu * x + skew * y) / z**2])
    dv = np.array([0.0, fv / z, -fv * y / z**2])
    a = s * (gx * du + gy * dv)
    J = np.concatenate([-a, np.cross(a, c)])

    def moved(xi):
        R, t = exp64(xi)
        return value(R.T @ (c - t))[0]  # exp(xi)^-1 c

    h = 1e-6
    num = np.array([(moved(h * np.eye(6)[i]) - moved(-h * np.eye(6)[i])) / (2 * h) for i in range(6)])
    assert np.abs(num - J).max() < 1e-8 * max(1.0, np.abs(J).max()), (num, J)
    assert np.abs(J).min() > 1e-4  # (every component is exercised; a wrong sign would show)


# ------------------------------------------------------------------------------------------------------------ 2. the evaluator against float64
@pytest.mark.parametrize("k", range(len(EVAL_POSES)))
def test_evaluator_against_float64(corner, k):
    pose = EVAL_POSES[k]
    ref = joint64(corner, pose, corner["fn"], MIN_COS, HUBER_M, PHOTO_SCALE_M, EVAL_PHOTO_HUBER_GREY, GATE_DIST_M)
    assert int(ref["doubtful"].sum()) == 0, "choose another pose: the float64 side itself has points at a decision"
    out = joint_host(corner, pose, GATE_DIST_M, iters=0, frame_normals=corner["fn"], min_cos=MIN_COS, huber_m=HUBER_M,
                     photo_scale_m=PHOTO_SCALE_M, photo_huber_grey=EVAL_PHOTO_HUBER_GREY)
    want = [int(ref[key].sum()) for key in ("with_depth", "within", "matched", "linear")]
    pwant = [int(ref["photo"].sum()), int(ref["photo_linear"].sum())]
    print(f"pose {k}: gate counts {out['gate_counts'].tolist()}, photo counts {out['photo_counts'].tolist()}")
    assert np.array_equal(~np.isnan(out["residuals"]), ref["matched"]) and np.array_equal(~np.isnan(out["photo_residuals"]), ref["photo"])
    assert out["gate_counts"].tolist() == want and out["photo_counts"].tolist() == pwant
    assert out["stats"]["matched"] == want[2] and out["sums29"][1] == float(want[2])  # the geometric count
    assert want[2] > pwant[0] > pwant[1] > 0  # some matched points have no footprint inside; both Huber branches are taken
    s64 = ref["joint_terms"].sum(0)
    mag = magnitudes(ref, HUBER_M) + photo_magnitudes(ref, PHOTO_SCALE_M * EVAL_PHOTO_HUBER_GREY)
    s32 = np.delete(out["sums29"], 1).astype(np.float64)
    rel = np.abs(s32 - s64) / np.where(mag > 0, mag, 1.0)
    print(f"pose {k}: largest |s32 - s64| / magnitude = {rel.max():.3g}")
    assert rel.max() <= SUM_REL_BOUND
    m, p = ref["matched"], ref["photo"]
    assert np.abs(out["residuals"][m] - ref["rows"][m, 0]).max() < 1e-5  # the raw geometric r
    assert np.abs(out["photo_residuals"][p] - ref["photo_d"][p]).max() < 2e-3  # grey levels, unscaled (|gradient| x eps |u| and roundings of ~255)
    energy = ref["loss"][m].sum() + ref["photo_loss"][p].sum()
    assert np.isclose(out["stats"]["rms"], np.sqrt(energy / want[2]), rtol=1e-5)  # the joint energy over the geometric count


# ------------------------------------------------------------------------------------------------------------ 3. the neutral case
OFF = pose_from_xi([0.01, -0.015, 0.02, 0.01, 0.005, -0.012])


@pytest.mark.parametrize("ranged", [False, True])
@pytest.mark.parametrize("count", COUNTS)
def test_neutral_case_is_the_robust_pass(corner, count, ranged):
    s = corner
    start = V.iso_mul(P_TRUE, OFF)
    rng = (3, max(1, count - 5)) if ranged else None
    for iters in (0, 3):
        for given in (True, False):  # the grey pointers may be NULL
            kw = dict(iters=iters, count=count, range2=rng, frame_normals=s["fn"], min_cos=MIN_COS, huber_m=HUBER_M)
            robust = V.icp_points_robust_host(s["xyz"], s["nrm"], s["depth"], CAM, SCALE, start, DIST_M,
                                              residuals=np.full(len(s["xyz"]), 42.0, np.float32), **kw)
            joint = V.icp_points_joint_host(s["xyz"], s["nrm"], s["gray"] if given else None, s["depth"], s["frame_gray"] if given else None, CAM,
                                            SCALE, start, DIST_M, photo_scale_m=0.0, photo_huber_grey=PHOTO_HUBER_GREY,
                                            residuals=np.full(len(s["xyz"]), 42.0, np.float32),
                                            photo_residuals=np.full(len(s["xyz"]), 42.0, np.float32), **kw)
            for key in ("pose", "sums29", "residuals", "gate_counts"):
                assert np.array_equal(bits(joint[key]), bits(robust[key])), key
            assert joint["stats"].tobytes() == robust["stats"].tobytes()
            assert joint["photo_counts"].tolist() == [0, 0]
            first, last = (0, min(count, len(s["xyz"]))) if rng is None else (min(3, count), min(count, 3 + rng[1]))
            pr = joint["photo_residuals"]
            assert np.isnan(pr[first:last]).all() and (pr[:first] == 42.0).all() and (pr[last:] == 42.0).all()


# ------------------------------------------------------------------------------------------------------------ the tree
def photo_rows32(c, u, v, gray_w, G, scale):
    """icp_row_photo in float32 with lie.h's operand order, for points whose footprint is inside."""
    f = np.float32
    cu, cv, fu, fv, skew = [f(x) for x in CAM]
    x0, y0 = np.floor(u), np.floor(v)
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    fx, fy = u - x0, v - y0
    i00, i10, i01, i11 = [G[yi + dy, xi + dx].astype(f) for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1))]
    dx0, dx1 = i10 - i00, i11 - i01
    top, bot = i00 + fx * dx0, i01 + fx * dx1
    im = top + fy * (bot - top)
    gx = (f(1) - fy) * dx0 + fy * dx1
    gy = (f(1) - fx) * (i01 - i00) + fx * (i11 - i10)
    d = im - gray_w.astype(f)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    iz = f(1) / z
    dux, duy, duz = fu * iz, skew * iz, -(((fu * x + skew * y) * iz) * iz)
    dvy, dvz = fv * iz, -(((fv * y) * iz) * iz)
    g = np.stack([scale * (gx * dux), scale * (gx * duy + gy * dvy), scale * (gx * duz + gy * dvz)], -1)
    return np.concatenate([(scale * d)[:, None], -g, cross(g, c)], -1).astype(f), d


@pytest.mark.parametrize("count", COUNTS)
def test_order_of_the_sums(corner, count):
    """The point's products are p_g + p_p in f32, geometric first, p_g alone without a photometric row; then the tree, unchanged."""
    from test_icp_robust_host import rows32
    s = corner
    f = np.float32
    pose = EVAL_POSES[2]
    scale, hub = f(PHOTO_SCALE_M), f(PHOTO_SCALE_M) * f(EVAL_PHOTO_HUBER_GREY)
    out = joint_host(s, pose, iters=0, count=count, frame_normals=s["fn"], min_cos=MIN_COS, huber_m=HUBER_M, photo_scale_m=PHOTO_SCALE_M,
                     photo_huber_grey=EVAL_PHOTO_HUBER_GREY)
    xyz, nrm, depth = s["xyz"][:count], s["nrm"][:count], s["depth"]
    res = out["residuals"][:count]
    m, x0, y0, n = rows32(xyz, nrm, pose, res)
    cu, cv, fu, fv, skew = [f(v) for v in CAM]
    xi, yi = np.where(m, x0, 0).astype(np.int64), np.where(m, y0, 0).astype(np.int64)
    z = f(1.0) / (f(SCALE) / np.where(m, depth[yi, xi], 1).astype(f))
    qy = (yi.astype(f) - cv) * z / fv
    qx = ((xi.astype(f) - cu) * z - skew * qy) / fu
    J = np.concatenate([n, cross(np.stack([qx, qy, z], -1), n)], -1)
    a = np.where(m[:, None], np.concatenate([res[:, None], J], -1), f(0.0)).astype(f)

    def weighted(a, h):
        r = a[:, 0]
        ar = np.abs(r)
        lin = ar <= h
        with np.errstate(all="ignore"):
            w = np.where(lin, f(1.0), h / ar).astype(f)
        e = np.where(lin, r * r, h * (f(2.0) * ar - h)).astype(f)
        return products(a, w, w * r, e).astype(f), ~lin

    pg, glin = weighted(a, f(HUBER_M))
    # the camera-frame point and (u, v) with lie.h's operand order (extr_project, project_uv)
    t, q = pose[:3].astype(f), pose[3:].astype(f)
    p = xyz + -t
    qv = np.broadcast_to(-q[:3], p.shape)
    tt = cross(qv, p) * f(2.0)
    c = ((tt * q[3] + cross(qv, tt)) + p).astype(f)
    with np.errstate(all="ignore"):
        u = ((fu * c[:, 0] + skew * c[:, 1]) + cu * c[:, 2]) / c[:, 2]
        v = (fv * c[:, 1] + cv * c[:, 2]) / c[:, 2]
        fu0, fv0 = np.floor(u), np.floor(v)
        photo = m & (fu0 >= 0) & (fu0 + f(1) <= f(COLS - 1)) & (fv0 >= 0) & (fv0 + f(1) <= f(ROWS - 1))
    terms = pg.copy()
    ap, d = photo_rows32(c[photo], u[photo], v[photo], s["gray"][:count][photo], s["frame_gray"], scale)
    pp, plin = weighted(ap, hub)
    terms[photo] = pg[photo] + pp
    want = tree32(terms, count)
    assert np.array_equal(bits(np.delete(out["sums29"], 1)), bits(want))
    assert np.array_equal(~np.isnan(out["photo_residuals"][:count]), photo)
    assert np.array_equal(bits(out["photo_residuals"][:count][photo]), bits(d.astype(f)))
    assert out["photo_counts"].tolist() == [int(photo.sum()), int(plin.sum())] and out["gate_counts"][3] == int((glin & m).sum())
    assert np.isnan(out["photo_residuals"][count:]).all()


# ------------------------------------------------------------------------------------------------------------ 4. it does what 7n lacked
def test_it_removes_the_in_plane_slide(plane):
    s = plane
    start = in_plane_start()
    a0, i0 = split_error(start)
    kw = dict(iters=ITERS, step_eps=0.0)
    plain = V.icp_points_robust_host(s["xyz"], s["nrm"], s["depth"], CAM, SCALE, start, DIST_M, **kw)
    joint = joint_host(s, start, photo_scale_m=PHOTO_SCALE_M, **kw)
    p64 = loop64(s, start, None, 0.0, 0.0, PHOTO_SCALE_M, 0.0, ITERS)
    ap, ip = split_error(plain["pose"])
    aj, ij = split_error(joint["pose"])
    a64, i64 = split_error(p64)
    p64 = p64 if p64[6] * joint["pose"][6] >= 0 else np.concatenate([p64[:3], -p64[3:]])
    diff = np.abs(joint["pose"].astype(np.float64) - p64).max()
    print(f"(along the normal, in the plane) in mm: start ({a0 * 1e3:.3g}, {i0 * 1e3:.3g}); plain ({ap * 1e3:.3g}, {ip * 1e3:.3g}) status "
          f"{plain['stats']['status']} after {plain['stats']['iterations']} updates; joint ({aj * 1e3:.3g}, {ij * 1e3:.3g}) status "
          f"{joint['stats']['status']} after {joint['stats']['iterations']} updates, photo counts {joint['photo_counts'].tolist()} of "
          f"{joint['stats']['matched']} matched; float64 ({a64 * 1e3:.3g}, {i64 * 1e3:.3g}); |pose32 - pose64| = {diff:.3g}")
    assert 0.009 < i0 < 0.011 and a0 < 1e-6  # the offset lies inside the plane
    assert ip >= i0 * (1 - 1e-4)  # THE FINDING of 7n: the point-to-plane pass does not reduce the in-plane error
    assert 2 * i64 <= IN_PLANE_BOUND_M  # the float64 loop alone meets the bound with a factor of 2 to spare
    assert ij < IN_PLANE_BOUND_M and ij < ip and ij < i0
    assert diff <= POSE_DIFF_BOUND
    assert joint["stats"]["iterations"] == ITERS and joint["photo_counts"][0] > 0.9 * joint["stats"]["matched"]


# ------------------------------------------------------------------------------------------------------------ 5. the photo Huber weight
def test_photo_huber(plane):
    s = dict(plane)
    gray = s["frame_gray"].astype(np.int32)
    gray[16:30, 20:38] += 70  # a patch of foreign grey: a shadow, a highlight, a moved object
    s["frame_gray"] = np.clip(gray, 0, 255).astype(np.uint8)
    start = in_plane_start()
    kw = dict(iters=ITERS, step_eps=0.0, photo_scale_m=PHOTO_SCALE_M)
    without = joint_host(s, start, **kw)
    with_ = joint_host(s, start, photo_huber_grey=PHOTO_HUBER_GREY, **kw)
    ref = joint64(s, with_["pose"], None, 0.0, 0.0, PHOTO_SCALE_M, PHOTO_HUBER_GREY)
    assert int(ref["doubtful"].sum()) == 0
    iw, ih = split_error(without["pose"])[1], split_error(with_["pose"])[1]
    print(f"in-plane error: without the weight {iw * 1e3:.3g} mm, with it {ih * 1e3:.3g} mm; photo counts {with_['photo_counts'].tolist()}")
    assert with_["photo_counts"].tolist() == [int(ref["photo"].sum()), int(ref["photo_linear"].sum())]
    assert with_["photo_counts"][1] > 100 and without["photo_counts"][1] == 0
    assert ih < iw


# ------------------------------------------------------------------------------------------------------------ 6. the border
def test_border_points_are_matched_but_not_photo(plane):
    """Points that project 0.3 pixel right of and below the pixel centres: those of the last row and column land inside the plane (their
    nearest pixel) but their bilinear footprint would read row `rows` or column `cols`."""
    s = plane
    n, dist = PLANES[0]
    cu, cv, fu, fv, skew = [float(v) for v in CAM]
    ys, xs = np.nonzero(s["depth"])
    u, v = xs + 0.3, ys + 0.3
    ry = (v - cv) / fv
    rx = ((u - cu) - skew * ry) / fu
    z = dist / (n[0] * rx + n[1] * ry + n[2])
    xyz = V.camera_back_project(CAM, P_TRUE, np.stack([u, v], -1).astype(np.float32), z.astype(np.float32))
    out = V.icp_points_joint_host(xyz, s["nrm"], s["gray"], s["depth"], s["frame_gray"], CAM, SCALE, P_TRUE, DIST_M, iters=0,
                                  photo_scale_m=PHOTO_SCALE_M)
    matched, photo = ~np.isnan(out["residuals"]), ~np.isnan(out["photo_residuals"])
    has_normal = np.abs(s["nrm"]).sum(-1) > 0
    border = (xs == COLS - 1) | (ys == ROWS - 1)
    assert np.array_equal(matched, has_normal)  # every point lands on its own pixel, the border's too
    assert (matched & border).sum() > 80 and not photo[border].any()
    assert np.array_equal(photo, matched & ~border)
    assert out["photo_counts"][0] == photo.sum() and out["stats"]["matched"] == matched.sum()
