"""What tests/test_pose_graph_host.py and tests/test_gpu_pose_graph.py share: a float64 numpy restatement of the pose-graph definition
(include/vors_hip.h 2g) and the test graphs. Poses are (t, q) with q = (i, j, k, w), camera -> world; a measurement M_ij maps camera i's
coordinates into camera j's, so consistent poses have T_j = T_i M_ij^-1 and E = T_i^-1 T_j M_ij is the identity."""
import numpy as np


def qmul(a, b):
    ai, aj, ak, aw = a
    bi, bj, bk, bw = b
    return np.array([aw * bi + ai * bw + aj * bk - ak * bj, aw * bj - ai * bk + aj * bw + ak * bi, aw * bk + ai * bj - aj * bi + ak * bw,
                     aw * bw - ai * bi - aj * bj - ak * bk])


def qrot(q, p):
    qv = q[:3]
    t = 2.0 * np.cross(qv, p)
    return p + q[3] * t + np.cross(qv, t)


def iso_mul(a, b):
    return np.concatenate([a[:3] + qrot(a[3:], b[:3]), qmul(a[3:], b[3:])])


def iso_inv(a):
    qi = np.array([-a[3], -a[4], -a[5], a[6]])
    return np.concatenate([qrot(qi, -a[:3]), qi])


def se3_exp(xi):
    """exp of (v, w) in float64: the closed form, series below 1e-6 rad."""
    xi = np.asarray(xi, np.float64)
    v, w = xi[:3], xi[3:]
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-6:
        c1, c2, s = 0.5, 1.0 / 6.0, 0.5 - th * th / 48.0
    else:
        c1, c2, s = (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3, np.sin(th / 2) / th
    t = (np.eye(3) + c1 * W + c2 * W @ W) @ v
    return np.concatenate([t, s * w, [np.cos(th / 2)]])


def residual(ti, tj, m):
    e = iso_mul(iso_mul(iso_inv(ti), tj), m)
    s = 1.0 if e[6] >= 0 else -1.0
    return np.concatenate([e[:3], 2.0 * s * e[3:6]])


def valid_edges(n_nodes, edges, meas, info, weight):
    ok = np.ones(len(edges), bool)
    for e, (i, j) in enumerate(edges):
        w = 1.0 if weight is None else weight[e]
        ok[e] = (i != j and i < n_nodes and j < n_nodes and np.isfinite(w) and w > 0 and np.isfinite(meas[e]).all()
                 and (info is None or np.isfinite(info[e]).all()))
    return ok


def energy(poses, edges, meas, info=None, weight=None):
    poses = np.asarray(poses, np.float64)
    ok = valid_edges(len(poses), edges, meas, info, weight)
    total = 0.0
    for e, (i, j) in enumerate(edges):
        if not ok[e]:
            continue
        r = residual(poses[i], poses[j], np.asarray(meas[e], np.float64))
        om = np.eye(6) if info is None else np.asarray(info[e], np.float64).reshape(6, 6)
        total += (1.0 if weight is None else float(weight[e])) * r @ om @ r
    return total


def numeric_jacobians(ti, tj, m, h=1e-6):
    """Central differences of the restatement's residual for T_k <- T_k exp(d_k) -> (J_i, J_j) [6, 6] float64."""
    ti, tj, m = (np.asarray(v, np.float64) for v in (ti, tj, m))
    ji, jj = np.zeros((6, 6)), np.zeros((6, 6))
    for a in range(6):
        d = np.zeros(6)
        d[a] = h
        ji[:, a] = (residual(iso_mul(ti, se3_exp(d)), tj, m) - residual(iso_mul(ti, se3_exp(-d)), tj, m)) / (2 * h)
        jj[:, a] = (residual(ti, iso_mul(tj, se3_exp(d)), m) - residual(ti, iso_mul(tj, se3_exp(-d)), m)) / (2 * h)
    return ji, jj


def gauss_newton(poses, edges, meas, info=None, weight=None, fixed=(0,), rounds=12):
    """The restatement's minimiser: Gauss-Newton with numerically differentiated Jacobians and a dense solve over the free nodes."""
    poses = np.array(poses, np.float64)
    n = len(poses)
    ok = valid_edges(n, edges, meas, info, weight)
    free = [k for k in range(n) if k not in fixed and any(ok[e] and k in edges[e] for e in range(len(edges)))]
    col = {k: 6 * c for c, k in enumerate(free)}
    for _ in range(rounds):
        H, g = np.zeros((6 * len(free), 6 * len(free))), np.zeros(6 * len(free))
        for e, (i, j) in enumerate(edges):
            if not ok[e]:
                continue
            m = np.asarray(meas[e], np.float64)
            r = residual(poses[i], poses[j], m)
            ji, jj = numeric_jacobians(poses[i], poses[j], m)
            om = (np.eye(6) if info is None else np.asarray(info[e], np.float64).reshape(6, 6)) * (1.0 if weight is None else float(weight[e]))
            for a, ja in ((i, ji), (j, jj)):
                if a not in col:
                    continue
                g[col[a]:col[a] + 6] += ja.T @ om @ r
                for b, jb in ((i, ji), (j, jj)):
                    if b in col:
                        H[col[a]:col[a] + 6, col[b]:col[b] + 6] += ja.T @ om @ jb
        d = np.linalg.solve(H, -g)
        for k in free:
            poses[k] = iso_mul(poses[k], se3_exp(d[col[k]:col[k] + 6]))
            poses[k][3:] /= np.linalg.norm(poses[k][3:])
        if np.abs(d).max() < 1e-12:
            break
    return poses


def random_pose(rng, trans, rot):
    return se3_exp(np.concatenate([rng.uniform(-trans, trans, 3), rng.uniform(-rot, rot, 3) / np.sqrt(3)]))


def measurement(ti, tj):
    """The exact M_ij of two poses: T_j^-1 T_i."""
    return iso_mul(iso_inv(tj), ti)


def pose_error(a, b):
    """Largest translation distance and rotation angle (rad) between two pose arrays."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dt = np.linalg.norm(a[:, :3] - b[:, :3], axis=1).max()
    dots = np.abs((a[:, 3:] * b[:, 3:]).sum(1)) / (np.linalg.norm(a[:, 3:], axis=1) * np.linalg.norm(b[:, 3:], axis=1))
    return dt, (2 * np.arccos(np.clip(dots, 0, 1))).max()


def _graph(truth, edges, seed, perturb=True):
    rng = np.random.default_rng(seed)
    start = np.array([truth[k] if k == 0 or not perturb else iso_mul(truth[k], random_pose(rng, 0.05, 0.05)) for k in range(len(truth))])
    meas = np.array([measurement(truth[i], truth[j]) for i, j in edges])
    return dict(truth=np.array(truth), poses=start.astype(np.float32), edges=np.array(edges, np.uint32), meas=meas.astype(np.float32))


def ring(n=24, chords=6, seed=1):
    """n poses on a circle looking around, consecutive edges, the closing edge, and `chords` edges across. Exact measurements; the start
    is the truth perturbed by up to 5 cm / 0.05 rad, node 0 excepted."""
    truth = [iso_mul(se3_exp([0, 0, 0, 0, 2 * np.pi * k / n, 0]), se3_exp([0, 0.1 * np.sin(k), 2.0, 0, 0, 0])) for k in range(n)]
    edges = [(k, (k + 1) % n) for k in range(n)] + [(k * (n // chords), (k * (n // chords) + n // 2 + 1) % n) for k in range(chords)]
    return _graph(truth, edges, seed)


def chain(n=40, seed=2):
    """A chain with one closing edge from the last node to the first."""
    truth = [iso_identity()]
    rng = np.random.default_rng(seed + 100)
    for _ in range(n - 1):
        truth.append(iso_mul(truth[-1], random_pose(rng, 0.2, 0.2)))
    return _graph(truth, [(k, k + 1) for k in range(n - 1)] + [(n - 1, 0)], seed)


def star(degree=200, seed=3):
    """A hub (node 1, free) with `degree` edges, to node 0 (fixed) and to degree - 1 leaves, every fourth leaf tied to node 0 as well."""
    rng = np.random.default_rng(seed + 200)
    truth = [iso_identity()] + [random_pose(rng, 1.0, 1.0) for _ in range(degree)]
    edges = [(1, 0)] + [((1, k) if k % 2 else (k, 1)) for k in range(2, degree + 1)] + [(0, k) for k in range(2, degree + 1, 4)]
    return _graph(truth, edges, seed)


def iso_identity():
    return np.array([0, 0, 0, 0, 0, 0, 1.0])


def noisy_ring(seed=4):
    """The ring with measurement noise (up to 1 cm / 0.01 rad) and random SPD information matrices."""
    g = ring(seed=seed)
    rng = np.random.default_rng(seed + 300)
    g["meas"] = np.array([iso_mul(m.astype(np.float64), random_pose(rng, 0.01, 0.01)) for m in g["meas"]]).astype(np.float32)
    info = []
    for _ in g["edges"]:
        a = rng.normal(size=(6, 6))
        info.append((a @ a.T + 6 * np.eye(6)).reshape(36))
    g["info"] = np.array(info, np.float32)
    return g


def grid(side, seed=5, extra=0):
    """side x side poses on a plane with edges to the right and downward neighbours (and `extra` random ones): many nodes, low degree."""
    rng = np.random.default_rng(seed + 400)
    truth = [iso_mul(se3_exp([0.3 * (k % side), 0.3 * (k // side), 0, 0, 0, 0]), random_pose(rng, 0.0, 0.3)) for k in range(side * side)]
    edges = [(k, k + 1) for k in range(side * side) if k % side != side - 1] + [(k, k + side) for k in range(side * (side - 1))]
    edges += [tuple(rng.choice(side * side, 2, replace=False)) for _ in range(extra)]
    return _graph(truth, edges, seed)
