"""The DSO selector (candidates_mode = 2, dso_rounds_kernel and what reads its picks) on image content that reaches every branch. GPU only.

tests/test_dso_content.py pins, on the CPU oracle alone, what select() does with each (pattern, shape) of its CASES: rounds, base block sizes,
picks per block level, the end taken. The device has no accessor for its DsoState; its branch is pinned through what it produces: the
level-0 candidate set must be the oracle's mask (whose branch is asserted there), and every level's points the oracle tracker's.

Inputs per case: keyframe grey = the pattern; depth 5000 with ~10 % zeros; current grey = the pattern shifted by one column; a batch of two
pairs, the second another pattern of the same shape (PARTNER), so that the workgroups of one launch take different branches.

Empty selections (`constant`, `checker4`: no pick at any level in any round, and `steps` next to `constant`): the oracle tracks an empty set —
NaN energy, Cholesky failure, status 1, identity pose, n_points 0 at every level — so the device must return exactly that. On the device
the rounds kernel publishes a list of 0 picks, the records kernel leaves its loop at `n0 == 0` with n_used = 0 at every level, and the LM
kernels sum over no slots (as test_gpu_parity.py::test_no_usable_candidates_keeps_pose has it for the coarse-to-fine records).

No pose gate in the EXACT / FUSED arithmetics: periodic patterns shifted by a column are ill-conditioned (most of them fail in the oracle
too), and the 1e-4 pose bar was stated for the synthetic scenes. REFERENCE arithmetic is held to the oracle's bits as everywhere.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import vors_amd as V
from oracle import oracle as O

import test_dso_content as T
import test_gpu_dso_sparse as S

BLOCKY = 1 << 63  # seeds with the top bit set render the piecewise-constant texture (synth_scene.h)
LEVELS = {(120, 160): 4, (96, 128): 3, (61, 83): 3, (121, 163): 4, (240, 320): 5, (250, 331): 4, (360, 480): 5}
PARTNER = dict(constant="weak_lines", checker4="dense_dots", checker8="steps", dense_dots="plateaus", weak_lines="checker8", lines16="ramp",
               ramp="lines16", lines40="weak_grid", weak_grid="lines40", steps="constant")
ARITHS = {"reference": V.ARITH_REFERENCE, "exact": V.ARITH_EXACT, "fused": V.ARITH_FUSED}


def case_depth(rows, cols):
    rng = np.random.default_rng(rows * 1009 + cols)
    kd = np.full((rows, cols), 5000, np.uint16)
    kd[rng.random((rows, cols)) < 0.1] = 0
    return kd


def case_batch(family, rows, cols):
    """(keyframe grey, keyframe depth, current grey) of the two pairs of a case."""
    kg = np.stack([T.FAMILIES[family](rows, cols), T.FAMILIES[PARTNER[family]](rows, cols)])
    kd = np.stack([case_depth(rows, cols)] * 2)
    return kg, kd, np.ascontiguousarray(np.roll(kg, 1, axis=2))


def to_dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a)).cuda() for a in arrays]


def hip_last_error():
    from test_gpu_reproject_depth import hip_last_error as f
    return f()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def sort_xy(xy):
    return np.lexsort((xy[:, 1], xy[:, 0]))


_oracle = {}


def oracle_of(case):
    """What the oracle makes of a case, computed once and shared by the arithmetics (never written to)."""
    if case not in _oracle:
        family, rows, cols = case
        L = LEVELS[(rows, cols)]
        intr = O.scaled_intrinsics(rows, cols)
        kg, kd, cg = case_batch(*case)
        cfg = O.make_config(L, intr, candidates_mode=2)
        masks = [T.trace(family, rows, cols)["mask"], T.trace(PARTNER[family], rows, cols)["mask"]]
        points = []
        for p in range(2):
            tr = O.Tracker(cfg, 0.0, kd[p], 0.0, kg[p])
            points.append([tr.points(l) for l in range(L)])
        _oracle[case] = dict(L=L, intr=intr, inputs=(kg, kd, cg), masks=masks, points=points, ref=O.track_pairs(cfg, kg, kd, cg))
    return _oracle[case]


def level0_set(b, p, rows, cols):
    xy = b.points(p, 0)[0]
    mask = np.zeros((rows, cols), np.uint8)
    mask[xy[:, 1], xy[:, 0]] = 1
    return mask


@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("case", list(T.CASES), ids=T.CASE_IDS)
def test_content_case_vs_oracle(case, arith):
    """A row of the table: level-0 set = oracle mask & (depth != 0); every level's points the oracle tracker's (coordinates always, inverse
    depths and Jacobians by bits in REFERENCE and EXACT — FUSED may take shorter forms of the same values on large levels, README);
    n_points at every level; in REFERENCE also status, iteration counts, models and poses by bits. An empty selection: status 1 and
    n_points 0 like the oracle (module docstring)."""
    import torch
    family, rows, cols = case
    o = oracle_of(case)
    L, intr, ref = o["L"], o["intr"], o["ref"]
    kg, kd, cg = o["inputs"]
    cfg = V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=2, arithmetic=ARITHS[arith])
    b = V.Batch(cfg, 2, rows, cols)
    poses = torch.zeros((2, 7), dtype=torch.float32, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    stats = V.stats_tensor(2)
    b.track_pairs(*to_dev(kg, kd, cg), poses, status, stats)
    torch.cuda.synchronize()
    poses, status, stats = poses.cpu().numpy(), status.cpu().numpy(), V.decode_stats(stats)
    print(f"[{family} {cols}x{rows} {arith}] level-0 points {stats['n_points'][:, 0]}, status {status}, oracle status {ref['status']}")
    for p in range(2):
        m = level0_set(b, p, rows, cols)
        assert (m == (o["masks"][p] & (kd[p] != 0))).all(), f"level-0 set of pair {p}"
        for l in range(L):
            xy, iz, jac, tm = b.points(p, l)
            oxy, oiz, ojac = o["points"][p][l]
            o1, o2 = sort_xy(xy), sort_xy(oxy)
            assert xy.shape == oxy.shape and (xy[o1] == oxy[o2]).all(), f"pair {p} level {l}"
            if arith != "fused":
                assert (bits(iz[o1]) == bits(oiz[o2])).all() and (bits(jac[o1]) == bits(ojac[o2])).all(), f"pair {p} level {l}"
    assert (stats["n_points"][:, :L] == ref["n_points"]).all()
    for p in range(2):
        if not o["masks"][p].any():  # the empty selection
            assert status[p] == ref["status"][p] == 1 and (stats["n_points"][p, :L] == 0).all()
    if arith == "reference":
        assert (status == ref["status"]).all() and (stats["nb_iter"][:, :L] == ref["nb_iter"]).all()
        assert (bits(stats["lm_model"]) == bits(ref["models"])).all() and (bits(poses) == bits(ref["poses"])).all()
    assert hip_last_error() == 0


# ------------------------------------------------------------------------------------------------ forms of the same computation
# the rows where the list overflows in a later round, where round 0 is final (no stamps in the LDS form) and where the upper levels pick
FORM_ROWS = [("checker8", 120, 160), ("weak_lines", 120, 160), ("lines16", 96, 128), ("checker8", 61, 83), ("lines16", 240, 320), ("steps", 121, 163)]
FORMS = {"planes": dict(planes=True), "scan": dict(scan=True), "stamps": dict(extra_env={"VORS_DSO_STAMPS": "1"}),
         "rounds_global": dict(extra_env={"VORS_DSO_ROUNDS_LDS": "0"}), "no_first_maxima": dict(extra_env={"VORS_DSO_FIRST_MAXIMA": "0"}),
         "bitonic": dict(sort="bitonic")}
# (the environment switches are read once per process: each form in its own interpreter, all six rows in one go; lists in DEVICE order)
DUMP = r"""
import sys, os
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "visual-odometry-rs_amd")); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np, torch
import vors_amd as V
from test_gpu_dso_content import FORM_ROWS, LEVELS, case_batch, to_dev
res = dict()
for fam, rows, cols in FORM_ROWS:
    L, intr = LEVELS[(rows, cols)], V.scaled_intrinsics(rows, cols)
    b = V.Batch(V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=2), 2, rows, cols)
    poses = torch.zeros((2, 7), device="cuda"); status = torch.zeros(2, dtype=torch.int32, device="cuda")
    b.track_pairs(*to_dev(*case_batch(fam, rows, cols)), poses, status); torch.cuda.synchronize()
    tag = f"{{fam}}_{{rows}}x{{cols}}"
    res[f"{{tag}}/poses"] = poses.cpu().numpy().view(np.uint32); res[f"{{tag}}/status"] = status.cpu().numpy()
    for p in range(2):
        for l in range(L):
            xy, iz, jac, tm = b.points(p, l)
            res[f"{{tag}}/xy_{{p}}_{{l}}"] = xy; res[f"{{tag}}/iz_{{p}}_{{l}}"] = iz.view(np.uint32); res[f"{{tag}}/jac_{{p}}_{{l}}"] = jac.view(np.uint32); res[f"{{tag}}/tm_{{p}}_{{l}}"] = tm
np.savez({out!r}, **res)
"""


def run_form(tmp_path, tag, **kw):
    """test_gpu_dso_sparse.run (one interpreter per form, its handling of the VORS_DSO_* environment) on this module's dump script."""
    dump, S.DUMP = S.DUMP, DUMP
    try:
        return dict(S.run(tmp_path, tag, kw.pop("planes", False), 0, 0, 0, **kw))
    finally:
        S.DUMP = dump


@pytest.fixture(scope="module")
def default_form(tmp_path_factory):
    return run_form(tmp_path_factory.mktemp("dso_content_default"), "default")


@pytest.mark.parametrize("form", list(FORMS))
def test_forms_give_the_same_lists_on_content(tmp_path, default_form, form):
    """The default form (pick lists from the rounds kernel, round 0 in LDS on the first pass's maxima, bucket sort) against each other
    form, on FORM_ROWS: the same lists, values and order at every level, hence status and poses bit for bit. The plane path lists in raster
    order, not Morton order: the same sets with the same values and the same status (the empty second pair of steps 121 x 163 included:
    status 1); its sums differ in their last bits, the pose difference is printed and, on this ill-conditioned content, held to no bar."""
    a, b = default_form, run_form(tmp_path, form, **FORMS[form])
    assert set(a) == set(b) and any(k.endswith("/xy_0_0") and len(a[k]) > 1000 for k in a)
    for key in a:
        if form != "planes":
            assert a[key].shape == b[key].shape and (a[key] == b[key]).all(), key
            continue
        tag, name = key.split("/")
        if name == "status":
            assert (a[key] == b[key]).all(), key
        if name == "poses":
            print(f"[{tag}] plane path vs default form: max pose difference {np.abs(a[key].view(np.float32) - b[key].view(np.float32)).max():.2e}")
        if name in ("poses", "status"):
            continue
        xy = f"{tag}/xy{name[name.index('_'):]}"  # (the coordinates of the same pair and level)
        assert a[key].shape == b[key].shape and (a[key][sort_xy(a[xy])] == b[key][sort_xy(b[xy])]).all(), key


# ------------------------------------------------------------------------------------------------ stamps across keyframes of changing content
@pytest.mark.parametrize("form", [{}, {"VORS_DSO_SCAN": "1"}, {"VORS_DSO_PLANES": "1"}], ids=["pick_lists", "stamp_scan", "mask_planes"])
def test_stamps_stay_valid_over_keyframes_of_changing_content(form, monkeypatch):
    """34 keyframes through ONE handle at 120 x 160 (two wraps of the stamp epoch), the content cycling through checker8 (final round 2),
    dense_dots (final round 1), constant (empty: nothing stamped), weak_lines (round 1, sub-sampled, its list overflowing: read back from
    the stamps) and a BLOCKY scene; the second pair two steps ahead in the cycle. The level-0 set is the oracle's every time: a stamp left by
    any round of one keyframe is never taken for a pick of a later keyframe, whether that keyframe's final round is the same or another one,
    before and after the stamp plane is cleared at a wrap."""
    import torch
    for k, v in form.items():
        monkeypatch.setenv(k, v)
    rows, cols, L, n = 120, 160, 4, 2
    intr = O.scaled_intrinsics(rows, cols)
    cycle = ["checker8", "dense_dots", "constant", "weak_lines", None]
    assert [len(T.CASES[(f, rows, cols)][0]) - 1 for f in cycle[:4]] == [2, 1, 1, 1]  # (final rounds, as the CPU table has them)
    b = V.Batch(V.Config(nb_levels=L, intrinsics=V.Intrinsics(intr[:2], intr[2:4], intr[4]), candidates_mode=2), n, rows, cols)
    poses = torch.zeros((n, 7), device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    kd = np.stack([case_depth(rows, cols)] * n)

    def content(k):
        f = cycle[k % len(cycle)]
        if f is not None:
            return T.FAMILIES[f](rows, cols), T.trace(f, rows, cols)["mask"]
        g = O.synth_batch(1, rows, cols, seed0=BLOCKY | (0x5EED1200 + 16 * k), intr=intr)[0][0]
        return g, O.dso_mask(g)[0]

    for it in range(34):
        frames = [content(it + 2 * p) for p in range(n)]
        kg = np.stack([f[0] for f in frames])
        b.track_pairs(*to_dev(kg, kd, np.roll(kg, 1, axis=2)), poses, status)
        torch.cuda.synchronize()
        for p in range(n):
            assert (level0_set(b, p, rows, cols) == (frames[p][1] & (kd[p] != 0))).all(), f"keyframe {it}, pair {p}"
    assert hip_last_error() == 0
