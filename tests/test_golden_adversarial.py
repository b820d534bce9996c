"""The oracle on the adversarial fixtures (tests/golden/adversarial/*.npz, written by tests/golden/make_adversarial.py): the builders of
tests/adversarial.py still make the committed inputs, the oracle still gives the committed results bit for bit, its LM replay still
equals it, and every fixture still holds the outcome it targets — a change to a builder or to the oracle cannot empty a scenario
without this going red. CPU only."""
import glob
import os

import numpy as np
import pytest

from oracle import oracle as O

import adversarial as A

FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "adversarial", "*.npz")))
# fixture -> the outcomes it must contain (at least one pair each; mid_pyramid: every pair)
TARGETS = {"mid_pyramid": ("o1",), "rank_deficient": ("o2",), "outcomes": ("o1", "o2", "o3")}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_every_family_has_a_fixture():
    names = {os.path.basename(p)[:-4] for p in FIXTURES}
    assert names == set(A.FAMILIES) | {"outcomes"}


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_oracle_reproduces_adversarial_fixture(path):
    g = np.load(path)
    name, family, L, mode = os.path.basename(path)[:-4], str(g["family"]), int(g["L"]), int(g["mode"])
    rows, cols, intr = int(g["rows"]), int(g["cols"]), tuple(g["intr"])
    init = g["init"] if bool(g["has_init"]) else None
    # the builder still makes these inputs
    if family == "rank_deficient":
        kg, kd, cg, init_b = A.rank_deficient(int(g["seed"]), int(g["n_generated"]), rows, cols, intr, mode=mode, L=L)
    else:
        kg, kd, cg, init_b = A.FAMILIES[family](int(g["seed"]), int(g["n_generated"]), rows, cols, intr)
    keep = g["picked"]
    assert (kg[keep] == g["kf_gray"]).all() and (kd[keep] == g["kf_depth"]).all() and (cg[keep] == g["cur_gray"]).all()
    assert (init_b is None) == (init is None) and (init is None or (bits(init_b[keep]) == bits(init)).all())
    # the oracle still gives these results, and its replay still equals it
    cfg = O.make_config(L, intr, candidates_mode=mode, huber_delta=float(g["huber"]))
    ref = O.track_pairs(cfg, g["kf_gray"], g["kf_depth"], g["cur_gray"], init_poses7=init, n_threads=4)
    assert (ref["status"] == g["status"]).all() and (ref["nb_iter"] == g["nb_iter"]).all() and (ref["n_points"] == g["n_points"]).all()
    for k in ("poses", "models", "flow"):
        assert (bits(ref[k]) == bits(g[k])).all(), k
    cls = A.classify(cfg, g["kf_gray"], g["kf_depth"], g["cur_gray"], init)
    A.check_replay(ref, cls)
    assert all(A.same_energy(cls["energy"][p], g["energy"][p]) for p in range(len(cls["energy"])))
    for k in ("o1", "o2", "o3"):
        assert (cls[k] == g[k]).all(), k
    # a failed pair keeps its previous pose exactly (inverse_compositional.rs:206-208)
    failed = ref["status"] != 0
    assert (bits(ref["poses"][failed]) == bits(g["init"][failed])).all()
    # ... and the fixture still holds what it was made for
    for k in TARGETS.get(name, ()):
        assert cls[k].any(), f"{name}: no pair of outcome {k[1]} any more"
    if name == "mid_pyramid":
        assert cls["o1"].all() and (cls["fail_level"] == 0).all()
