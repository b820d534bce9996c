"""Image content that takes the DSO selector (candidates_mode = 2) through every branch it has, pinned on the CPU oracle alone.

The selector of csrc/dso_kernels.hip decides from the image which of its paths run: one to three rounds with an adapted base block size,
picks at three block levels with masks handed down, four ends, a pick list that may overflow. The synthetic scenes of synth_scene.h reach a
few of them. The ten integer patterns below (no RNG; i = row, j = column) reach the others, and CASES records, per pattern and shape, what
the oracle's select() does with it: the base size and the picks per block level of every round, the end it takes, the size of the final mask.
This module holds that table against O.dso_trace() — a second output of the very select() behind O.dso_mask(), not a restatement — and
asserts that the cases together cover the branches listed in test_cases_cover_every_branch. tests/test_gpu_dso_content.py runs the same
cases on the device.

OUT_OF_RANGE_EXHAUSTED (three rounds, the ratio still outside [0.8, 4], another block size wanted) is reached by none of the ten. A sweep on
the oracle over vertical lines, grids, checkers and dot lattices (periods 1 .. 40, contrasts 220/30, 255/0, 60/30 and 40/30, twelve shapes up
to 360 x 480) found it for weak content only, ten times; the eleventh pattern `weak_grid` at 250 x 331 is the richest of them: base sizes
4 -> 1 -> 3, no level-0 pick in any round, 8816 picks in round 1 (ratio 4.4, past the pick list's capacity in a round that is not the
final one), 956 in round 2 (ratio 0.48, target size 2, no round left).

Not marked gpu: everything here runs on the CPU.
"""
import numpy as np
import pytest

from oracle import oracle as O


def _ij(rows, cols):
    return np.arange(rows, dtype=np.int64)[:, None], np.arange(cols, dtype=np.int64)[None, :]


def _u8(a, rows, cols):
    a = np.broadcast_to(a, (rows, cols))
    assert a.min() >= 0 and a.max() <= 255
    return np.ascontiguousarray(a, np.uint8)


def constant(rows, cols):
    return np.full((rows, cols), 77, np.uint8)


def checker8(rows, cols):
    i, j = _ij(rows, cols)
    return _u8(255 * ((i // 8 + j // 8) & 1), rows, cols)


def checker4(rows, cols):
    i, j = _ij(rows, cols)
    return _u8(np.where((i // 4 + j // 4) & 1, 200, 50), rows, cols)


def lines16(rows, cols):
    i, j = _ij(rows, cols)
    return _u8(np.where((j % 16 == 0) | (i % 16 == 0), 220, 30), rows, cols)


def lines40(rows, cols):
    i, j = _ij(rows, cols)
    return _u8(np.where(j % 40 == 7, 220, 30), rows, cols)


def ramp(rows, cols):
    i, j = _ij(rows, cols)
    return _u8((3 * j + 2 * i) & 255, rows, cols)


def plateaus(rows, cols):
    i, j = _ij(rows, cols)
    return _u8(40 * ((i // 12 + 2 * (j // 20)) % 6), rows, cols)


def dense_dots(rows, cols):
    i, j = _ij(rows, cols)
    return _u8(np.where((i % 4 == 1) & (j % 4 == 2), 250, 10), rows, cols)


def weak_lines(rows, cols):
    i, j = _ij(rows, cols)
    a = 4 + ((i // 7) * 5 + (j // 9) * 3) % 36
    return _u8(np.where((j % 6 == 0) | (i % 10 == 0), 30 + a, 30), rows, cols)


def steps(rows, cols):
    i, j = _ij(rows, cols)
    return _u8(30 + ((i // 5) * 7 + (j // 6) * 11) % 29, rows, cols)


def weak_grid(rows, cols):
    i, j = _ij(rows, cols)
    return _u8(np.where((j % 4 == 0) | (i % 3 == 0), 40, 30), rows, cols)


FAMILIES = dict(constant=constant, checker8=checker8, checker4=checker4, lines16=lines16, lines40=lines40, ramp=ramp, plateaus=plateaus,
                dense_dots=dense_dots, weak_lines=weak_lines, steps=steps, weak_grid=weak_grid)

ALL, SUB, SAME, EXHAUSTED = O.DSO_OUTCOMES

# (family, rows, cols): ([(base size, (picks at block level 0, 1, 2)) per round], outcome, keep or -1, pixels of the final mask)
CASES = {
    ("constant", 120, 160): ([(4, (0, 0, 0)), (1, (0, 0, 0))], SAME, -1, 0),
    ("checker4", 120, 160): ([(4, (0, 0, 0)), (1, (0, 0, 0))], SAME, -1, 0),
    ("checker8", 120, 160): ([(4, (1196, 0, 0)), (3, (1504, 0, 0)), (2, (3456, 0, 0))], SUB, 147, 2009),
    ("dense_dots", 120, 160): ([(4, (1200, 0, 0)), (3, (1990, 0, 0))], ALL, -1, 1990),
    ("weak_lines", 120, 160): ([(4, (904, 31, 0)), (2, (2596, 213, 1))], SUB, 181, 2026),
    ("lines16", 96, 128): ([(4, (547, 0, 0)), (2, (1259, 0, 0)), (1, (2479, 0, 0))], SUB, 205, 1992),
    ("checker8", 61, 83): ([(4, (299, 0, 0)), (1, (2034, 0, 0))], ALL, -1, 2034),
    ("checker8", 121, 163): ([(4, (1199, 0, 0)), (3, (1572, 0, 0))], SAME, -1, 1572),  # (target size 3 again, a round still left)
    ("weak_lines", 121, 163): ([(4, (914, 31, 0)), (2, (2672, 207, 1))], SUB, 177, 2010),
    ("steps", 121, 163): ([(4, (0, 39, 48)), (1, (0, 57, 625))], SAME, -1, 682),
    ("ramp", 240, 320): ([(4, (372, 0, 0)), (1, (1767, 0, 0))], ALL, -1, 1767),
    ("lines16", 240, 320): ([(4, (3529, 0, 0))], SUB, 144, 2034),  # (the outcome is fixed in round 0)
    ("lines40", 250, 331): ([(4, (1054, 0, 0)), (3, (1245, 0, 0)), (2, (2232, 0, 0))], SUB, 228, 2016),
    ("weak_grid", 250, 331): ([(4, (0, 240, 240)), (1, (0, 4976, 3840)), (3, (0, 540, 416))], EXHAUSTED, -1, 956),
    ("steps", 360, 480): ([(4, (0, 175, 600)), (2, (0, 287, 2279))], SUB, 198, 1981),
    ("checker8", 360, 480): ([(4, (10796, 0, 0)), (11, (1408, 0, 0)), (9, (2160, 0, 0))], ALL, -1, 2160),
    ("weak_lines", 360, 480): ([(4, (8202, 268, 0)), (9, (1956, 0, 0))], ALL, -1, 1956),
}
CASE_IDS = [f"{f}_{r}x{c}" for f, r, c in CASES]

_traces = {}


def trace(family, rows, cols):
    """The oracle's trace of a case, computed once per process and shared (read-only)."""
    key = (family, rows, cols)
    if key not in _traces:
        t = O.dso_trace(FAMILIES[family](rows, cols))
        t["mask"].setflags(write=False)
        _traces[key] = t
    return _traces[key]


def test_generators_are_the_formulas():
    """The vectorised generators against the formulas written out per pixel (one small odd shape)."""
    rows, cols = 23, 45
    per_pixel = dict(
        constant=lambda i, j: 77,
        checker8=lambda i, j: 255 * ((i // 8 + j // 8) & 1),
        checker4=lambda i, j: 200 if ((i // 4 + j // 4) & 1) else 50,
        lines16=lambda i, j: 220 if (j % 16 == 0 or i % 16 == 0) else 30,
        lines40=lambda i, j: 220 if j % 40 == 7 else 30,
        ramp=lambda i, j: (3 * j + 2 * i) & 255,
        plateaus=lambda i, j: 40 * ((i // 12 + 2 * (j // 20)) % 6),
        dense_dots=lambda i, j: 250 if (i % 4 == 1 and j % 4 == 2) else 10,
        weak_lines=lambda i, j: 30 + (4 + ((i // 7) * 5 + (j // 9) * 3) % 36) if (j % 6 == 0 or i % 10 == 0) else 30,
        steps=lambda i, j: 30 + ((i // 5) * 7 + (j // 6) * 11) % 29,
        weak_grid=lambda i, j: 40 if (j % 4 == 0 or i % 3 == 0) else 30)
    assert set(per_pixel) == set(FAMILIES)
    for name, f in per_pixel.items():
        want = np.array([[f(i, j) for j in range(cols)] for i in range(rows)], np.uint8)
        got = FAMILIES[name](rows, cols)
        assert got.dtype == np.uint8 and got.shape == (rows, cols) and (got == want).all(), name


@pytest.mark.parametrize("case", list(CASES), ids=CASE_IDS)
def test_trace_is_the_recorded_one(case):
    """The trace entry gives the table's rounds, outcome and mask size, and its mask IS vo_dso_mask's (the two entries share select())."""
    rounds, outcome, keep, n_mask = CASES[case]
    t = trace(*case)
    mask, bs = O.dso_mask(FAMILIES[case[0]](*case[1:]))
    assert (t["mask"] == mask).all() and t["base_sizes"] == [int(b) for b in bs]
    assert set(np.unique(mask)) <= {0, 1}
    assert list(zip(t["base_sizes"], t["level_counts"])) == rounds
    assert (t["outcome"], t["keep"]) == (outcome, keep)
    assert int(mask.sum()) == n_mask
    final = sum(rounds[-1][1])
    if outcome == SUB:
        assert 1.1 * 2000 < final <= 4.0 * 2000 and keep == int(np.float32(255.0) / (np.float32(final) / np.float32(2000))) and n_mask < final
    else:
        assert n_mask == final and keep == -1
        assert (0.8 * 2000 <= final <= 1.1 * 2000) == (outcome == ALL)
        if outcome == EXHAUSTED:
            assert len(rounds) == 3


def test_cases_cover_every_branch():
    """What the GPU tests of these cases can reach is what this union reaches: each condition below loses its last case -> this fails."""
    t = {case: trace(*case) for case in CASES}
    finals = {case: (len(v["base_sizes"]) - 1, v["base_sizes"][-1], v["level_counts"][-1]) for case, v in t.items()}
    assert {v["outcome"] for v in t.values()} == {ALL, SUB, SAME, EXHAUSTED}
    assert {f[0] for f in finals.values()} == {0, 1, 2}
    assert {b for v in t.values() for b in v["base_sizes"]} >= {1, 2, 3, 4, 9, 11}
    assert any(f[2][1] >= 100 for f in finals.values())
    assert any(f[2][2] >= 500 for f in finals.values())
    assert any(f[2][0] == 0 and f[2][1] + f[2][2] > 0 for f in finals.values())
    assert any(not v["mask"].any() for v in t.values())
    # the pick list of a pair holds S0/16 + S0/64 + S0/256 + 1024 entries (rounded up to 4: plan_dso of csrc/batch.cpp), sized for base size 4

    def cap(case):
        s0 = case[1] * case[2]
        return (s0 // 16 + s0 // 64 + s0 // 256 + 1024 + 3) & ~3

    # ... a later round that is the final one overflows it (the usable picks are then read back from the stamps, band by band)
    for case in (("lines16", 96, 128), ("checker8", 61, 83), ("weak_lines", 120, 160)):
        assert finals[case][0] >= 1 and sum(finals[case][2]) > cap(case), case
    # ... a round that is NOT the final one overflows it and the final round fits again (the list starts over in every round)
    case = ("weak_grid", 250, 331)
    assert sum(t[case]["level_counts"][1]) > cap(case) >= sum(finals[case][2]) and finals[case][0] == 2
    # ... and round 0 is final with a list that fits (the LDS form of round 0 then never writes its stamps)
    case = ("lines16", 240, 320)
    assert finals[case][0] == 0 and sum(finals[case][2]) <= cap(case)
