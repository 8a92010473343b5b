"""Carrier overlaps and clumping, host side: report.carrier_rows / overlap_reference on a hand-worked 6-patient example,
and report.clump_rows on hand-made rows against a brute-force loop written here.  No GPU needed."""
from __future__ import annotations

import numpy as np
import pytest

from geneticscre_amd import report

# ---- a hand-worked example: 6 patients, columns 0-2 the cases, 3-5 the controls -----------------------------------------

ROWS = np.array([
    [1, 1, 1, 1, 1, 1],   # 0: everybody
    [0, 0, 0, 0, 0, 0],   # 1: nobody
    [1, 0, 0, 1, 0, 0],   # 2: case 0, control 3
    [0, 1, 0, 1, 1, 0],   # 3: case 1, controls 3 4
    [0, 0, 1, 0, 0, 1],   # 4: case 2, control 5
], np.int8)
SETS = [
    [2, 3],    # 0: "G2 (+) -> G3 (-)": signs do not matter, carriers {0, 1, 3, 4}        2 cases, 2 controls
    [3, 3],    # 1: a duplicate member: {1, 3, 4}                                          1, 2
    [2, -1],   # 2: an NA member: no carriers, not valid                                  -1, -1
    [1],       # 3: the empty row                                                          0, 0
    [0],       # 4: the full row                                                           3, 3
    [4, 4],    # 5: "G4 (+) -> G4 (-)", one member under both signs: {2, 5}                1, 1
]
CARRIERS = [{0, 1, 3, 4}, {1, 3, 4}, set(), set(), {0, 1, 2, 3, 4, 5}, {2, 5}]
SIZE = [[2, 2], [1, 2], [-1, -1], [0, 0], [3, 3], [1, 1]]
# BOTH[i][j] = (shared cases, shared controls); row / column 2 (NA) and 3 (nobody) are zeros
Z = [0, 0]
BOTH = [
    [[2, 2], [1, 2], Z, Z, [2, 2], Z],
    [[1, 2], [1, 2], Z, Z, [1, 2], Z],
    [Z, Z, Z, Z, Z, Z],
    [Z, Z, Z, Z, Z, Z],
    [[2, 2], [1, 2], Z, Z, [3, 3], [1, 1]],
    [Z, Z, Z, Z, [1, 1], [1, 1]],
]


def test_carrier_rows_and_overlap_reference_by_hand():
    C, valid = report.carrier_rows(SETS, ROWS, 6)
    assert C.dtype == bool and C.shape == (6, 6)
    assert valid.tolist() == [True, True, False, True, True, True]
    for s, want in enumerate(CARRIERS):
        assert set(np.flatnonzero(C[s]).tolist()) == want, s
    size, both = report.overlap_reference(SETS, ROWS, 3, 3)
    assert size.dtype == np.int32 and both.dtype == np.int32
    np.testing.assert_array_equal(size, np.array(SIZE))
    np.testing.assert_array_equal(both, np.array(BOTH))
    # index lists: repeats, a != b, empty
    a, b = [4, 0, 0, 2], [5, 1, 4]
    _, sub = report.overlap_reference(SETS, ROWS, 3, 3, a=a, b=b)
    np.testing.assert_array_equal(sub, np.array(BOTH)[a][:, b])
    _, none = report.overlap_reference(SETS, ROWS, 3, 3, a=[], b=None)
    assert none.shape == (0, 6, 2)
    # another split of the same patients: one case, five controls
    size15, both15 = report.overlap_reference(SETS, ROWS, 1, 5)
    assert size15.tolist() == [[1, 3], [0, 3], [-1, -1], [0, 0], [1, 5], [0, 2]]
    assert both15[0][1].tolist() == [0, 3] and both15[4][5].tolist() == [0, 2]
    np.testing.assert_array_equal(both15.sum(axis=2), np.array(BOTH).sum(axis=2))


# ---- clump_rows against a brute-force loop -----------------------------------------------------------------------------


def brute_clumps(order, size, both, r, measure, patients):
    S = len(size)
    clump, lead, value = [-1] * S, [-1] * S, [np.nan] * S
    shared = [[-1, -1] for _ in range(S)]
    tot = [int(c + (t if patients == "all" else 0)) for c, t in size]
    k = 0
    for i, row in enumerate(order):
        if clump[row] >= 0:
            continue
        clump[row], lead[row] = k, row
        for o in order[i + 1:]:
            if clump[o] >= 0:
                continue
            bo = int(both[row][o][0] + (both[row][o][1] if patients == "all" else 0))
            den = tot[row] + tot[o] - bo if measure == "jaccard" else min(tot[row], tot[o])
            v = np.float64(bo) / np.float64(den) if den > 0 else 0.0
            if v >= r:
                clump[o], lead[o], value[o], shared[o] = k, row, v, [int(x) for x in both[row][o]]
        k += 1
    return np.array(clump), np.array(lead), np.array(value), np.array(shared)


# 12 patients, the first 6 the cases.  Rows by hand: a strong row and nested / shifted copies of it, a second signal among
# the controls, two identical rows, two rows without carriers.
P = np.array([
    [1, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0],   # 0  signal A: cases 0-3, controls 6 7
    [1, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0],   # 1  A minus a case                       jaccard 5/6 with 0
    [1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0],   # 2  inside A                             jaccard 3/6, containment 1
    [1, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0],   # 3  == row 0
    [0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0],   # 4  shares case 3 with A                 jaccard 1/8
    [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1],   # 5  signal B: controls only
    [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0],   # 6  inside B
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],   # 7  nobody
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],   # 8  nobody
    [1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1],   # 9  B plus a case of A
    [0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1],   # 10 near row 4
], np.int8)
PSETS = [[i] for i in range(len(P))]
PSIZE, PBOTH = report.overlap_reference(PSETS, P, 6, 6)
SCORES = np.array([9.0, 7.0, 7.0, 9.0, 5.0, 8.0, 8.0, 6.0, 1.0, 7.0, 2.0])


def both_of_array(calls=None):
    def f(leads, others):
        if calls is not None:
            calls.append((len(leads), len(others)))
        return PBOTH[np.asarray(leads, np.int64)][:, np.asarray(others, np.int64)]
    return f


def by_score(rows):
    rows = np.asarray(rows, np.int64)
    return rows[np.argsort(-SCORES[rows], kind="stable")]


@pytest.mark.parametrize("patients", ["all", "cases"])
@pytest.mark.parametrize("measure", ["jaccard", "containment"])
@pytest.mark.parametrize("r", [0.1, 0.5, 0.75, 1.0])
def test_clump_rows_equals_brute_force_whatever_the_block(r, measure, patients):
    order = by_score(np.arange(len(P)))
    # ties in the score keep their table position: 0 before 3, 5 before 6, 1 before 2 before 9
    assert order.tolist() == [0, 3, 5, 6, 1, 2, 9, 7, 4, 10, 8]
    want = brute_clumps(order.tolist(), PSIZE, PBOTH, r, measure, patients)
    for block in (1, 2, 3, 10**6):
        got = report.clump_rows(order, PSIZE, both_of_array(), r, measure, patients, block=block)
        for g, w, name in zip(got, want, ("clump", "lead", "value", "shared")):
            np.testing.assert_array_equal(g, w, err_msg=f"{name}, block {block}")
    default = report.clump_rows(order, PSIZE, both_of_array(), r, measure, patients)
    for g, w in zip(default, want):
        np.testing.assert_array_equal(g, w)


def test_clump_rows_by_hand():
    order = by_score(np.arange(len(P)))
    # r = 1: only identical carrier sets merge, and rows without carriers stay alone (0 / 0 reads as 0.0)
    clump, lead, value, shared = report.clump_rows(order, PSIZE, both_of_array(), 1.0)
    assert clump.tolist() == [0, 3, 4, 0, 7, 1, 2, 6, 9, 5, 8]
    assert lead[3] == 0 and value[3] == 1.0 and shared[3].tolist() == [4, 2]
    assert np.isnan(value[0]) and shared[0].tolist() == [-1, -1] and lead[0] == 0
    # jaccard 0.5, all patients: A = {0, 3, 1, 2}, B = {5, 6, 9}, {4, 10}, and the rows without carriers each on its own
    clump, lead, value, shared = report.clump_rows(order, PSIZE, both_of_array(), 0.5)
    assert clump.tolist() == [0, 0, 0, 0, 3, 1, 1, 2, 4, 1, 3]
    assert value[1] == 5 / 6 and value[2] == 3 / 6 and value[6] == 3 / 4 and value[9] == 4 / 5
    assert value[10] == 2 / 4 and lead[10] == 4          # cases 4 5 of {3 4 5} + {4 5 11}
    assert shared[2].tolist() == [2, 1]
    # containment 1.0 on the cases only: row 4 joins A through its one shared case?  no: 1 / min(4, 3) < 1; row 9 does
    # (its only case is case 0), and rows 5, 6 (no cases at all) stay alone: 0 / min(.., 0) reads as 0.0
    clump, lead, value, shared = report.clump_rows(order, PSIZE, both_of_array(), 1.0, "containment", "cases")
    assert lead[9] == 0 and value[9] == 1.0 and shared[9].tolist() == [1, 0]
    assert lead[4] == 4 and lead[5] == 5 and lead[6] == 6 and lead[7] == 7 and lead[8] == 8
    # rows outside `order` get -1 everywhere
    part = by_score([0, 1, 4, 7])
    clump, lead, value, shared = report.clump_rows(part, PSIZE, both_of_array(), 0.5)
    assert clump.tolist() == [0, 0, -1, -1, 2, -1, -1, 1, -1, -1, -1]
    assert lead.tolist() == [0, 0, -1, -1, 4, -1, -1, 7, -1, -1, -1]
    assert np.isnan(value[[2, 3, 5]]).all() and (shared[[2, 3, 5]] == -1).all()
    # an empty order
    clump, _, _, _ = report.clump_rows([], PSIZE, both_of_array(), 0.5)
    assert (clump == -1).all()


def test_clump_rows_asks_in_blocks_and_checks_its_arguments():
    order = by_score(np.arange(len(P)))
    calls = []
    report.clump_rows(order, PSIZE, both_of_array(calls), 0.5, block=2)
    # every call: at most `block` candidate leads, against the unassigned rows after the first of them
    assert len(calls) > 1 and all(1 <= na <= 2 for na, _ in calls)
    assert calls[0] == (2, len(order) - 1)
    assert all(nb < calls[0][1] for _, nb in calls[1:])
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            report.clump_rows(order, PSIZE, both_of_array(), bad)
    with pytest.raises(ValueError):
        report.clump_rows(order, PSIZE, both_of_array(), 0.5, measure="dice")
    with pytest.raises(ValueError):
        report.clump_rows(order, PSIZE, both_of_array(), 0.5, patients="controls")
