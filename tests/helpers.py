"""Shared comparison helpers for the parity tests."""
from __future__ import annotations

import numpy as np

from geneticscre_amd.synth import Problem, make_problem


def small_table(n_cases: int, n_ctrls: int, seed: int = 0) -> np.ndarray:
    """A cheap value table with many distinct f64 values whose f32 roundings differ from them."""
    rng = np.random.default_rng(seed)
    return rng.random((n_cases + 1, n_ctrls + 1)) * 20.0 + rng.random((n_cases + 1, n_ctrls + 1)) * 1e-7


# ---- value tables that hold special values (tests/test_tables_host.py, tests/test_gpu_tables.py) -----------------------
# Each family keeps to one kind of trouble, so that one cannot drown another (a table with 1 % of overflowing cells saturates
# every null maximum to +inf from level 2 on at 1,000 patients).  Deterministic in (kind, n_cases, n_ctrls, seed) and the variant, where a
# family has several.  What each family has to provoke in the oracle's own results is
# asserted in tests/test_tables_host.py.
TABLE_FAMILIES = ("zeros", "nonfinite", "tiny", "huge", "ladder", "shapes")
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_DENORM = 2.0 ** -149                       # the smallest f32 denormal, 1.4e-45
FLT_OVERFLOW = FLT_MAX + 2.0 ** 103            # FLT_MAX + ulp/2: the smallest double that rounds to +inf


def _choose(rng, shape, shares):
    """An integer class per cell: class k with probability shares[k], the last class takes the rest."""
    edges = np.cumsum(list(shares))
    return np.searchsorted(edges, rng.random(shape), side="right")


def special_table(kind: str, n_cases: int, n_ctrls: int, seed: int = 0, variant: int = 0) -> np.ndarray:
    """A value table of the family ``kind`` for an n_cases / n_ctrls cohort ((n_cases + 1) x (n_ctrls + 1) doubles);
    ``variant`` picks among the forms a family has (nonfinite: variant % 3 says what table[0][0] is, 3 to 5 mirror the NaN
    cells; huge: 1 = the sparse form; ladder: 1 = the band)."""
    shape = (n_cases + 1, n_ctrls + 1)
    rng = np.random.default_rng([seed, TABLE_FAMILIES.index(kind), n_cases, n_ctrls])
    if kind == "zeros":
        # both zeros by the third, negatives, positives that are nearly zero, the rest on a grid of halves (ties)
        c = _choose(rng, shape, (0.3, 0.3, 0.08, 0.07))
        t = np.round(rng.random(shape) * 6.0) / 2.0 + 0.5
        t[c == 0] = 0.0
        t[c == 1] = -0.0
        t[c == 2] = -np.round(rng.random(shape) * 8.0 + 1.0)[c == 2] / 4.0
        t[c == 3] = (1e-16 * np.round(rng.random(shape) * 3.0 + 1.0))[c == 3]
        return t
    if kind == "nonfinite":
        # NaN and -inf by the few percent on either side of the diagonal, +inf in one cell of a thousand (fewer past 1,000
        # patients: one +inf cell that a level reaches is the maximum of most of its permutations), finite negatives;
        # table[0][0] is NaN, negative or +inf by variant (what the pruned kernels' first ladder row is built from)
        c = _choose(rng, shape, (0.04, 0.04, 0.001 * min(1.0, 1000.0 / (n_cases + n_ctrls)), 0.1))
        t = rng.random(shape) * 12.0 + rng.random(shape) * 1e-7
        t[c == 1] = -np.inf
        t[c == 2] = np.inf
        t[c == 3] = -(rng.random(shape) * 5.0)[c == 3]
        nan = c == 0
        if variant >= 3:
            # the mirrored form: NaN only where the transposed cell is in the table and is NaN too, so that the signed
            # method's vtmax = std::max(t[r][c], t[c][r]) stays symmetric and its pruned kernels, which stand aside for a
            # table with a NaN on one side of the diagonal only, read NaN, -inf and +inf themselves
            m = min(shape)
            upper = np.triu(nan[:m, :m])
            nan = np.zeros(shape, bool)
            nan[:m, :m] = upper | upper.T
        t[nan] = np.nan
        t[0, 0] = (np.nan, -2.5, np.inf)[variant % 3]
        return t
    # A null maximum is the largest of thousands of cells, so a value that a few cells in a hundred hold is every
    # permutation's maximum.  The three families below therefore draw the bulk of their cells from a heavy-tailed law (c / u,
    # u uniform: the largest of N draws spreads over a decade) and place their special cells at a share that shrinks with the
    # cohort, so that the part of the table a level's paths reach holds a handful of them whatever its size.
    rare = min(1.0, 70.0 / (n_cases + n_ctrls))
    u = 1.0 - rng.random(shape)
    if kind == "tiny":
        # everything below FLT_MIN: the f32 image of a cell is a denormal or 0.  The bulk stays below FLT_MIN / 2, so that
        # the signed method's sums of two cells are denormals too
        t = np.minimum(2e-42 * rare / u, 5e-39) + 1e-44
        c = _choose(rng, shape, (0.02, 0.02, 0.02, 0.02, 0.001 * rare, 0.001 * rare, 0.001 * rare, 0.001 * rare, 0.05))
        t[c == 0] = 0.7e-45                                   # below half the smallest denormal: rounds to 0
        t[c == 1] = 1.4e-45                                   # rounds to the smallest denormal
        k = np.floor(rng.random(shape) * 1000.0)
        t[c == 2] = ((k + 0.5) * FLT_DENORM)[c == 2]          # exactly halfway between two denormals (ties to even)
        t[c == 3] = 2.0 ** -150                               # halfway between 0 and the smallest denormal
        t[c == 4] = np.nextafter(FLT_MIN, 0.0)                # the doubles next to FLT_MIN ...
        t[c == 5] = np.nextafter(FLT_MIN, 1.0)
        t[c == 6] = FLT_MIN - FLT_DENORM                      # ... and the floats next to it
        t[c == 7] = FLT_MIN + FLT_DENORM
        t[c == 8] = (10.0 ** (-50.0 + rng.random(shape) * 6.0))[c == 8]   # 1e-50 .. 1e-44: all round to 0 or one denormal
        return t
    if kind == "huge":
        # everything at the top of the f32 range.  The bulk stays below FLT_MAX / 2 so that a sum of two cells stays finite;
        # halves of FLT_MAX sum to FLT_MAX exactly, a half plus half an f32 ulp to the double that rounds to +inf
        t = 1e38 + np.minimum(1e35 * rare / u, 0.65e38)
        c = _choose(rng, shape, (0.02 * rare, 0.004 * rare, 0.004 * rare, 0.004 * rare, 0.004 * rare, 0.002 * rare,
                                 0.001 * rare))
        t[c == 0] = FLT_MAX / 2.0
        t[c == 1] = FLT_MAX / 2.0 + 2.0 ** 103                # + FLT_MAX / 2 = FLT_OVERFLOW although neither term is near it
        t[c == 2] = (1.66e38 + rng.random(shape) * 0.1e38)[c == 2]
        t[c == 3] = FLT_MAX
        t[c == 4] = np.nextafter(FLT_OVERFLOW, 0.0)           # rounds to FLT_MAX
        t[c == 5] = FLT_OVERFLOW                              # rounds to +inf
        t[c == 6] = 3.5e38
        if variant % 2 == 1:   # the sparser variant: mostly zeros, a few cells far beyond f32
            t[rng.random(shape) < 0.7] = 0.0
            t[rng.integers(0, n_cases + 1, 6), rng.integers(0, n_ctrls + 1, 6)] = 1e300
        return t
    if kind == "ladder":
        # cells on the levels of both pruning ladders (multiples of 1/8 and of 1/16) up to 50, past both ladders' tops (32
        # and 22), each exact or one f64 ulp or one f32 ulp to either side: a double one f64 ulp above a level has its f32
        # image ON the level
        t = np.floor(np.minimum(0.6 * rare / u, 50.0) * 16.0) / 16.0
        if variant == 1:
            # the band: every non-zero cell in [8, 10.5), thinning out towards the top, so that the maxima of a level lie
            # within a few ladder steps of one another and below both ladders' tops (the signed method adds two cells): what a
            # ladder row admits one step too early is then some permutation's maximum
            t = np.floor((10.5 - 2.5 * rng.random(shape) ** (1.0 / 3.0)) * 32.0) / 32.0     # (half steps of the finer ladder too)
        c = _choose(rng, shape, (0.3, 0.1, 0.1, 0.1, 0.1))
        up32 = np.nextafter(t.astype(np.float32), np.float32(np.inf)).astype(np.float64)
        dn32 = np.nextafter(t.astype(np.float32), np.float32(-np.inf)).astype(np.float64)
        t = np.where(c == 1, np.nextafter(t, np.inf), t)
        t = np.where(c == 2, np.nextafter(t, -np.inf), t)
        t = np.where(c == 3, up32, t)
        t = np.where(c == 4, dn32, t)
        t[c == 0] = 0.0
        return t
    raise ValueError(kind)


def shape_tables(n_cases: int, n_ctrls: int, seed: int = 0):
    """The family ``shapes``: [(name, table, undersized)] -- a positive table of the wrong size for the cohort.  Cells the
    table does not have read as -1 (the reference pads its (n + 1)^2 copy with -1, join_base.cpp:67-78); with the signed
    method the transposed reads fall outside a non-square table."""
    n = n_cases + n_ctrls
    sizes = [("0x0", 0, 0), ("1x1", 1, 1), ("few_rows", 3, n_ctrls + 1), ("few_cols", n_cases + 1, 2), ("few_both", 4, 3),
             ("larger", n_cases + 9, n_ctrls + 5), ("square", n + 1, n + 1)]
    out = []
    for name, r, c in sizes:
        t = small_table(max(r, 1) - 1, max(c, 1) - 1, seed + 1)[:r, :c]
        out.append((name, np.ascontiguousarray(t), r < n_cases + 1 or c < n_ctrls + 1))
    return out


# the cohorts of the table tests: (genes, edges, n_cases, n_ctrls, permutations, path length, carrier threshold; at 70
# patients the usual 5 % would leave every gene at most 3 carriers and a level a dozen table cells to read).  2,300 permutations are more
# than one 2,048-permutation tile: thresholds are read again, and the ladder row recomputed, with maxima already high.
# p5000 has the mask width of BASELINE configs[2] (79 words).
TABLE_SIZES = {"p70": (60, 150, 37, 33, 300, 5, 0.3), "p1000": (60, 200, 460, 540, 2300, 4, 0.05),
               "p5000": (120, 400, 2450, 2600, 2300, 4, 0.05)}
# (family, size, method) -> (seed, variant) of the table AND the seed of the network: chosen so that the oracle's results
# meet the family's conditions (tests/test_tables_host.py asserts them), variants spread over the cases
TABLE_CASES = {
    ("zeros", "p70", "method1"): (0, 0), ("zeros", "p70", "method2"): (0, 0),
    ("nonfinite", "p70", "method1"): (2, 0), ("nonfinite", "p70", "method2"): (2, 1),
    ("tiny", "p70", "method1"): (1, 0), ("tiny", "p70", "method2"): (6, 0),
    ("huge", "p70", "method1"): (0, 0), ("huge", "p70", "method2"): (0, 0),
    ("ladder", "p70", "method1"): (28, 0), ("ladder", "p70", "method2"): (18, 0),
    ("zeros", "p1000", "method1"): (0, 0), ("zeros", "p1000", "method2"): (0, 0),
    ("nonfinite", "p1000", "method1"): (1, 2), ("nonfinite", "p1000", "method2"): (1, 1),
    ("tiny", "p1000", "method1"): (0, 0), ("tiny", "p1000", "method2"): (0, 0),
    ("huge", "p1000", "method1"): (0, 1), ("huge", "p1000", "method2"): (9, 1),
    ("ladder", "p1000", "method1"): (1, 0), ("ladder", "p1000", "method2"): (1, 0),
}
# the ladder's band variant, at the sizes whose joins run the pruned kernels for long
BAND_TABLE_CASES = {("ladder", "p1000", "method1"): (0, 1), ("ladder", "p1000", "method2"): (0, 1),
                    ("ladder", "p5000", "method1"): (0, 1), ("ladder", "p5000", "method2"): (0, 1)}
# the nonfinite family with mirrored NaN cells, signed method, by what table[0][0] is (g00: 0 NaN, 1 negative, 2 +inf: what
# the pruned kernels' staircase of an empty half is built from): (size, g00) -> (seed, variant)
MIRRORED_TABLE_CASES = {("p70", 0): (3, 3), ("p70", 1): (2, 4), ("p70", 2): (0, 5),
                        ("p1000", 0): (1, 3), ("p1000", 1): (1, 4), ("p1000", 2): (0, 5),
                        ("p5000", 0): (0, 3), ("p5000", 1): (0, 4), ("p5000", 2): (0, 5)}
WIDE_TABLE_CASES = {
    ("nonfinite", "p5000", "method1"): (0, 1), ("nonfinite", "p5000", "method2"): (0, 0),
    ("huge", "p5000", "method1"): (0, 0), ("huge", "p5000", "method2"): (7, 0),
    ("ladder", "p5000", "method1"): (3, 0), ("ladder", "p5000", "method2"): (1, 0),
}


# ---- the table families through the sequential entries (tests/test_seq_tables_host.py, tests/test_gpu_seq_tables.py) ------
# The inputs are those of tests/test_gpu_sequential.py (make_input, 70 + 61 patients, one stratum, permutation seed 11, 5
# hits, at most 3,000 permutations); the table is special_table(family, ..., seed, variant), for the family "shapes"
# shape_tables(..., seed)[SEQ_SHAPE_NAMES[variant]].  "huge+hi" / "huge+mid" are the huge table with one planted cell under
# the observed counts of set 3: a finite score beyond FLT_OVERFLOW, and one between FLT_MAX and FLT_OVERFLOW.
SEQ_SHAPE_NAMES = ("0x0", "1x1", "few_rows", "few_cols", "few_both", "larger", "square")
SEQ_PLANTED = {"huge+hi": 3.5e38, "huge+mid": FLT_MAX + 2.0 ** 102}
SEQ_ENTRIES = ("sequential", "weighted", "prefix", "dose")
# (entry, family, method) -> [(table seed, variant, trial of make_input, max_perms)]: found on the CPU by
# tools/seq_table_seeds.py so that the numpy definitions alone meet what tests/test_seq_tables_host.py asks of every case
_SHAPE_SPECS = [(0, v, 0, 3000) for v in range(len(SEQ_SHAPE_NAMES))]
SEQ_TABLE_CASES = {
    ("sequential", "zeros", 1): [(0, 0, 0, 3000)],
    ("sequential", "zeros", 2): [(1, 0, 0, 1562)],
    ("sequential", "nonfinite", 1): [(0, 0, 0, 3000), (0, 1, 0, 3000), (0, 2, 0, 3000)],
    ("sequential", "nonfinite", 2): [(1, 0, 0, 3000), (0, 1, 0, 3000), (0, 2, 0, 3000), (0, 3, 0, 3000), (0, 4, 0, 3000),
                                     (0, 5, 0, 3000)],
    ("sequential", "tiny", 1): [(0, 0, 0, 3000)],
    ("sequential", "tiny", 2): [(2, 0, 1, 3000)],
    ("sequential", "huge", 1): [(0, 0, 0, 3000), (3, 1, 0, 3000)],
    ("sequential", "huge", 2): [(0, 0, 0, 3000), (5, 1, 7, 3000)],
    ("sequential", "huge+hi", 1): [(0, 0, 0, 3000)],
    ("sequential", "huge+hi", 2): [(0, 0, 0, 3000)],
    ("sequential", "huge+mid", 1): [(0, 1, 0, 3000)],
    ("sequential", "huge+mid", 2): [(0, 1, 0, 3000)],
    ("sequential", "ladder", 1): [(1, 0, 0, 3000), (0, 1, 0, 3000)],
    ("sequential", "ladder", 2): [(3, 0, 0, 3000), (5, 1, 1, 3000)],
    ("sequential", "shapes", 1): _SHAPE_SPECS,
    ("sequential", "shapes", 2): _SHAPE_SPECS,
    ("weighted", "zeros", 1): [(0, 0, 0, 1137)],
    ("weighted", "zeros", 2): [(1, 0, 0, 3000)],
    ("weighted", "nonfinite", 1): [(0, 2, 0, 3000)],
    ("weighted", "nonfinite", 2): [(0, 2, 0, 3000)],
    ("weighted", "huge", 1): [(3, 1, 0, 3000)],
    ("weighted", "huge", 2): [(1, 1, 65, 3000)],
    ("weighted", "shapes", 1): [(0, 4, 0, 3000)],
    ("weighted", "shapes", 2): [(0, 4, 0, 3000)],
    ("prefix", "zeros", 1): [(1, 0, 1, 3000)],
    ("prefix", "zeros", 2): [(2, 0, 0, 3000)],
    ("prefix", "nonfinite", 1): [(0, 0, 0, 3000), (0, 1, 1, 3000), (4, 2, 0, 3000)],
    ("prefix", "nonfinite", 2): [(1, 0, 0, 3000), (4, 1, 1, 736), (2, 2, 0, 3000), (0, 3, 0, 3000), (4, 4, 0, 3000),
                                 (2, 5, 0, 3000)],
    ("prefix", "tiny", 1): [(0, 0, 0, 3000)],
    ("prefix", "tiny", 2): [(2, 0, 0, 3000)],
    ("prefix", "huge", 1): [(0, 0, 0, 3000), (0, 1, 0, 3000)],
    ("prefix", "huge", 2): [(0, 0, 0, 3000), (0, 1, 0, 3000)],
    ("prefix", "huge+hi", 1): [(0, 0, 0, 3000)],
    ("prefix", "huge+hi", 2): [(0, 0, 0, 3000)],
    ("prefix", "huge+mid", 1): [(0, 1, 0, 3000)],
    ("prefix", "huge+mid", 2): [(0, 1, 0, 3000)],
    ("prefix", "ladder", 1): [(1, 0, 0, 3000), (0, 1, 0, 3000)],
    ("prefix", "ladder", 2): [(3, 0, 0, 3000), (1, 1, 0, 3000)],
    ("prefix", "shapes", 1): _SHAPE_SPECS,
    ("prefix", "shapes", 2): _SHAPE_SPECS,
    ("dose", "zeros", 1): [(1, 0, 0, 3000)],
    ("dose", "zeros", 2): [(2, 0, 0, 3000)],
    ("dose", "nonfinite", 1): [(0, 0, 0, 1662), (0, 1, 0, 3000), (0, 2, 0, 3000)],
    ("dose", "nonfinite", 2): [(1, 0, 0, 3000), (0, 1, 0, 3000), (3, 2, 1, 3000), (1, 3, 0, 3000), (0, 4, 0, 3000),
                               (0, 5, 0, 3000)],
    ("dose", "tiny", 1): [(0, 0, 0, 3000)],
    ("dose", "tiny", 2): [(2, 0, 1, 3000)],
    ("dose", "huge", 1): [(0, 0, 0, 3000), (1, 1, 0, 3000)],
    ("dose", "huge", 2): [(0, 0, 0, 3000), (1, 1, 0, 3000)],
    ("dose", "huge+hi", 1): [(0, 0, 0, 3000)],
    ("dose", "huge+hi", 2): [(0, 0, 0, 3000)],
    ("dose", "huge+mid", 1): [(0, 1, 0, 3000)],
    ("dose", "huge+mid", 2): [(0, 1, 0, 3000)],
    ("dose", "ladder", 1): [(1, 0, 0, 3000), (4, 1, 0, 3000)],
    ("dose", "ladder", 2): [(3, 0, 0, 3000), (1, 1, 0, 3000)],
    ("dose", "shapes", 1): _SHAPE_SPECS[:3] + [(0, 3, 5, 3000)] + _SHAPE_SPECS[4:],
    ("dose", "shapes", 2): _SHAPE_SPECS,
}


def table_problem(kind: str, size: str, method: str, top_k: int = 3000, table=None, case=None) -> Problem:
    """The problem of a table test.  ``case`` = (seed, variant): the table is special_table(kind, ..., seed, variant) unless
    ``table`` is given, and the network is drawn from the same seed; by default the case TABLE_CASES / WIDE_TABLE_CASES name."""
    genes, edges, nc, nt, perms, length, threshold = TABLE_SIZES[size]
    seed, variant = case if case is not None else {**TABLE_CASES, **WIDE_TABLE_CASES}.get((kind, size, method), (0, 0))
    if table is None:
        table = special_table(kind, nc, nt, seed, variant)
    return make_problem(genes, edges, nc, nt, perms, length, method=method, top_k=top_k, seed=40 + seed, threshold=threshold,
                        table=table)


def zeros_cut_top_k(all_scores: np.ndarray) -> int:
    """The top_k that puts the cut of a level in the middle of its zero-scored paths (0 if the level has fewer than two)."""
    positive = int((all_scores > 0).sum())
    zero = int((all_scores == 0).sum())
    return positive + zero // 2 if zero >= 2 else 0


def assert_same_result(got, want, check_ids: bool = True):
    """got: geneticscre_amd.api.JoinResult; want: oracle.OracleResult in canonical order.  Bit-exact."""
    assert got.scores.dtype == np.float64
    np.testing.assert_array_equal(got.scores.view(np.uint64), want.scores.view(np.uint64))
    np.testing.assert_array_equal(got.cases, want.cases)
    np.testing.assert_array_equal(got.ctrls, want.ctrls)
    if check_ids:
        np.testing.assert_array_equal(got.src, want.src)
        np.testing.assert_array_equal(got.trg, want.trg)
    assert got.null.dtype == np.float32
    np.testing.assert_array_equal(got.null.view(np.uint32), want.null.view(np.uint32))


def fnv_rows(rows: np.ndarray) -> str:
    """FNV-1a over the uint64 words of a kept path set, as oracle/ref_partial/ref_driver.cpp hashes them."""
    h = 1469598103934665603
    for w in np.ascontiguousarray(rows, dtype=np.uint64).ravel().tolist():
        h ^= w
        h = (h * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def load_ref_cases():
    """(name, Problem, expected dict) for every golden generated from the partial reference build."""
    import json
    import os
    from geneticscre_amd.harness_io import read_problem

    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_cases")
    out = []
    for name in json.load(open(os.path.join(d, "INDEX.json")))["cases"]:
        exp = json.load(open(os.path.join(d, name + ".json")))
        c = exp["_case"]
        p = read_problem(os.path.join(d, name + ".txt"), method=c["method"], iterations=c["iterations"],
                         top_k=c["top_k"], path_length=c["path_length"])
        out.append((name, p, exp))
    return out


# ---- goldens at BASELINE mask widths (tests/golden/ref_cases/w*.json) ------------------------------------------------
# The reference's own scoring code (oracle/ref_partial) run on problems too large to commit as text: 16, 79 and 157 mask
# words (BASELINE configs[1], [2], [3]), both methods, the hypergeometric value table.  Only the outputs are committed;
# the inputs are regenerated from the seed by the same generator call, and their SHA-256 is checked against the one
# recorded when the golden was cut, so a drifting generator fails loudly.
WIDE_CASES = {
    # name: method, genes, edges, cases, ctrls, permutations, length, top_k, seed
    "w16_m1": ("method1", 200, 700, 460, 540, 300, 4, 20, 211),
    "w16_m2": ("method2", 200, 700, 460, 540, 300, 4, 20, 212),
    "w79_m1": ("method1", 200, 700, 2400, 2600, 300, 4, 20, 213),
    "w79_m2": ("method2", 200, 700, 2400, 2600, 300, 4, 20, 214),
    "w157_m1": ("method1", 200, 700, 4300, 5700, 300, 4, 20, 215),
    "w157_m2": ("method2", 200, 700, 4300, 5700, 300, 4, 20, 216),
    # round 4: path length 5 (paths3 x paths3, src/wrapper.cpp:271-276) at the width of configs[2], both methods, and the
    # signed method at 313 words (20,000 patients: the sorted-prefix-sum form of the native table builder)
    "w79_m1_len5": ("method1", 110, 300, 2450, 2550, 300, 5, 20, 217),
    "w79_m2_len5": ("method2", 110, 300, 2450, 2550, 300, 5, 20, 218),
    "w313_m2": ("method2", 70, 200, 9400, 10600, 150, 4, 20, 219),
}
# goldens whose reference run takes minutes (the reference's signed method copies and symmetrises its padded (n+1)^2 table
# once per join, src/methods.h:128: 230 s at 20,000 patients): committed like the others, checked against the oracle and
# the GPU like the others, but cut again by test_committed_goldens_regenerate only under GCRE_SLOW_GOLDENS=1
SLOW_WIDE_CASES = {"w313_m2"}
_WIDE_TABLES: dict = {}
_WIDE_PROBLEMS: dict = {}


def wide_problem(name: str) -> Problem:
    """The inputs of a wide golden, rebuilt from its seed (cached per session; the 10,000-patient table takes ~15 s)."""
    if name not in _WIDE_PROBLEMS:
        from geneticscre_amd import api
        method, genes, edges, nc, nt, perms, length, top_k, seed = WIDE_CASES[name]
        if (nc, nt) not in _WIDE_TABLES:
            _WIDE_TABLES[(nc, nt)] = api.values_table(nc, nt)
        _WIDE_PROBLEMS[name] = make_problem(genes, edges, nc, nt, perms, length, method=method, top_k=top_k, seed=seed,
                                            table=_WIDE_TABLES[(nc, nt)])
    return _WIDE_PROBLEMS[name]


# ---- goldens of the oracle fuzz (tests/golden/ref_cases/fuzz*.json) -------------------------------------------------
# The first cases of tests/test_oracle_fuzz.py with the outputs the reference's own scoring code printed for them, so that
# the default run compares against the reference without its source tree.  As for the wide goldens, only the outputs are
# committed: the inputs are redrawn and their SHA-256 is checked against the one recorded with the golden.
FUZZ_GOLDEN_CASES = 4


def fuzz_problem(case: int):
    """(cfg, Problem) of tests/test_oracle_fuzz.py case ``case``: the draw of tests/test_gpu_fuzz.py case 400000 + case,
    cut to what the reference's inline mode runs in seconds."""
    from test_gpu_fuzz import draw, value_table
    cfg, _ = draw(400000 + case)
    perms = max(1, min(cfg["perms"], 600))   # the reference's inline mode is one thread (K = 0 is a golden of its own)
    if cfg["n_cases"] + cfg["n_ctrls"] > 3000:
        perms = min(perms, 100)
    cfg["perms"] = perms
    if (cfg["n_cases"] + cfg["n_ctrls"]) % 64 == 0:
        # PathSet::load asserts patients < 64 * width (src/gcre_paths.h:63).  The reference pads the width to its SIMD
        # width (src/join_base.cpp:15-23), so it refuses cohorts of exactly k * gs_vec_width patients; the driver's width is
        # ceil(n / 64) (the padding is layout only), so it refuses every multiple of 64: an error there, nothing to compare
        cfg["n_ctrls"] += 1
    p = make_problem(cfg["genes"], cfg["edges"], cfg["n_cases"], cfg["n_ctrls"], perms, cfg["length"], method=cfg["method"],
                     top_k=cfg["top_k"], seed=cfg["seed"], threshold=cfg["threshold"],
                     table=value_table(cfg["table"], cfg["n_cases"], cfg["n_ctrls"], cfg["seed"]))
    return cfg, p


def load_wide_case(name: str):
    """(Problem, expected dict) of a wide golden; fails if the regenerated inputs are not the ones the golden was cut from."""
    import json
    import os
    from geneticscre_amd.harness_io import problem_digest
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_cases")
    exp = json.load(open(os.path.join(d, name + ".json")))
    p = wide_problem(name)
    assert problem_digest(p) == exp["_case"]["input_sha256"], f"{name}: the generator no longer reproduces the golden's inputs"
    return p, exp


# ---- goldens of the special-value tables (tests/golden/ref_cases/table_*.json) ----------------------------------------
# One case per table family and method at the 70-patient size, through the reference's own scoring code: what a NaN, an
# infinity, a signed zero, a denormal or a padded cell does to scores, heap order and f32 maxima is the reference's to say.
# Outputs only, inputs regenerated and checked by SHA-256, like the wide and the fuzz goldens.
TABLE_GOLDEN_CASES = [f"table_{kind}_{m}" for kind in TABLE_FAMILIES for m in ("m1", "m2")]


GOLDEN_PERMS = 24      # of the cohort's 300: a golden is a few kB, and the reference's inline mode takes no time


def table_golden_problem(name: str) -> Problem:
    _, kind, m = name.split("_")
    method = "method1" if m == "m1" else "method2"
    table, top_k = None, 12
    if kind == "shapes":     # fewer rows and fewer columns than the cohort needs: the padding is read in every level
        table = dict((n, t) for n, t, _ in shape_tables(37, 33))["few_both"]
    if kind == "zeros":      # the smallest top_k that puts some level's cut among its zeros
        from oracle import process_paths
        full = process_paths(table_problem(kind, "p70", method), order="canonical")
        top_k = min(k for k in (zeros_cut_top_k(full[f"lst{l}"].all_scores) for l in range(1, 6)) if k)
    p = table_problem(kind, "p70", method, top_k=top_k, table=table)
    p.perm_cases, p.iterations = p.perm_cases[:GOLDEN_PERMS].copy(), GOLDEN_PERMS
    return p


def load_table_case(name: str):
    """(Problem, expected dict) of a table golden; fails if the regenerated inputs are not the ones the golden was cut from."""
    import json
    import os
    from geneticscre_amd.harness_io import problem_digest
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_cases")
    exp = json.load(open(os.path.join(d, name + ".json")))
    p = table_golden_problem(name)
    assert problem_digest(p) == exp["_case"]["input_sha256"], f"{name}: the generator no longer reproduces the golden's inputs"
    return p, exp
