"""The special-value table families of tests/helpers.py, host side: the two rules the families exist for, stated in numpy
on a hand-worked table, and the conditions under which a GPU test on a family is not vacuous, asserted on the CPU oracle's
own results for every (family, size, method) that tests/test_gpu_tables.py runs.  A generator that drifts fails here, loudly,
instead of quietly no longer reaching the branch it was written for.  No GPU needed."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from helpers import (BAND_TABLE_CASES, FLT_DENORM, FLT_MAX, FLT_MIN, FLT_OVERFLOW, MIRRORED_TABLE_CASES, TABLE_CASES, TABLE_SIZES, WIDE_TABLE_CASES,
                     shape_tables, special_table,
                     table_problem, zeros_cut_top_k)

NAN = np.nan


# ---- the two rules ---------------------------------------------------------------------------------------------------
def vtmax_rule(t):
    """The signed method's table (compute_value_table_max, methods.h:110-118): std::max(t[r][c], t[c][r]), which is
    ``a < b ? b : a`` -- a NaN in the first argument stays, a NaN in the second is dropped."""
    a, b = np.asarray(t, np.float64), np.asarray(t, np.float64).T
    return np.where(a < b, b, a)


def null_fold(p):
    """What a permutation's score adds to the f32 null maximum, which starts at +0: rounded to f32, kept if > 0."""
    with np.errstate(over="ignore"):
        f = np.asarray(p, np.float64).astype(np.float32)
    return np.where(f > 0, f, np.float32(0)).astype(np.float32)


def test_the_two_rules_on_a_hand_worked_table():
    t = np.array([[1.0, NAN, 5.0],
                  [2.0, -0.0, NAN],
                  [7.0, 3.0, -np.inf]])
    m = vtmax_rule(t)
    # (0,1) holds NaN and (1,0) holds 2: vtmax[0][1] = max(NaN, 2) = NaN, vtmax[1][0] = max(2, NaN) = 2 -- not symmetric
    assert np.isnan(m[0, 1]) and m[1, 0] == 2.0
    assert np.isnan(m[1, 2]) and m[2, 1] == 3.0
    assert m[0, 2] == 7.0 and m[2, 0] == 7.0 and m[0, 0] == 1.0 and m[2, 2] == -np.inf
    assert m[1, 1] == 0 and np.signbit(m[1, 1])
    assert not np.array_equal(np.isnan(m), np.isnan(np.maximum(t, t.T)))     # np.maximum propagates NaN both ways
    f = null_fold([NAN, -np.inf, -0.0, -3.0, 0.7e-45, 1.4e-45, FLT_MIN, FLT_MAX, np.nextafter(FLT_OVERFLOW, 0.0),
                   FLT_OVERFLOW, 1e300, np.inf])
    assert f[:5].view(np.uint32).tolist() == [0, 0, 0, 0, 0]                 # NaN, negatives and -0 fold to +0
    assert f[5] == np.float32(FLT_DENORM) and f[6] == np.float32(FLT_MIN)    # denormals are kept, not flushed
    assert f[7] == f[8] == np.float32(FLT_MAX) and np.isinf(f[9:]).all()


def test_families_are_deterministic_and_hold_what_they_say():
    for kind in ("zeros", "nonfinite", "tiny", "huge", "ladder"):
        a, b = special_table(kind, 37, 33, 5), special_table(kind, 37, 33, 5)
        assert a.shape == (38, 34) and np.array_equal(a.view(np.uint64), b.view(np.uint64))
        assert not np.array_equal(a.view(np.uint64), special_table(kind, 37, 33, 6).view(np.uint64))
    z = special_table("zeros", 460, 540, 0)
    assert ((z == 0) & np.signbit(z)).mean() > 0.2 and ((z == 0) & ~np.signbit(z)).mean() > 0.2 and (z < 0).any()
    assert ((z > 0) & (z < 1e-15)).any()
    for v, want in enumerate((np.isnan, lambda x: x < 0, lambda x: x == np.inf)):
        nf = special_table("nonfinite", 460, 540, 0, variant=v)
        assert want(nf[0, 0])
        nan = np.isnan(nf)
        assert np.triu(nan[:400, :400], 1).any() and np.tril(nan[:400, :400], -1).any()
        assert 0.02 < nan.mean() < 0.06 and 0.02 < (nf == -np.inf).mean() < 0.06 and 0 < (nf == np.inf).mean() < 0.003
    t = special_table("tiny", 460, 540, 0)
    assert t.min() >= 1e-50 and t.max() <= 1.2e-38
    for cell in (0.7e-45, 1.4e-45, np.nextafter(FLT_MIN, 0.0), np.nextafter(FLT_MIN, 1.0), 2.0 ** -150):
        assert (t == cell).any()
    frac = t / FLT_DENORM
    assert ((frac - np.floor(frac) == 0.5) & (frac > 1)).any()                # halfway between two denormals
    h = special_table("huge", 460, 540, 0)
    assert h.min() >= 1e38 and h.max() <= 3.5e38
    for cell in (FLT_MAX, np.nextafter(FLT_OVERFLOW, 0.0), FLT_OVERFLOW, FLT_MAX / 2, FLT_MAX / 2 + 2.0 ** 103):
        assert (h == cell).any()
    assert null_fold(np.nextafter(FLT_OVERFLOW, 0.0)) == np.float32(FLT_MAX) and np.isinf(null_fold(FLT_OVERFLOW))
    assert np.isinf(null_fold(FLT_MAX / 2 + (FLT_MAX / 2 + 2.0 ** 103))) and null_fold(FLT_MAX / 2 + FLT_MAX / 2) == np.float32(FLT_MAX)
    assert (special_table("huge", 460, 540, 0, variant=1) == 1e300).any()
    lad = special_table("ladder", 460, 540, 0)
    assert -FLT_DENORM <= lad.min() < 0                        # (one f32 ulp below level 0)
    assert 49 < lad.max() <= 50.001 and (lad == 0).mean() > 0.25
    on8, f32 = lad * 8 == np.round(lad * 8), lad.astype(np.float32).astype(np.float64)
    assert on8.any() and (lad * 16 == np.round(lad * 16)).mean() > 0.3
    assert (np.ceil(16 * lad) != np.ceil(16 * f32)).any()                     # the f32 image is on the other side of a level
    assert (np.ceil(8 * lad) != np.ceil(8 * f32)).any()
    names = [n for n, _, _ in shape_tables(37, 33)]
    assert names == ["0x0", "1x1", "few_rows", "few_cols", "few_both", "larger", "square"]


def padded_vtmax(t, n):
    """vtmax of the (n + 1)^2 copy the reference pads with -1 (join_base.cpp:67-78)."""
    pad = np.full((n + 1, n + 1), -1.0)
    pad[:t.shape[0], :t.shape[1]] = t
    return vtmax_rule(pad)


def test_which_nonfinite_variants_keep_vtmax_symmetric():
    """A NaN on one side of the diagonal only makes the signed method's vtmax differ from its transpose; the library then
    scores permutations by the dense kernel alone (gcre_set_value_table).  Variants 0-2 of the nonfinite family are such
    tables; variants 3-5 mirror their NaN cells, so that vtmax is symmetric, NaN included, and the pruned kernels run."""
    same = lambda m: np.array_equal(np.isnan(m), np.isnan(m.T)) and np.array_equal(m[~np.isnan(m)], m.T[~np.isnan(m)])
    for size, (_, _, nc, nt, _, _, _) in TABLE_SIZES.items():
        if size == "p5000":
            continue        # (a 5,051^2 padded copy: the generator is the same)
        for v in range(6):
            t = special_table("nonfinite", nc, nt, 1, v)
            m = padded_vtmax(t, nc + nt)
            assert same(m) == (v >= 3), (size, v)
            nan = np.isnan(t)
            assert np.triu(nan, 1).any() and np.tril(nan, -1).any() and 0.02 < nan.mean() < 0.06, (size, v)
            assert (t == -np.inf).any() and (np.isnan, lambda x: x < 0, lambda x: x == np.inf)[v % 3](t[0, 0])
    for (size, g00), (seed, variant) in MIRRORED_TABLE_CASES.items():
        assert variant == 3 + g00
        if size != "p5000":
            nc, nt = TABLE_SIZES[size][2:4]
            assert same(padded_vtmax(special_table("nonfinite", nc, nt, seed, variant), nc + nt)), (size, g00)


# ---- what each family has to provoke in the oracle's results ---------------------------------------------------------
def signed_zero_counts(x):
    z = x == 0
    return int((z & np.signbit(x)).sum()), int((z & ~np.signbit(x)).sum())


def check_conditions(kind, size, p, res, g00=None):
    """The non-vacuity conditions of the family ``kind`` on the oracle's canonical results ``res`` of problem ``p``.
    ``g00``: for the signed method's mirrored nonfinite cases, what table[0][0] = vtmax[0][0] is -- the cell an empty half
    reads.  With a NaN there (g00 = 0) every one-gene path scores NaN + x in every permutation, which folds to +0: level 1
    has the single maximum +0 by arithmetic, and the count of distinct maxima is asked from level 2 up.  With +inf there
    (g00 = 2) one path with an empty half makes every permutation's maximum +inf: that all maxima are +inf is then what is
    asserted, in place of the shares of finite ones, which no generator can meet."""
    levels = range(1, p.path_length + 1)
    null = {l: res[f"lst{l}"].null for l in levels}
    every = {l: res[f"lst{l}"].all_scores for l in levels}
    big = size == "p1000"      # (where the counts of distinct values are asked for)
    if kind == "zeros":
        both = [l for l in levels if min(signed_zero_counts(res[f"lst{l}"].scores)) > 0]
        assert len(both) >= 2, f"both zeros in the top-k list of levels {both} only"
        assert any(zeros_cut_top_k(every[l]) for l in levels), "no level where a cut can fall among the zeros"
    elif kind == "nonfinite" and g00 == 2:
        for l in levels:
            assert (null[l] == np.inf).all(), l
            if l >= 2:
                assert np.isnan(every[l]).any() and (every[l] == -np.inf).any() and np.isfinite(every[l]).any(), l
    elif kind == "nonfinite":
        for l in levels:
            fin = np.isfinite(null[l])
            assert fin.mean() >= 0.5, (l, fin.mean())
            if g00 == 0 and l == 1:
                assert (null[l].view(np.uint32) == 0).all()
            elif big:
                assert len(np.unique(null[l][fin])) >= 8, (l, len(np.unique(null[l][fin])))
            if l >= 2:
                assert np.isnan(every[l]).any() and (every[l] == -np.inf).any(), l
        assert any((null[l] == np.inf).any() for l in levels)
    elif kind == "tiny":
        for l in levels:
            den = (null[l] > 0) & (null[l] < np.float32(FLT_MIN))
            assert den.mean() >= 0.5, (l, den.mean())
            assert len(np.unique(null[l])) >= 4, (l, np.unique(null[l]))
    elif kind == "huge":
        assert any((null[l] == np.float32(FLT_MAX)).any() and (null[l] == np.inf).any() for l in levels)
        for l in levels:
            assert np.isfinite(null[l]).any(), l
    elif kind == "ladder":
        for l in levels:
            if l >= 2:
                assert (null[l] < 22).any() and ((null[l] >= 22) & (null[l] <= 32)).any() and (null[l] > 32).any(), \
                    (l, null[l].min(), null[l].max())
            if big:
                assert len(np.unique(null[l])) >= 8, l
    else:
        raise ValueError(kind)


@pytest.mark.parametrize("kind,size,method", list(TABLE_CASES), ids=lambda v: str(v))
def test_family_meets_its_conditions_on_the_oracle(kind, size, method):
    p = table_problem(kind, size, method)
    check_conditions(kind, size, p, oracle.process_paths(p, order="canonical", nthreads=4))


@pytest.mark.parametrize("kind,size,method", list(WIDE_TABLE_CASES), ids=lambda v: str(v))
def test_family_meets_its_conditions_at_the_baseline_mask_width(kind, size, method):
    p = table_problem(kind, size, method, top_k=50)
    check_conditions(kind, size, p, oracle.process_paths(p, order="canonical", nthreads=8))


@pytest.mark.parametrize("size,g00", list(MIRRORED_TABLE_CASES), ids=lambda v: str(v))
def test_mirrored_nonfinite_meets_its_conditions_on_the_oracle(size, g00):
    """The signed method on the nonfinite family with mirrored NaN cells, for a NaN, a negative and a +inf table[0][0]."""
    p = table_problem("nonfinite", size, "method2", top_k=50, case=MIRRORED_TABLE_CASES[(size, g00)])
    check_conditions("nonfinite", size, p, oracle.process_paths(p, order="canonical", nthreads=8), g00=g00)


@pytest.mark.parametrize("kind,size,method", list(BAND_TABLE_CASES), ids=lambda v: str(v))
def test_ladder_band_keeps_the_maxima_within_a_few_steps(kind, size, method):
    """The band variant of the ladder family: from level 2 up every maximum lies under its ladder's top (32, and 22 for the
    signed method), the maxima of a level span at most two units, and at least three ladder steps (1/8) hold two or more
    distinct maxima each -- values that only an exact look-up tells apart: a ladder row that admits a cell one step too
    early loses the larger of them."""
    p = table_problem(kind, size, method, top_k=50, case=BAND_TABLE_CASES[(kind, size, method)])
    res = oracle.process_paths(p, order="canonical", nthreads=8)
    for l in range(2, p.path_length + 1):
        n = res[f"lst{l}"].null.astype(np.float64)
        assert n.max() < (32 if method == "method1" else 22) and n.max() - n.min() <= 2, (l, n.min(), n.max())
        steps = np.floor(np.unique(n) * 8)
        assert (np.unique(steps, return_counts=True)[1] >= 2).sum() >= 3, (l, np.unique(n)[:12])


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_zeros_cut_falls_among_the_zeros(method):
    """With the top_k that helpers.zeros_cut_top_k names, the lowest kept score is a zero and zero-scored paths stay out;
    the kept zeros are those of the smallest ordinals, whatever their sign."""
    full = oracle.process_paths(table_problem("zeros", "p70", method), order="canonical")
    hit = 0
    for lvl in range(2, 6):
        k = zeros_cut_top_k(full[f"lst{lvl}"].all_scores)
        if not k:
            continue
        r = oracle.process_paths(table_problem("zeros", "p70", method, top_k=k), order="canonical")[f"lst{lvl}"]
        a = r.all_scores
        assert r.scores[0] == 0 and (a == 0).sum() > (r.scores == 0).sum() > 0
        assert len(r.scores) == k
        neg, pos = signed_zero_counts(r.scores)
        hit += neg > 0 and pos > 0
    assert hit >= 1, "no cut with both zeros on the kept side"


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_undersized_tables_reach_the_padding(method):
    """Every table smaller than the cohort needs: some observed score is the -1 the reference pads with."""
    for name, table, undersized in shape_tables(37, 33):
        p = table_problem("shapes", "p70", method, table=table)
        res = oracle.process_paths(p, order="canonical")
        # the table is positive, so a negative score has read a padded cell: exactly -1 with method 1; with the signed method,
        # which adds two cells, exactly -2 or -1 + a cell of the table
        neg = np.concatenate([res[f"lst{l}"].all_scores for l in range(1, 6)])
        neg = neg[neg < 0]
        if method == "method1":
            assert (neg == -1.0).all(), name
        else:
            assert np.isin(neg, np.concatenate([[-2.0], -1.0 + table.ravel()])).all(), name
        if undersized:
            assert len(neg) > 0, name
        else:
            assert len(neg) == 0, name
