"""Carrier tallies per patient on the device (gcre_set_patient_counts: k_set_patient_counts) against
``report.patient_counts_reference``: counts, group_sets and skipped, every comparison exact integer equality (pytest -m gpu).
The hand-worked cases of the definition itself are in tests/test_patients_host.py.

A context needs at least one case and one control (gcre_create), so the smallest cohort a call can see has 2 patients and
n_cases lies in 1 .. n - 1: the patient counts below start at 2 and take n_cases at both of those ends.

GCRE_PATIENT_FUZZ_CASES=300 [GCRE_PATIENT_FUZZ_BASE=...] for a long run of the seeded loop at the end
(GCRE_PATIENT_FUZZ_OUT: a file for its summary); a handful by default."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from geneticscre_amd import api, report, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = int(re.search(r"constexpr int kPatientPlanes = (\d+);",
                       open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_kernels.h")).read()).group(1))


def same(got, want, what=""):
    """(counts, group_sets, skipped) against the reference's, as integers."""
    assert got[0].dtype == np.int32 and got[0].shape == want[0].shape, (what, got[0].shape, want[0].shape)
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"counts {what}")
    np.testing.assert_array_equal(np.asarray(got[1], np.int64), want[1], err_msg=f"group_sets {what}")
    assert int(got[2]) == int(want[2]), f"skipped {what}"


def check(ex, sets, rows, which=None, group=None, n_groups=None, by_sign=False, signs=None, what=""):
    n = np.asarray(rows).shape[1]
    got = ex.patient_counts(sets, rows, which, group, n_groups, by_sign, signs)
    want = report.patient_counts_reference(sets, rows, signs, which, group, n_groups, n, by_sign)
    same(got, want, what)
    return got


def random_sets(rng, R, S, max_members=5, na=0.0):
    sets = [rng.integers(0, R, int(rng.integers(1, max_members + 1))).tolist() for _ in range(S)]
    for s in sets:
        if rng.random() < na:
            s[int(rng.integers(0, len(s)))] = -1
    return sets


def random_signs(rng, sets):
    return [rng.choice([1, -1], len(s)).tolist() for s in sets]


def raw_patients(ex, sets, packed, n_cols, which, group, n_groups=1, by_sign=0, signs=None, n_which=None, want_counts=True,
                 want_extras=True):
    """gcre_set_patient_counts through the C entry: (rc, counts, group_sets, skipped); the outputs start as -7."""
    lib = api._patients_lib()
    S = len(sets)
    off = np.zeros(S + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in sets])
    mem = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int64) for s in sets]) if S else np.zeros(0), np.int32)
    sg = None if signs is None else np.ascontiguousarray(np.concatenate([np.asarray(s, np.int64) for s in signs]), np.int32)
    iw = None if which is None else np.ascontiguousarray(which, np.int64)
    ig = None if group is None else np.ascontiguousarray(group, np.int32)
    if n_which is None:
        n_which = S if iw is None else len(iw)
    inp = api.gcre_set_input(S, api._ptr(off), api._ptr(mem), api._ptr(sg), api._ptr(packed), len(packed), n_cols)
    H = 2 if by_sign == 1 else 1
    counts = np.full((max(int(n_groups), 1), H, n_cols), -7, np.int32) if want_counts else None
    group_sets = np.full(max(int(n_groups), 1), -7, np.int64) if want_extras else None
    skipped = ctypes.c_int64(-7)
    rc = lib.gcre_set_patient_counts(ex._h, ctypes.byref(inp), api._ptr(iw), n_which, api._ptr(ig), n_groups, by_sign,
                                     api._ptr(counts), api._ptr(group_sets), ctypes.byref(skipped) if want_extras else None)
    return rc, counts, group_sets, skipped.value


# ---- 1. patient counts: the partial last dword, the second tile, stray bits ------------------------------------------------------

# n_cases off a dword boundary, and once at each end a context admits
@pytest.mark.parametrize("n,nc", [(2, 1), (31, 13), (32, 1), (33, 32), (77, 45), (2048, 1000), (2085, 1037)])
def test_patient_counts(n, nc):
    rng = np.random.default_rng(100 + n)
    R, S = 9, 70
    W = -(-n // 64)
    wide = (rng.random((R, W * 64)) < 0.35).astype(np.int8)
    wide[:, n:] = 1                                        # bits beyond n_cols: they are not patients
    wide[0, :n] = 1                                        # one gene everybody carries: the last patient is counted
    rows = wide[:, :n]
    packed = api.pack_carriers(wide, W * 64)
    assert packed.shape == (R, W) and (n % 64 == 0 or (packed[:, -1] >> np.uint64(n % 64)).all())
    sets = random_sets(rng, R, S, na=0.1)
    sets[0] = [0]
    signs = random_signs(rng, sets)
    which = rng.integers(0, S, 150)
    group = rng.integers(-1, 3, 150)
    ex = api.JoinExec(1, nc, n - nc, 0)
    try:
        for by_sign in (0, 1):
            want = report.patient_counts_reference(sets, rows, signs, which, group, 3, n, by_sign)
            rc, counts, group_sets, skipped = raw_patients(ex, sets, packed, n, which, group, 3, by_sign, signs)
            assert rc == api.GCRE_OK, ex._lib.gcre_last_error(ex._h)
            same((counts, group_sets, skipped), want, f"n {n} by_sign {by_sign}")
            assert want[0][:, 0, n - 1].sum() > 0
            check(ex, sets, rows, which, group, 3, bool(by_sign), signs, f"n {n} by_sign {by_sign} (method)")
        # group_sets and skipped may be NULL
        rc, counts, _, _ = raw_patients(ex, sets, packed, n, which, group, 3, 0, want_extras=False)
        assert rc == api.GCRE_OK
        np.testing.assert_array_equal(counts, report.patient_counts_reference(sets, rows, None, which, group, 3, n, False)[0])
    finally:
        ex.close()
    if n == 2:   # why there is no n = 1
        with pytest.raises(ValueError, match="num_ctrls > 0"):
            api.JoinExec(1, 1, 0, 0)


# ---- 2. entry counts around the adder batches -------------------------------------------------------------------------------------

@pytest.mark.parametrize("entries", [0, 1, 3, 4, 5, 15, 16, 17, 33])
def test_entry_counts_around_the_batches(entries):
    rng = np.random.default_rng(200 + entries)
    n, R = 70, 12
    rows = (rng.random((R, n)) < 0.4).astype(np.int8)
    sets = random_sets(rng, R, 20)
    signs = random_signs(rng, sets)
    which = rng.integers(0, 20, entries)
    ex = api.JoinExec(1, 30, n - 30, 0)
    try:
        before = ex.patient_launches
        for by_sign in (False, True):
            got = check(ex, sets, rows, which, None, None, by_sign, signs, f"{entries} entries by_sign {by_sign}")
            assert got[1].tolist() == [entries]
        assert ex.patient_launches - before == (2 if entries else 0)       # one kernel per call; none without entries
    finally:
        ex.close()


# ---- 3. plane overflow, segment size ------------------------------------------------------------------------------------------------

def test_plane_overflow(monkeypatch):
    """One all-ones row listed 2^kPatientPlanes + 17 times in one group: the planes must be flushed before they wrap -- inside
    a segment when the segment holds every entry, and at the segments' ends with the default size."""
    n, times = 70, (1 << PLANES) + 17
    rows = np.zeros((3, n), np.int8)
    rows[1] = 1
    rows[2, ::3] = 1
    sets = [[1], [2], [1, 2]]
    which = np.zeros(times + 5, np.int64)
    which[times:] = 1
    ex = api.JoinExec(1, 33, n - 33, 0)
    try:
        for seg in (None, str(times + 100), str((1 << PLANES) - 1), str(1 << PLANES)):
            if seg is None:
                monkeypatch.delenv("GCRE_PATIENT_SEG", raising=False)
            else:
                monkeypatch.setenv("GCRE_PATIENT_SEG", seg)
            counts, group_sets, skipped = ex.patient_counts(sets, rows, which)
            want = np.full(n, times, np.int32)
            want[::3] += 5
            np.testing.assert_array_equal(counts[0, 0], want, err_msg=f"GCRE_PATIENT_SEG {seg}")
            assert group_sets.tolist() == [times + 5] and skipped == 0
            # both planes overflow together
            both = ex.patient_counts(sets, rows, np.full(times, 2), by_sign=True, signs=[[1], [1], [1, -1]])[0]
            np.testing.assert_array_equal(both[0, 0], np.full(n, times))
            np.testing.assert_array_equal(both[0, 1], np.where(np.arange(n) % 3 == 0, times, 0))
    finally:
        ex.close()


def test_segment_size_changes_nothing(monkeypatch):
    rng = np.random.default_rng(31)
    n, R, S, E = 2085, 15, 60, 700
    rows = (rng.random((R, n)) < 0.3).astype(np.int8)
    sets = random_sets(rng, R, S, na=0.05)
    signs = random_signs(rng, sets)
    which, group = rng.integers(0, S, E), rng.integers(-1, 4, E)
    want = {b: report.patient_counts_reference(sets, rows, signs, which, group, 4, n, b) for b in (False, True)}
    ex = api.JoinExec(2, 1000, n - 1000, 0)
    try:
        for seg in ("1", "7", str(E + 50), None):
            if seg is None:
                monkeypatch.delenv("GCRE_PATIENT_SEG", raising=False)
            else:
                monkeypatch.setenv("GCRE_PATIENT_SEG", seg)
            for b in (False, True):
                same(ex.patient_counts(sets, rows, which, group, 4, b, signs), want[b], f"GCRE_PATIENT_SEG {seg} by_sign {b}")
    finally:
        ex.close()


# ---- 4. groups ------------------------------------------------------------------------------------------------------------------------

def test_groups():
    rng = np.random.default_rng(41)
    n, R, S = 77, 10, 30
    rows = (rng.random((R, n)) < 0.3).astype(np.int8)
    sets = random_sets(rng, R, S)
    ex = api.JoinExec(1, 40, n - 40, 0)
    try:
        # unsorted group ids, group 2 of 5 empty, uncounted entries in between
        which = rng.integers(0, S, 90)
        group = rng.choice([4, 0, 3, 1, -1], 90)
        got = check(ex, sets, rows, which, group, 5, what="unsorted")
        assert got[1][2] == 0 and not got[0][2].any() and got[1].sum() == (group >= 0).sum()
        # a group change inside a batch of 16: runs of 5, 16 + 3 and 1 entries
        group = np.array([0] * 5 + [1] * 19 + [2])
        check(ex, sets, rows, np.arange(25), group, 3, what="a change inside a batch")
        # sorted by group already, and the reverse
        which = rng.integers(0, S, 40)
        for group in (np.sort(rng.integers(0, 3, 40)), np.sort(rng.integers(0, 3, 40))[::-1].copy()):
            check(ex, sets, rows, which, group, 3, what="sorted")
        # group = None: everything in group 0; n_groups from the list
        got = check(ex, sets, rows, which, None, None, what="no groups")
        assert got[0].shape == (1, 1, n)
        assert check(ex, sets, rows, which, rng.integers(0, 4, 40), None)[0].shape[0] <= 4
        check(ex, sets, rows, what="every set once")
        # every entry -1: zeros, nothing launched
        before = ex.patient_launches
        got = ex.patient_counts(sets, rows, which, np.full(40, -1), 2)
        assert not got[0].any() and got[0].shape == (2, 1, n) and got[1].tolist() == [0, 0] and got[2] == 0
        # ... and every counted entry NA
        got = ex.patient_counts([[0, -1], [1]], rows, [0, 0, 1], [0, 0, -1])
        assert not got[0].any() and got[1].tolist() == [0] and got[2] == 2
        assert ex.patient_launches == before
    finally:
        ex.close()


# ---- 5. signs, methods, member width ---------------------------------------------------------------------------------------------------

def test_signs_and_the_method_change_nothing():
    rng = np.random.default_rng(51)
    n, R, S = 90, 12, 50
    rows = (rng.random((R, n)) < 0.3).astype(np.int8)
    sets = random_sets(rng, R, S, na=0.05)
    sets[0], sets[1] = [3, 3, 4], [5, 5]                   # a repeated member; one member under both signs
    signs = random_signs(rng, sets)
    signs[0], signs[1] = [1, 1, -1], [1, -1]
    which, group = rng.integers(0, S, 120), rng.integers(-1, 2, 120)
    got = {}
    for method in (1, 2):
        ex = api.JoinExec(method, 41, n - 41, 0)
        try:
            for by_sign in (False, True):
                for sg in (None, signs):
                    got[method, by_sign, sg is None] = check(ex, sets, rows, which, group, 2, by_sign, sg,
                                                            f"method {method} by_sign {by_sign} signs {sg is not None}")
        finally:
            ex.close()
    for key in [k for k in got if k[0] == 1]:
        same(got[(2,) + key[1:]], got[key], f"method 2 against method 1 {key[1:]}")
    # without by_sign the signs are not read; with it and no signs everything is in plane 0
    np.testing.assert_array_equal(got[1, False, False][0], got[1, False, True][0])
    np.testing.assert_array_equal(got[1, True, True][0][:, 0], got[1, False, True][0][:, 0])
    assert not got[1, True, True][0][:, 1].any() and got[1, True, False][0][:, 1].any()


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 6])
def test_member_width(M):
    rng = np.random.default_rng(60 + M)
    n, R, S = 100, 20, 80
    rows = (rng.random((R, n)) < 0.15).astype(np.int8)
    sets = random_sets(rng, R, S, max_members=M)            # ragged: 1 .. M members
    sets[7] = rng.integers(0, R, M).tolist()
    signs = random_signs(rng, sets)
    lens = np.array([len(s) for s in sets])
    ex = api.JoinExec(1, 50, 50, 0)
    try:
        for by_sign in (False, True):
            check(ex, sets, rows, None, None, None, by_sign, signs, f"M {M}")
            check(ex, sets, rows, None, lens - 1, M, by_sign, signs, f"M {M}, grouped by length")      # gwaspa's grouping
            off = np.cumsum(np.concatenate([[0], lens])).astype(np.int64)
            flat = (off, np.concatenate(sets).astype(np.int32))
            same(ex.patient_counts(flat, rows, None, lens - 1, M, by_sign, np.concatenate(signs)),
                 report.patient_counts_reference(sets, rows, signs, None, lens - 1, M, n, by_sign), "(off, members)")
    finally:
        ex.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(monkeypatch):
    n, nc = 45, 20
    rng = np.random.default_rng(3)
    rows = (rng.random((6, n)) < 0.3).astype(np.int8)
    packed = api.pack_carriers(rows, n)
    ex = api.JoinExec(2, nc, n - nc, 0)
    good = [[0], [2, 3], [4, -1], [5]]
    lib = api._patients_lib()
    monkeypatch.delenv("GCRE_PATIENT_MAX_MB", raising=False)

    def failed(res, code, text):
        msg = ex._lib.gcre_last_error(ex._h)
        assert res[0] == code and text in msg, (res[0], msg)
        assert ex.patient_launches == 0

    ARG, RANGE = api.GCRE_ERR_ARG, api.GCRE_ERR_RANGE
    W = b"set_patient_counts: "
    # what check_set_shape / check_set_members refuse
    failed(raw_patients(ex, good, packed, n + 1, [0], [0]), ARG, W + b"the rows have 46 columns")
    failed(raw_patients(ex, [[0], []], packed, n, [0], [0]), ARG, W + b"set 1 has no members")
    failed(raw_patients(ex, [[0], [6]], packed, n, [0], [0]), RANGE, W + b"set 1: member row 6 out of range")
    failed(raw_patients(ex, [[0], [1]], packed, n, [0], [0], signs=[[1], [0]]), ARG, W + b"set 1: sign 0 is neither +1 nor -1")
    failed((lib.gcre_set_patient_counts(ex._h, None, None, 0, None, 1, 0, None, None, None),), ARG, b"NULL argument")
    # its own
    for b in (-1, 2):
        failed(raw_patients(ex, good, packed, n, [0], [0], by_sign=b), ARG, W + b"by_sign must be 0 or 1")
    for g in (0, -3):
        failed(raw_patients(ex, good, packed, n, [0], [0], n_groups=g), ARG, W + b"n_groups must be at least 1")
    failed(raw_patients(ex, good, packed, n, [0], [0], n_which=-1), ARG, W + b"bad index list")
    failed(raw_patients(ex, good, packed, n, None, [0, 0, 0], n_which=3), ARG, W + b"bad index list")
    failed(raw_patients(ex, good, packed, n, [0, 1], None, n_groups=2), ARG, W + b"NULL `group` puts every entry in group 0")
    failed(raw_patients(ex, good, packed, n, [0], [0], want_counts=False), ARG, W + b"NULL counts")
    failed(raw_patients(ex, good, packed, n, [0], [0], n_which=2**31 - 17), ARG, W + b"2147483631 entries: a 32-bit count could overflow")
    failed(raw_patients(ex, good, packed, n, [0, 4], [0, 0]), RANGE, W + b"which[1] = 4 out of range (4 sets)")
    failed(raw_patients(ex, good, packed, n, [-1], [0]), RANGE, W + b"which[0] = -1 out of range")
    failed(raw_patients(ex, good, packed, n, [0, 1], [0, 2], n_groups=2), RANGE, W + b"group[1] = 2 out of range (2 groups")
    failed(raw_patients(ex, good, packed, n, [0, 1], [-2, 0], n_groups=2), RANGE, W + b"group[0] = -2 out of range")
    monkeypatch.setenv("GCRE_PATIENT_MAX_MB", "0.001")           # 1048 bytes: 5 groups x 45 patients x 4 bytes = 900 fit
    failed(raw_patients(ex, good, packed, n, [0, 1], [0, 5], n_groups=6), ARG,
           W + b"6 groups x 1 planes x 45 patients x 4 bytes exceed GCRE_PATIENT_MAX_MB")
    failed(raw_patients(ex, good, packed, n, [0, 1], [0, 2], n_groups=3, by_sign=1), ARG,
           W + b"3 groups x 2 planes x 45 patients x 4 bytes exceed GCRE_PATIENT_MAX_MB")
    # a refused call leaves the outputs alone
    res = raw_patients(ex, good, packed, n, [0, 4], [0, 0])
    assert (res[1] == -7).all() and (res[2] == -7).all() and res[3] == -7
    rc, counts, group_sets, skipped = raw_patients(ex, good, packed, n, [0, 1, 2, 3], [0, 4, 4, -1], n_groups=5)
    assert rc == api.GCRE_OK and ex.patient_launches == 1
    same((counts, group_sets, skipped), report.patient_counts_reference(good, rows, None, [0, 1, 2, 3], [0, 4, 4, -1], 5, n, False))
    monkeypatch.delenv("GCRE_PATIENT_MAX_MB")
    # the Python method: its own ValueErrors, and the library's message
    with pytest.raises(ValueError, match="which: a set index outside"):
        ex.patient_counts(good, rows, [4])
    with pytest.raises(api.GcreError, match="the rows have 44 columns"):
        ex.patient_counts(good, rows[:, :44])
    assert ex.patient_launches == 1
    # the context still works
    check(ex, good, rows, [3, 0, 1, 1], [1, 0, 1, 1], 2, True, [[1], [-1, 1], [1, 1], [-1]])
    size, _ = ex.set_overlap(good, rows)
    np.testing.assert_array_equal(size, report.overlap_reference(good, rows, nc, n - nc)[0])
    ex.close()


# ---- 7. the front end -----------------------------------------------------------------------------------------------------------------

def _network_case(seed, nc=48, nt=52):      # the small problem of test_gpu_hits.py
    rng = np.random.default_rng(seed)
    g, src, trg, sign = synth.signed_network(30, 70, rng)
    uid = np.arange(g) * 5 + 100
    symbols = [f"G{u}" for u in uid]
    data = (rng.random((g, nc + nt)) < 0.06).astype(np.int32)
    return symbols, data, (uid, symbols, uid[src], uid[trg], sign)


@pytest.mark.parametrize("signed", [False, True])
def test_gwaspa_patient_table(signed):
    import pandas as pd
    nc, nt, L = 48, 52, 5
    genes, data, network = _network_case(17)
    strata = (np.arange(nc + nt) * 5 % 3).astype(np.int32)
    kw = dict(signed=signed, threshold=0.2, n_permutations=1000, strata=strata, seed=909, path_length=L)
    # the problem has no planted signal: the level is the largest p-value below 1 that any path has
    full = report.gwaspa(genes, data, nc, nt, network, top_k=2000, **kw)["GWASPA.Results"]
    pv = full["Pvalues"].to_numpy(np.float64)[np.isfinite(full["Scores"].to_numpy(np.float64))]
    alpha = float(pv[pv < 1].max())
    kw.update(top_k=3, significant=alpha)
    base = report.gwaspa(genes, data, nc, nt, network, **kw)
    got = report.gwaspa(genes, data, nc, nt, network, patient_table=True, **kw)
    sig = got["Significant.Results"]
    assert len(sig) > 3 and len(set(sig["Lengths"])) > 1
    # the oracle: the printed paths, looked up in the dataset as gwaspa filtered it
    pgenes, pdata = report.preprocess_table(genes, data, 0.2, nc, nt)
    _, sets, _ = report.parse_sets([str(p) for p in sig["SignedPaths"]], pgenes)
    assert all(x >= 0 for s in sets for x in s)
    lengths = sig["Lengths"].to_numpy(np.int64)
    want = report.patient_counts_reference(sets, pdata, None, None, lengths - 1, L, nc + nt, False)
    names = [f"Hits.L{k}" for k in range(1, L + 1)]
    table = got["Patient.Results"]
    assert list(table.columns) == ["Patient", "Label"] + names + ["Hits", "HitShare"] and len(table) == nc + nt
    pd.testing.assert_frame_equal(table, report.patient_table(want[0], nc, columns=names, group_sets=want[1]), check_exact=True)
    same(got["patient_counts"], want, "gwaspa")
    C, _ = report.carrier_rows(sets, pdata, nc + nt)
    assert table["Hits"].sum() == C.sum() > 0 and want[1].sum() == len(sig)
    if not signed:       # the unsigned method's own counts are carriers of the path
        assert table["Hits"].sum() == sig["Cases"].sum() + sig["Controls"].sum()
        assert table["Hits"][:nc].sum() == sig["Cases"].sum()
    print(f"Patient.Results at {alpha}: {len(sig)} hits, most on one patient {table['Hits'].max()}")
    # every other key is what it is without
    assert set(got) == set(base) | {"Patient.Results", "patient_counts"}
    for key in base:
        if isinstance(base[key], pd.DataFrame):
            pd.testing.assert_frame_equal(got[key], base[key], check_exact=True)
    for k in base["significant"]:
        for f in ("score", "ordinal", "src", "trg", "cases", "ctrls"):
            assert getattr(got["significant"][k], f).tobytes() == getattr(base["significant"][k], f).tobytes(), (k, f)
        for f in ("scores", "src", "trg", "cases", "ctrls", "null"):
            assert getattr(got["levels"][f"lst{k}"], f).tobytes() == getattr(base["levels"][f"lst{k}"], f).tobytes(), (k, f)
    assert got["significant_cutoffs"] == base["significant_cutoffs"]
    # with the clumps: the leads once more, in a group of their own
    cl = report.gwaspa(genes, data, nc, nt, network, patient_table=True, clump=0.5, clump_significant=True, **kw)
    csig = cl["Significant.Results"]
    pd.testing.assert_frame_equal(csig[report.COLUMNS], sig[report.COLUMNS], check_exact=True)
    leads = np.flatnonzero((csig["Clump"].to_numpy() >= 0) & np.isnan(csig["LeadOverlap"].to_numpy()))      # a lead has no overlap value
    assert 0 < len(leads) < len(csig) and len(leads) == csig["Clump"].max() + 1
    ctable = cl["Patient.Results"]
    assert list(ctable.columns) == ["Patient", "Label"] + names + ["Leads", "Hits", "HitShare"]
    lead_counts = report.patient_counts_reference(sets, pdata, None, leads, None, 1, nc + nt, False)[0]
    np.testing.assert_array_equal(ctable["Leads"].to_numpy(), lead_counts[0, 0])
    pd.testing.assert_frame_equal(ctable.drop(columns="Leads"), table, check_exact=True)
    assert cl["patient_counts"][1].tolist() == want[1].tolist() + [len(leads)]


def test_gwaspa_patient_table_needs_significant():
    genes, data, network = _network_case(17)
    with pytest.raises(ValueError, match="patient_table: needs significant"):
        report.gwaspa(genes, data, 48, 52, network, patient_table=True)


# ---- 8. seeded loop -----------------------------------------------------------------------------------------------------------------
N_FUZZ = int(os.environ.get("GCRE_PATIENT_FUZZ_CASES", "6"))
FUZZ_BASE = int(os.environ.get("GCRE_PATIENT_FUZZ_BASE", "0"))


def test_seeded_loop(monkeypatch):
    lines = []
    for k in range(FUZZ_BASE, FUZZ_BASE + N_FUZZ):
        rng = np.random.default_rng(8_000_000 + k)
        n = int(rng.choice([int(rng.integers(2, 70)), int(rng.integers(70, 2049)), int(rng.integers(2049, 4300))]))
        nc = int(rng.integers(1, n))
        R, S = int(rng.integers(1, 50)), int(rng.integers(1, 300))
        rows = (rng.random((R, n)) < rng.choice([0.02, 0.08, 0.3, 0.9])).astype(np.int8)
        sets = random_sets(rng, R, S, max_members=int(rng.integers(1, 8)), na=float(rng.choice([0.0, 0.05, 0.5])))
        signs = random_signs(rng, sets) if rng.random() < 0.7 else None
        E = int(rng.choice([0, int(rng.integers(1, 40)), int(rng.integers(40, 1500))]))
        which = rng.integers(0, S, E) if rng.random() < 0.8 else None
        entries = S if which is None else E
        G = int(rng.integers(1, 7))
        group = rng.integers(-1, G, entries) if rng.random() < 0.8 else None
        G = G if group is not None else 1
        by_sign = bool(rng.integers(0, 2))
        seg = rng.choice(["", "1", "3", "16", "17", "100"])
        if seg:
            monkeypatch.setenv("GCRE_PATIENT_SEG", str(seg))
        else:
            monkeypatch.delenv("GCRE_PATIENT_SEG", raising=False)
        ex = api.JoinExec(1 + k % 2, nc, n - nc, 0)
        try:
            got = check(ex, sets, rows, which, group, G, by_sign, signs, f"case {k}")
        finally:
            ex.close()
        lines.append(f"case {k}: patients {n} rows {R} sets {S} entries {entries} groups {G} by_sign {int(by_sign)} "
                     f"signs {int(signs is not None)} seg {seg or 'default'} counted {int(got[1].sum())} skipped {got[2]} "
                     f"most {int(got[0].max())} ok")
    out = os.environ.get("GCRE_PATIENT_FUZZ_OUT")
    if out:
        with open(out, "w") as f:
            f.write(f"test_gpu_patients.py::test_seeded_loop: cases {FUZZ_BASE}..{FUZZ_BASE + N_FUZZ - 1}, every one exact\n")
            f.write("\n".join(lines) + "\n")
