"""The method-1 inspector's counts from row totals (k_stats_ie2<NL, true>, k_row_counts): a joined path's carriers, its
carriers among the cases and its delta are sums of per-row totals minus what the few non-zero words of x & z hold.  Through
the test-only export gcre_test_inspect, against a numpy restatement (np.unpackbits popcounts) and against the inspector that
counts every word (GCRE_STATS_IE_COUNTS=0), word for word; lists are compared as the sets of entries they hold."""
import os

import numpy as np
import pytest

from geneticscre_amd import api
from geneticscre_amd.synth import make_problem
from helpers import small_table

pytestmark = pytest.mark.gpu

# patients -> Wp = 4, 36, 80, 112, 160 words: 1 to 5 blocks of 32 words per row, the last one partly outside the row but at 160
PATIENTS = {4: 250, 36: 2200, 80: 5000, 112: 7100, 160: 10200}
OVERLAPS = (0, 1, 7, 8, 9, 16, 17, 40)
TABLE_SIDE = 200        # cells beyond the table read as -1 (the reference's padding)


def combos():
    """(overlap, delta): the mode rule's edges (overlap <= 8, overlap < delta), z inside x, empty z."""
    out = []
    for ov in OVERLAPS:
        for dl in (0, ov - 1, ov, ov + 1, 100):
            if dl >= 0 and (ov, dl) not in out:
                out.append((ov, dl))
    return out


def rows_of(bit_lists, words):
    r = np.zeros((len(bit_lists), words), np.uint64)
    for i, bits in enumerate(bit_lists):
        for b in bits:
            r[i, b // 64] |= np.uint64(1) << np.uint64(b % 64)
    return r


def popc(rows):
    return np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=-1).sum(axis=-1).astype(np.int64)


def bits_of(row):
    """Set bits of one row, as patient numbers."""
    return np.flatnonzero(np.unpackbits(row.view(np.uint8), bitorder="little"))


class Cohort:
    """A context per knob setting at one row width, x rows, and z rows constructed per (x row, overlap, delta)."""

    def __init__(self, wp):
        self.wp, self.n = wp, PATIENTS[wp]
        n = self.n
        self.n_cases = n // 2
        rng = np.random.default_rng(wp)
        self.table = small_table(TABLE_SIDE - 1, TABLE_SIDE - 1, wp)
        self.ex = {}
        for knob in (1, 0):
            os.environ["GCRE_STATS_IE_COUNTS"] = str(knob)
            try:
                e = api.JoinExec("method1", self.n_cases, n - self.n_cases, 0)
            finally:
                del os.environ["GCRE_STATS_IE_COUNTS"]
            assert (e.vlen + 3) // 4 * 4 == wp          # rows of vlen words on the host, padded to a multiple of 4 on the device
            e.set_value_table(self.table)
            self.ex[knob] = e
        words = self.ex[1].vlen
        self.cm = rows_of([range(self.n_cases)], words)[0]
        # x rows: empty; 60 carriers with bit 63 of word 1 and the last patient; three random ones of 45 to 90
        xs = [[], sorted({127, n - 1} | set(rng.choice(n, 58, replace=False).tolist()))]
        xs += [sorted(rng.choice(n, int(k), replace=False).tolist()) for k in (45, 70, 90)]
        zs, pairs = [], []          # pairs: (x row, z row, overlap, delta) in uid order
        for xi, xb in enumerate(xs):
            inside = np.array(xb, np.int64)
            outside = np.setdiff1d(np.arange(n), inside)
            for ov, dl in combos():
                if ov > len(inside):
                    continue
                z = list(rng.choice(inside, ov, replace=False)) + list(rng.choice(outside, dl, replace=False))
                pairs.append((xi, len(zs), ov, dl))
                zs.append(z)
        # a word whose only overlap bit is bit 63; an overlap in the row's last word; both and something new
        for z in ([127], [n - 1], [127, n - 1, int(np.setdiff1d(np.arange(n), xs[1])[0])]):
            pairs.append((1, len(zs), len(set(z) & set(xs[1])), len(set(z) - set(xs[1]))))
            zs.append(z)
        self.x, self.z, self.pairs = rows_of(xs, words), rows_of(zs, words), pairs
        ovw = self.x[[p[0] for p in pairs]] & self.z[[p[1] for p in pairs]]
        assert (popc(ovw & self.cm) > 0).any() and (popc(ovw & ~self.cm) > 0).any()    # overlaps on both sides of the case mask
        assert (ovw == np.uint64(1) << np.uint64(63)).any()
        self.sets = {k: (e.from_words(self.x), None) for k, e in self.ex.items()}

    def close(self):
        for e in self.ex.values():
            e.close()

    # ---- orders of the same paths: uids of ~40 paths, of one path, of 1 to 7 paths ----
    def order(self, kind, count):
        rng = np.random.default_rng(count)
        p = np.array([(a, b) for a, b, _, _ in self.pairs], np.int64)
        if kind == "one":                 # every path another x row than the one before
            by = [p[p[:, 0] == xi] for xi in range(len(self.x))]
            out, i = [], 0
            while len(out) < len(p):
                q = by[i % len(by)]
                if len(q) > i // len(by):
                    out.append(q[i // len(by)])
                i += 1
            p = np.array(out)
        elif kind == "ragged":            # cut the uids into runs of 1 to 7 and shuffle the runs
            cuts, at = [], 0
            while at < len(p):
                k = int(rng.integers(1, 8))
                cuts.append(p[at:at + k])
                at += k
            p = np.concatenate([cuts[i] for i in rng.permutation(len(cuts))])
        reps = -(-count // len(p))
        p = np.concatenate([p] * reps)[:count]
        return p[:, 0].astype(np.uint32), p[:, 1].astype(np.uint32)


def want(x, z, cm, table, row0, rz):
    """The inspector's outputs restated: counts, list mode and length, the list as a set, the score's key."""
    X, Z = x[row0], z[rz]
    j = X | Z
    tot, cases = popc(j), popc(j & cm)
    ov, dl = popc(X & Z), popc(Z & ~X)
    mode = ((ov <= 8) | (ov < dl)).astype(np.int64)
    ln = np.where(mode == 1, ov, dl)
    len8 = np.maximum(8, (ln + 7) & ~7)
    linfo = len8 | mode | ((len8 - ln) << 28)
    ctrls = tot - cases
    inside = (cases < table.shape[0]) & (ctrls < table.shape[1])
    score = np.where(inside, table[np.minimum(cases, table.shape[0] - 1), np.minimum(ctrls, table.shape[1] - 1)], -1.0)
    b = score.view(np.uint64)
    key = np.where(b >> np.uint64(63), ~b, b | (np.uint64(1) << np.uint64(63)))
    lists = [np.sort(bits_of((X[i] & Z[i]) if mode[i] else (Z[i] & ~X[i])).astype(np.uint32) << 8) for i in range(len(row0))]
    return dict(tot=tot, cases=cases, ctrls=ctrls, rowz=np.asarray(rz, np.int64), linfo=linfo, key=key, lists=lists, rows=j,
                max_tot=int(tot.max()), modes=int(mode.sum()), max_len=int(len8.max()), over=int((len8 - 8).sum()))


def check(got, w, wp, keep_rows=False):
    for k in ("tot", "cases", "ctrls", "rowz", "linfo", "key"):
        np.testing.assert_array_equal(got[k].astype(np.uint64), w[k].astype(np.uint64), err_msg=k)
    for i, (g, pad) in enumerate(zip(got["lists"], got["padding"])):
        np.testing.assert_array_equal(np.sort(g), w["lists"][i], err_msg=f"list {i}")
        assert (pad == (64 * wp) << 8).all(), f"padding of list {i}"
    f = got["flags"]
    assert int(f[0]) == w["max_tot"] and int(f[2]) == w["modes"]
    assert int(f[5]) == (w["max_len"] if w["max_len"] > 8 else 0)
    if keep_rows:
        np.testing.assert_array_equal(got["rows"], w["rows"])


def same(a, b):
    """Two roads, word for word; list offsets into the overflow area are not part of the outputs."""
    for k in ("tot", "cases", "ctrls", "rowz", "linfo", "key"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for i in range(len(a["lists"])):
        np.testing.assert_array_equal(np.sort(a["lists"][i]), np.sort(b["lists"][i]), err_msg=f"list {i}")
    np.testing.assert_array_equal(a["flags"][[0, 1, 2, 5]], b["flags"][[0, 1, 2, 5]])


@pytest.fixture(scope="module", autouse=True)
def _trace():
    os.environ["GCRE_LAUNCH_TRACE"] = "1"
    yield
    del os.environ["GCRE_LAUNCH_TRACE"]


@pytest.fixture(scope="module", params=sorted(PATIENTS))
def cohort(request, _trace):
    c = Cohort(request.param)
    yield c
    c.close()


def run_both(c, row0, row1, capfd, expect_counts=True, **kw):
    """The used z rows as the reduced set (no more rows than paths), both roads; returns (new road, old road, z rows used)."""
    used, rz = np.unique(row1, return_inverse=True)
    zr = c.z[used]
    out = {}
    for knob, e in c.ex.items():
        red = e.from_words(zr)
        capfd.readouterr()
        out[knob] = e.test_inspect(c.sets[knob][0], red, row0, rz, ent_stride=112, over_entries=104 * len(row0), **kw)
        err = capfd.readouterr().err
        assert ("launch k_row_counts" in err) == (knob == 1 and expect_counts), err
        assert "launch k_stats_ie2 " in err
        red.free()
    return out[1], out[0], zr, rz


@pytest.mark.parametrize("kind", ["uids", "one", "ragged"])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 3001])
def test_counts_and_lists(cohort, count, kind, capfd):
    c = cohort
    row0, row1 = c.order(kind, count)
    if kind == "uids" and count >= 65:
        assert (row0[63] == row0[64])                        # a uid that spans two 64-path blocks
    new, old, zr, rz = run_both(c, row0, row1, capfd, keep_rows=(count == 65))
    w = want(c.x, zr, c.cm, c.table, row0, rz)
    if count == 3001:
        assert w["max_len"] > 8 and (w["linfo"] & 1 == 0).any() and (w["tot"] == 0).any()   # overflow lists, delta lists, empty joins
    check(new, w, c.wp, keep_rows=(count == 65))
    check(old, w, c.wp, keep_rows=(count == 65))
    same(new, old)


def hinted(c, count):
    """A hinted join over the cohort's paths: paths1 row l stands for reduced row zindex[l]; every uid (run of one x row) has a
    range whose excess lies inside its x row."""
    row0, row1 = c.order("uids", count)
    zindex = np.arange(len(c.z), dtype=np.int32)[::-1].copy()       # paths1 row l <-> reduced row n - 1 - l
    p1 = (len(c.z) - 1 - row1.astype(np.int64)).astype(np.uint32)
    range_of = np.arange(len(c.x), dtype=np.int32)
    excess = c.x.copy()
    excess[:, ::2] = 0                                               # some of the x row's own bits: inside it
    return row0, p1, zindex, range_of, excess


@pytest.mark.parametrize("stray", [False, True])
def test_hint_is_checked(cohort, stray, capfd):
    """The excess of a uid's range must lie inside its paths0 row: one stray bit in one range raises the flag on both roads."""
    c = cohort
    row0, p1, zindex, range_of, excess = hinted(c, 700)
    if stray:
        free = np.setdiff1d(np.arange(c.n), bits_of(c.x[2]))
        excess[2, free[-1] // 64] |= np.uint64(1) << np.uint64(free[-1] % 64)
    out = {}
    for knob, e in c.ex.items():
        red = e.from_words(c.z)
        capfd.readouterr()
        out[knob] = e.test_inspect(c.sets[knob][0], red, row0, p1, zindex=zindex, excess=excess, range_of=range_of,
                                   ent_stride=112, over_entries=104 * len(row0))
        assert ("launch k_row_counts" in capfd.readouterr().err) == (knob == 1)
        assert int(out[knob]["flags"][1]) == int(stray), f"knob {knob}"
        red.free()
    rz = zindex[p1].astype(np.int64)
    w = want(c.x, c.z, c.cm, c.table, row0, rz)
    check(out[1], w, c.wp)
    same(out[1], out[0])


def test_more_reduced_rows_than_paths_takes_the_old_road(cohort, capfd):
    c = cohort
    row0, row1 = c.order("ragged", 100)
    assert len(c.z) > 100
    for knob, e in c.ex.items():
        red = e.from_words(c.z)
        capfd.readouterr()
        got = e.test_inspect(c.sets[knob][0], red, row0, row1, ent_stride=112, over_entries=104 * len(row0))
        err = capfd.readouterr().err
        assert "launch k_row_counts" not in err and "launch k_stats_ie2 " in err
        check(got, want(c.x, c.z, c.cm, c.table, row0, row1.astype(np.int64)), c.wp)
        red.free()


def test_totals_are_rebuilt_when_the_rows_are_rewritten(capfd):
    """A kept set as the reduced operand: inspected, rewritten by a join that keeps other rows in it, inspected again."""
    p = make_problem(40, 110, 31, 33, 100, 3, method="method1", top_k=15, seed=5, threshold=0.2)
    plan = api.ResidentPlan(p)
    try:
        e = plan.ex
        a, b, res = plan.operands("1a")
        du = api.DeviceUids(e, p.levels.uids["1a"])
        x = b.to_numpy()
        cm = rows_of([range(p.n_cases)], e.vlen)[0]
        n = res.size
        row0 = (np.arange(2 * n) % b.size).astype(np.uint32)
        row1 = (np.arange(2 * n) % n).astype(np.uint32)
        seen = []
        for paths1 in (b, e.from_words(np.roll(x, 1, axis=0) | np.roll(x, 2, axis=0))):
            e.join(du, a, paths1, res)
            z = res.to_numpy()
            seen.append(z)
            capfd.readouterr()
            got = e.test_inspect(b, res, row0, row1, ent_stride=72, over_entries=64 * len(row0))
            assert "launch k_row_counts" in capfd.readouterr().err
            w = want(x, z, cm, np.asarray(p.value_table, np.float64), row0, row1.astype(np.int64))
            for k in ("tot", "cases", "ctrls", "linfo"):
                np.testing.assert_array_equal(got[k].astype(np.int64), w[k], err_msg=k)
        assert (popc(seen[0]) != popc(seen[1])).any()
    finally:
        plan.close()
