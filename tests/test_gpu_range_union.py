"""The range check of a hinted join (k_range_union): per distinct uid range, what the paths1 rows have beyond their reduced
rows, and whether every reduced row lies inside the row it stands for.  Word for word against a numpy restatement through
the test-only export gcre_test_range_union, which hands the kernel a table full of 0xa5 bytes (it must write every word of
every range itself), and through joins against the oracle."""
import numpy as np
import pytest

import oracle
from geneticscre_amd import api
from geneticscre_amd.synth import make_problem
from helpers import assert_same_result

pytestmark = pytest.mark.gpu

SWAP = 1 << 31


@pytest.fixture(scope="module")
def ex():
    e = api.JoinExec("method1", 30, 34, 0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def piece(ex):
    """Rows above which a range is walked in pieces: read through the export, not copied."""
    z = np.zeros((1, 4), np.uint64)
    _, _, rows = ex.test_range_union(z, z, [0], [0], [1], 4, 1)
    assert rows >= 2
    return rows


def sparse_rows(rng, n, S, bits):
    """n rows of S words with about `bits` bits each, some in word 0 and in the last word of most rows."""
    rows = np.zeros((n, S), np.uint64)
    for _ in range(bits):
        w = rng.integers(0, S, n)
        rows[np.arange(n), w] |= np.uint64(1) << rng.integers(0, 64, n).astype(np.uint64)
    return rows


def oriented(pz, zindex, wp, method):
    """z'(loc): the reduced row of each paths1 row, halves swapped where bit 31 of the index says so (method 2)."""
    zi = np.asarray(zindex, np.int64)
    z = pz[zi & 0x7fffffff]
    if method == 2:
        sw = (zi & SWAP) != 0
        z = np.where(sw[:, None], np.concatenate([z[:, wp:], z[:, :wp]], axis=1), z)
    return z


def union_numpy(p1, pz, zindex, loc, cnt, wp, method):
    z = oriented(pz, zindex, wp, method)
    U = np.zeros((len(loc), p1.shape[1]), np.uint64)
    bad = 0
    for r, (l, c) in enumerate(zip(loc, cnt)):
        y, zz = p1[l:l + c], z[l:l + c]
        U[r] = np.bitwise_or.reduce(y & ~zz, axis=0)
        bad |= int((zz & ~y).any())
    return U, bad


class Case:
    """paths1 rows that hold their reduced rows plus some excess; rows that no range covers (uids without paths in front of,
    between and behind the ranges) hold nothing of theirs, so that reading one would raise the flag."""

    def __init__(self, seed, wp, method, ranges, gaps=(3, 2, 5)):
        rng = np.random.default_rng(seed)
        self.wp, self.method, S = wp, method, method * wp
        self.loc, self.cnt = [], []
        at = gaps[0]
        for i, c in enumerate(ranges):
            if c < 0:                       # a second count at the location of the range before
                self.loc.append(self.loc[-1])
                self.cnt.append(-c)
                at = max(at, self.loc[-1] - c)
                continue
            at += gaps[1] if i else 0
            self.loc.append(at)
            self.cnt.append(c)
            at += c
        n1 = at + gaps[2]
        nz = 40
        self.pz = sparse_rows(rng, nz, S, 6)
        self.zindex = rng.integers(0, nz, n1).astype(np.int64)
        if method == 2:
            self.zindex |= rng.integers(0, 2, n1).astype(np.int64) << 31
        z = oriented(self.pz, self.zindex, wp, method)
        self.p1 = z | sparse_rows(rng, n1, S, 3)
        covered = np.zeros(n1, bool)
        for l, c in zip(self.loc, self.cnt):
            covered[l:l + c] = True
        self.p1[~covered] = 0
        assert (z[~covered] != 0).any() or covered.all()
        self.zindex = (self.zindex & 0xffffffff).astype(np.uint32).view(np.int32)

    def run(self, ex):
        return ex.test_range_union(self.p1, self.pz, self.zindex, self.loc, self.cnt, self.wp, self.method)

    def want(self):
        return union_numpy(self.p1, self.pz, self.zindex.view(np.uint32), self.loc, self.cnt, self.wp, self.method)


def shapes(piece):
    # one row; exactly a piece, one more, three pieces; two counts at one location (-n: at the location before)
    return [1, piece, piece + 1, 2 * piece + 3, 5, -3, 2, -(piece + 2), 7]


# 300 patients: 5 words, padded to 8; 4,097 patients: 65 words, padded to 68 -- three 32-word columns, the last of 4 words
@pytest.mark.parametrize("wp", [8, 68])
@pytest.mark.parametrize("method", [1, 2])
def test_union_matches_numpy(ex, piece, wp, method):
    c = Case(wp + method, wp, method, shapes(piece))
    U, bad, _ = c.run(ex)
    wU, wbad = c.want()
    assert wbad == 0 and bad == 0
    np.testing.assert_array_equal(U, wU)
    assert U.any(axis=1).all()


@pytest.mark.parametrize("method", [1, 2])
def test_more_ranges_than_the_grid(ex, piece, method):
    """9,000 ranges of one to three rows and a few cut ones: more (piece, column) pairs than the launch has waves."""
    rng = np.random.default_rng(2)
    ranges = [int(x) for x in rng.integers(1, 4, 9000)]
    ranges[100] = ranges[5000] = ranges[8999] = 3 * piece + 1
    c = Case(7, 8, method, ranges, gaps=(1, 1, 1))
    U, bad, _ = c.run(ex)
    wU, wbad = c.want()
    assert bad == wbad == 0
    np.testing.assert_array_equal(U, wU)


def planted_rows(piece):
    """(name, row of the range of 2 * piece + 3 rows)"""
    return [("first row of the first piece", 0), ("last row of the first piece", piece - 1),
            ("first row of the second piece", piece), ("last row of the range", 2 * piece + 2)]


@pytest.mark.parametrize("wp", [8, 68])
@pytest.mark.parametrize("method", [1, 2])
def test_planted_faults_and_planted_excess(ex, piece, wp, method):
    """One bit of a reduced row that its paths1 row lacks, in word 0 and in the last word, at the ends of the pieces: the
    flag comes back set each time.  The same bit planted in the paths1 row too: accepted, and U has the bit wherever the
    reduced row does not."""
    base = Case(40 + wp + method, wp, method, shapes(piece))
    S = method * wp
    r = base.cnt.index(2 * piece + 3)
    z = oriented(base.pz, base.zindex.view(np.uint32), wp, method)
    for name, row in planted_rows(piece):
        loc = base.loc[r] + row
        for word in (0, S - 1):
            free = ~(base.p1[loc, word] | z[loc, word])
            assert free, "a row with no free bit in this word"
            bit = free & (~free + np.uint64(1))          # lowest bit neither row has
            # the fault: a reduced row of its own for this paths1 row, with the bit
            c = Case.__new__(Case)
            c.__dict__.update(base.__dict__)
            zi = base.zindex.view(np.uint32).astype(np.int64)
            swapped = method == 2 and bool(zi[loc] & SWAP)
            zword = (word + wp) % S if swapped else word
            c.pz = np.concatenate([base.pz, base.pz[zi[loc] & 0x7fffffff][None]])
            c.pz[-1, zword] |= bit
            zi2 = zi.copy()
            zi2[loc] = (len(c.pz) - 1) | (zi[loc] & SWAP)
            c.zindex = zi2.astype(np.uint32).view(np.int32)
            U, bad, _ = c.run(ex)
            assert c.want()[1] == 1
            assert bad == 1, f"{name}, word {word}: a reduced row outside its row went unnoticed"
            # the excess: the same bit in the paths1 row alone
            c = Case.__new__(Case)
            c.__dict__.update(base.__dict__)
            c.p1 = base.p1.copy()
            c.p1[loc, word] |= bit
            U, bad, _ = c.run(ex)
            wU, wbad = c.want()
            assert bad == wbad == 0
            np.testing.assert_array_equal(U, wU)
            assert U[r, word] & bit, f"{name}, word {word}: planted excess missing"


def hinted_level4(method, seed=7):
    """The level-4 join of a rare-variant problem with its real hint (test_gpu_ie.py: test_wrong_hint_is_detected_and_ignored)."""
    p = make_problem(70, 260, 310, 335, 200, 4, method=method, top_k=15, seed=seed, threshold=0.05)
    full = oracle.process_paths(p, order="canonical")
    real = np.asarray(p.levels.data_inds["3"], np.int64)
    if method == "method2":
        real = real | ((np.asarray(p.levels.uids["2"].signs) != 1).astype(np.int64) << 31)
    return p, full, real


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_planted_fault_through_a_join(method, monkeypatch):
    """The real hint is accepted; with one reduced row that is not inside its paths1 row -- at the first and at the last row
    of the longest uid range -- the hint is rejected (ie_hinted_joins 0) and the results are the oracle's all the same."""
    monkeypatch.setenv("GCRE_NULL_KERNEL", "ie")
    p, full, real = hinted_level4(method)
    u = p.levels.uids["4"]
    count, location = np.asarray(u.count), np.asarray(u.location)
    big = int(np.argmax(count))
    paths2 = np.asarray(full["paths2"]).view(np.uint64)
    wp = paths2.shape[1] // (2 if method == "method2" else 1)
    data = np.asarray(p.data1)
    e = api.JoinExec(method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        e.top_k = p.top_k
        e.set_value_table(p.value_table)
        e.set_permuted_cases(p.perm_cases)
        p3, p2 = e.from_words(full["paths3"]), e.from_words(full["paths2"])
        genes = e.load(p.data1)
        du = api.DeviceUids(e, u)
        du.set_reduced(genes, real)
        assert_same_result(e.join(du, p3, p2), full["lst4"])
        assert e.profile()["ie_hinted_joins"] == 1
        for loc in (int(location[big]), int(location[big] + count[big] - 1)):
            row = paths2[loc, :wp] | (paths2[loc, wp:2 * wp] if method == "method2" else np.uint64(0))
            has = ((row[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)[:data.shape[1]]
            outside = [g for g in range(data.shape[0]) if (data[g] != 0)[~has].any()]
            assert outside
            wrong = real.copy()
            wrong[loc] = outside[0]
            du.set_reduced(genes, wrong)
            assert_same_result(e.join(du, p3, p2), full["lst4"])
            assert e.profile()["ie_hinted_joins"] == 0
    finally:
        e.close()
