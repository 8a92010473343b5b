"""The radix select's pass structure (gcre_kernels.hip, launch_radix_select): two digit passes over all keys, one compaction
of the keys that share the 16 bits chosen by then into a candidate buffer, six digit passes over the candidates -- or, when
more keys share those bits than the buffer holds, over all keys as before.  Tested through joins, against the CPU oracle,
bit for bit: with the default buffer, with a buffer of 64 keys (GCRE_SELECT_CAND=64: the fallback, wherever more than 64
keys share the threshold's top 16 bits) and with the old sequence of eight passes over all keys (GCRE_SELECT_PASSES=8);
the three runs of a case must also give identical bytes.

The network is that of test_gpu_warm_sizes.py (level 4: 5,535 joined paths, 729 distinct (cases, controls) pairs, so that a
method-1 score is one cell of the value table and a table can be written for the case it is to provoke).  The cases: an
ordinary table; a constant one (every key ties); zeros of both signs around a handful of positive cells (the cut falls on
a zero); -inf in nearly every cell level 4 reads (fewer scorable paths than top_k: the threshold key is 0); top_k = 1 and
top_k = every path; and a join of two paths whose keys differ in their lowest byte only (the last digit pass decides).
test_oracle_puts_each_input_in_its_case asserts on the oracle's results alone that each input is what it is called."""
import numpy as np
import pytest

import oracle
from geneticscre_amd import api
from geneticscre_amd.synth import make_problem
from geneticscre_amd.uids import UidRelSet
from helpers import assert_same_result, small_table

NC, NT = 300, 330
TOP_K = 12
FORCED = 64                # GCRE_SELECT_CAND of the forced fallback
DEFAULT_CAND = 32768       # gcre_ctx::sel_cand
LEVELS4 = (("1b", "lst1"), ("2", "lst2"), ("3", "lst3"), ("4", "lst4"))
SETTINGS = ({}, {"GCRE_SELECT_CAND": str(FORCED)}, {"GCRE_SELECT_PASSES": "8"})
CASES = ("ordinary", "constant", "zeros", "unscorable", "top1", "top_all")
_CACHE: dict = {}


def problem(table, top_k=TOP_K):
    return make_problem(120, 420, NC, NT, 40, 4, method="method1", top_k=top_k, seed=3, table=table)


def keys_of(scores):
    """score_key (gcre_kernels.hip): the order-preserving image of a double's bits; 0 for a score that is not above -inf."""
    s = np.asarray(scores, np.float64)
    b = s.view(np.uint64)
    k = np.where((b >> np.uint64(63)) != 0, ~b, b | np.uint64(1 << 63))
    return np.where(s > -np.inf, k, np.uint64(0))


def level4_pairs():
    """(cases, controls) of every level-4 path -- they do not depend on the table -- and the five rarest pairs."""
    if "pairs" not in _CACHE:
        r = oracle.process_paths(problem(small_table(NC, NT, 5)), order="canonical", nthreads=8)["lst4"]
        pairs = np.stack([r.all_cases, r.all_ctrls], axis=1)
        u, cnt = np.unique(pairs, axis=0, return_counts=True)
        rare = u[np.argsort(cnt, kind="stable")[:5]]
        _CACHE["pairs"] = (pairs, u, rare)
    return _CACHE["pairs"]


def table_of(name):
    shape = (NC + 1, NT + 1)
    if name in ("ordinary", "top1", "top_all"):
        return small_table(NC, NT, 5)
    if name == "constant":
        return np.full(shape, 2.5)
    pairs, u, rare = level4_pairs()
    rng = np.random.default_rng(11)
    if name == "zeros":          # zero or -0.0 everywhere but in five cells that one level-4 path each reads
        t = np.where(rng.random(shape) < 0.5, 0.0, -0.0)
        t[rare[:, 0], rare[:, 1]] = 1.0 + np.arange(len(rare))
        return t
    if name == "unscorable":     # -inf in every cell level 4 reads but those five; the other levels keep most of theirs
        t = small_table(NC, NT, 5)
        t[u[:, 0], u[:, 1]] = -np.inf
        t[rare[:, 0], rare[:, 1]] = 1.0 + np.arange(len(rare))
        return t
    raise ValueError(name)


def case(name):
    """(problem, the oracle's results): computed once per session and shared."""
    if name not in _CACHE:
        top_k = {"top1": 1, "top_all": len(level4_pairs()[0])}.get(name, TOP_K)
        p = problem(table_of(name), top_k)
        _CACHE[name] = (p, oracle.process_paths(p, order="canonical", nthreads=8))
    return _CACHE[name]


def two_key_case():
    """A join of two paths -- the first two of a level-4 uid, every other uid's count set to 0 -- whose table cells hold two
    doubles that differ in their lowest byte: (problem, sub-index, paths3, paths2, the oracle's result of that join)."""
    if "two" not in _CACHE:
        pairs, _, _ = level4_pairs()
        base = problem(small_table(NC, NT, 5), 1)
        u = base.levels.uids["4"]
        cnt = np.maximum(np.asarray(u.count, np.int64), 0)
        first = np.concatenate([[0], np.cumsum(cnt)])
        uid = next(int(i) for i in np.nonzero(cnt >= 2)[0] if (pairs[first[i]] != pairs[first[i] + 1]).any())
        a, b = pairs[first[uid]], pairs[first[uid] + 1]
        t = small_table(NC, NT, 5)
        lo = np.array([7.25], np.float64)
        hi = (lo.view(np.uint64) + np.uint64(0x37)).view(np.float64)
        t[a[0], a[1]], t[b[0], b[1]] = lo[0], hi[0]
        p = problem(t, 1)
        full = oracle.process_paths(p, order="canonical", nthreads=8)
        sub = UidRelSet(u.path_length, u.src, u.trg, np.where(np.arange(len(cnt)) == uid, 2, 0).astype(np.int32), u.location, u.signs)
        ox = oracle.OracleJoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
        ox.top_k = 1
        ox.set_value_table(p.value_table)
        ox.set_permuted_cases(p.perm_cases)
        want = ox.join(sub, full["paths3"], full["paths2"], order="canonical")
        _CACHE["two"] = (p, sub, full["paths3"], full["paths2"], want)
    return _CACHE["two"]


@pytest.mark.parametrize("name", CASES + ("two_keys",))
def test_oracle_puts_each_input_in_its_case(name):
    """CPU only, the oracle alone."""
    if name == "two_keys":
        p, sub, _, _, want = two_key_case()
        k = keys_of(want.all_scores)
        assert len(k) == 2 and k[0] != k[1] and (k[0] ^ k[1]) < 256, k         # the first seven digits tie
        assert want.scores.tolist() == [float(want.all_scores.max())]
        return
    p, want = case(name)
    r = want["lst4"]
    k = keys_of(r.all_scores)
    assert len(k) > 4 * 1024
    desc = np.sort(k)[::-1]
    T = desc[min(p.top_k, len(k)) - 1]
    bucket = int(((k >> np.uint64(48)) == (T >> np.uint64(48))).sum())
    if name == "ordinary":
        assert FORCED < bucket <= DEFAULT_CAND, bucket       # the candidate road by default, the fallback at 64
        assert len(np.unique(k)) > 500                       # (one key per (cases, controls) pair)
    elif name == "constant":
        assert len(np.unique(k)) == 1 and bucket == len(k) > FORCED      # overflows every buffer smaller than the join
        assert r.scores.tolist() == [2.5] * TOP_K
    elif name == "zeros":
        above = int((r.all_scores > 0).sum())
        zeros = r.all_scores == 0
        assert 0 < above < TOP_K, above                      # fewer than top_k paths above +0: the cut falls on a zero
        assert int(zeros.sum()) > TOP_K - above              # more zeros than slots are left
        assert np.signbit(r.all_scores[zeros]).any() and not np.signbit(r.all_scores[zeros]).all()    # of both signs
        assert T in (np.uint64(1 << 63), np.uint64((1 << 63) - 1))
    elif name == "unscorable":
        scorable = int((r.all_scores > -np.inf).sum())
        assert 0 < scorable < TOP_K <= len(k), scorable
        assert T == 0 and r.scores[0] == -np.inf and len(r.scores) == scorable + 1     # the sentinel first
    elif name == "top1":
        assert p.top_k == 1 and len(r.scores) == 1
    elif name == "top_all":
        assert p.top_k == len(k) == len(r.scores) and np.isfinite(r.all_scores).all()
        assert bucket <= DEFAULT_CAND


def same_bytes(a, b):
    for f in ("scores", "null", "cases", "ctrls", "src", "trg"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_candidate_road_fallback_and_old_sequence(name, monkeypatch):
    """Every level of the plan (levels 2 to 4 are joins of the launch-ahead chain) under the three settings."""
    p, want = case(name)
    runs = []
    for env in SETTINGS:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            plan = api.ResidentPlan(p, device=0)
            try:
                got = plan.run()
            finally:
                plan.close()
        for lvl, lst in LEVELS4:
            assert_same_result(got[lvl], want[lst])
        runs.append(got)
    for other in runs[1:]:
        for lvl, _ in LEVELS4:
            same_bytes(runs[0][lvl], other[lvl])


@pytest.mark.gpu
def test_two_keys_that_differ_in_their_lowest_byte(monkeypatch):
    """One join of two paths: seven digit passes see one bucket of two, the eighth tells them apart -- on the candidates by
    default, and the same with the old sequence."""
    p, sub, paths3, paths2, want = two_key_case()
    runs = []
    for env in SETTINGS:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
            try:
                ex.top_k = 1
                ex.set_value_table(p.value_table)
                ex.set_permuted_cases(p.perm_cases)
                got = ex.join(api.DeviceUids(ex, sub), ex.from_words(paths3), ex.from_words(paths2))
            finally:
                ex.close()
        assert_same_result(got, want)
        runs.append(got)
    for other in runs[1:]:
        same_bytes(runs[0], other)
