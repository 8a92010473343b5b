"""The .Call shim (geneticscre_amd/csrc/r_shim.c) EXECUTED without R and without a GPU: linked with the stand-in R runtime of
tests/r_mock (our reading of "Writing R Extensions", not R) and pointed at a recording backend (tests/r_mock/gcre_stub.c)
through GCRE_HIP_LIB.  Every call goes through the function pointers the shim registered, as .Call would.  What this does
not show: the shim under real R, R's garbage collector, Rf_coerceVector corner cases beyond int <-> double."""
import ctypes

import numpy as np
import pytest

from geneticscre_amd import api, synth
from geneticscre_amd.synth import make_problem
from geneticscre_amd.uids import build_level_tables, count_locations
from helpers import small_table
from r_call import INTSXP, LEVELS, NA_INTEGER, REALSXP, STRSXP, VECSXP, RError, RMock, process_paths_args

PP = "_geneticsCRE_ProcessPaths"
FIELDS = ["scores", "ids", "TestScores", "cases", "controls", "debug"]


class Stub:
    def __init__(self, path):
        L = self.lib = ctypes.CDLL(path)
        P, I = ctypes.c_void_p, ctypes.c_int
        L.stub_set_real_lib.argtypes = [ctypes.c_char_p]
        L.stub_set_return.argtypes = [I, ctypes.c_char_p]
        L.stub_queue_result.argtypes = [I, I, P, P, P, P, P, I, P]
        L.stub_devices.restype = ctypes.POINTER(ctypes.c_int)
        L.stub_input.restype = ctypes.POINTER(api.gcre_pp_input)

    def queue(self, level, res):
        """res: None (n = -1) or (scores, src, trg, cases, ctrls, null_max)"""
        if res is None:
            self.lib.stub_queue_result(level, -1, None, None, None, None, None, 0, None)
            return
        sc, s, t, ca, ct, nm = res
        keep = [np.ascontiguousarray(sc, np.float64), *[np.ascontiguousarray(x, np.int32) for x in (s, t, ca, ct)],
                np.ascontiguousarray(nm, np.float32)]
        self.lib.stub_queue_result(level, len(keep[0]), *[k.ctypes.data for k in keep[:5]], len(keep[5]), keep[5].ctypes.data)

    def devices(self):
        return [self.lib.stub_devices()[i] for i in range(self.lib.stub_scalar(5))]

    def input(self):
        return self.lib.stub_input().contents


def _arr(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype)
    assert ptr, "NULL pointer with a non-zero count"
    ct = np.ctypeslib.as_ctypes_type(dtype)
    return np.array(ctypes.cast(ptr, ctypes.POINTER(ct))[0:n], dtype=dtype)


# the results the backend hands back: every corner of make_score_list.  Level 4 (lst4) is above path_length (n = -1), lst2 holds
# the sentinel only, lst3 has no permutations, the f32 maxima are not representable in decimal, ids reach the int32 top.
F32 = np.array([0.1, 1.0 / 3.0, 16777217.0, 1e-45, 3.4028235e38, 0.0], dtype=np.float32)
RESULTS = [
    (np.array([0.1, 2.5, np.nextafter(7.0, 8.0)]), [0, 5, 2147483646], [3, 0, 7], [4, 0, 33], [1, 9, 0], F32),
    (np.array([-np.inf]), [-1], [-1], [0], [0], F32[:2]),
    (np.array([1.0, 1.0]), [1, 0], [0, 1], [2, 2], [3, 3], np.zeros(0, np.float32)),
    None,
    (np.zeros(0), [], [], [], [], F32[:1]),
]


@pytest.fixture(scope="module")
def rt():
    """(runtime + shim, backend): one copy for the module, bound to the recording backend at its first call."""
    import os
    r = RMock()
    st = Stub(r.stub_path)
    api.load_library()   # (builds the library if the tree is newer; it loads without a GPU)
    assert st.lib.stub_set_real_lib(api.lib_path().encode()) == 0   # gcre_resolve_count_locs: host code of the real library
    old = os.environ.get("GCRE_HIP_LIB")
    os.environ["GCRE_HIP_LIB"] = r.stub_path
    try:   # getRels3 resolves the backend (load_abi); the shim keeps the handle
        r.call("_geneticsCRE_getRels3", [r.ints([0]), r.ints([1]), r.ints([1]), r.named_list([("1", r.reals([0, -1]))])])
    finally:
        if old is None:
            del os.environ["GCRE_HIP_LIB"]
        else:
            os.environ["GCRE_HIP_LIB"] = old
    assert st.lib.stub_resolve_calls() == 1, "the shim did not bind the recording backend"
    return r, st


@pytest.fixture
def call(rt, monkeypatch):
    """A clean slate per test: default results queued, counters zero, GCRE_DEVICES unset, objects of earlier tests gone."""
    r, st = rt
    monkeypatch.delenv("GCRE_DEVICES", raising=False)
    r.reset()
    st.lib.stub_reset_counters()
    st.lib.stub_set_return(0, b"")
    st.lib.stub_set_device_count(1)
    for i, res in enumerate(RESULTS):
        st.queue(i, res)
    yield r, st
    assert r.protect_depth() == 0
    assert st.lib.stub_double_frees() == 0 and st.lib.stub_foreign_frees() == 0


@pytest.fixture(scope="module")
def problem():
    # 33 + 41 patients: two mask words, ragged; 130 label rows for K = 130
    return make_problem(35, 80, 33, 41, 130, 4, method="method2", top_k=7, seed=3, table=small_table(33, 41, 2))


def test_exactly_the_three_routines_are_registered(rt):
    r, _ = rt
    assert r.registered() == [("_geneticsCRE_getRels3", 4), ("_geneticsCRE_getMatchingList", 3), (PP, 39)]
    assert r.lib.mock_dynamic_symbols() == 0          # R_useDynamicSymbols(dll, FALSE)
    # .Call checks the arity against the registration
    assert r.call_raw(PP, [r.ints([1])] * 38) is None and "expecting 39" in r.error_message()
    assert r.call_raw("_geneticsCRE_nothing", []) is None and "not available" in r.error_message()


@pytest.mark.parametrize("all_double", [False, True])
def test_backend_receives_the_problem_column_major(call, problem, all_double):
    r, st = call
    p = problem
    out = r.call(PP, process_paths_args(r, p, all_double=all_double))
    assert out is not None and st.lib.stub_calls() == 1
    assert [st.lib.stub_scalar(i) for i in range(5)] == [2, p.n_cases, p.n_ctrls, p.iterations, p.top_k]
    inp = st.input()
    n = p.n_cases + p.n_ctrls
    assert (inp.data_col_major, inp.vt_col_major, inp.perm_col_major) == (1, 1, 1)
    assert (inp.data1_rows, inp.data2_rows) == p.data1.shape[:1] + p.data2.shape[:1]
    assert (inp.vt_rows, inp.vt_cols) == p.value_table.shape
    assert inp.perm_rows == p.perm_cases.shape[0] == 130
    assert inp.path_length == p.path_length
    assert (inp.shard_rank, inp.shard_world, inp.window_perms) == (0, 0, 0)
    # the storage is column-major: read back in F order it is the logical matrix
    np.testing.assert_array_equal(_arr(inp.data1, inp.data1_rows * n, np.int32).reshape(p.data1.shape, order="F"), p.data1)
    np.testing.assert_array_equal(_arr(inp.data2, inp.data2_rows * n, np.int32).reshape(p.data2.shape, order="F"), p.data2)
    np.testing.assert_array_equal(_arr(inp.perm_cases, inp.perm_rows * n, np.int32).reshape(p.perm_cases.shape, order="F"),
                                  p.perm_cases)
    vt = _arr(inp.value_table, inp.vt_rows * inp.vt_cols, np.float64).reshape(p.value_table.shape, order="F")
    np.testing.assert_array_equal(vt.view(np.uint64), p.value_table.view(np.uint64))
    some_missing = False
    for i, k in enumerate(LEVELS):
        u, lv = p.levels.uids[k], inp.level[i]
        assert (lv.n_uids, lv.n_signs) == (len(u.count), len(u.signs)), k
        np.testing.assert_array_equal(_arr(lv.uid_count, lv.n_uids, np.int32), u.count, err_msg=k)
        np.testing.assert_array_equal(_arr(lv.uid_location, lv.n_uids, np.int64), u.location, err_msg=k)
        np.testing.assert_array_equal(_arr(lv.signs, lv.n_signs, np.int32), u.signs, err_msg=k)
        some_missing |= bool((u.location == -1).any())
    assert some_missing, "the problem has no c(0, -1) entry: the double branch of the count/location lists did not run"
    for i, k in enumerate(("1a", "1b", "2", "3")):
        assert inp.n_data_inds[i] == len(p.levels.data_inds[k])
        np.testing.assert_array_equal(_arr(inp.data_inds[i], inp.n_data_inds[i], np.int32), p.levels.data_inds[k])


def test_method_string_and_empty_permutation_matrix(call, problem):
    r, st = call
    p = problem
    for name, want in (("method1", 1), ("method2", 2), ("Method1", 2), ("", 2), ("signed", 2)):
        r.call(PP, process_paths_args(r, p, method=name))
        assert st.lib.stub_scalar(0) == want, name
    p0 = make_problem(20, 40, 33, 41, 0, 2, seed=1, table=small_table(33, 41, 2))
    r.call(PP, process_paths_args(r, p0, perm_cases=np.zeros((0, 0))))
    inp = st.input()
    assert st.lib.stub_scalar(3) == 0 and inp.perm_cases is None and inp.perm_rows == 0 and inp.perm_col_major == 1


def test_device_lists(call, problem, monkeypatch):
    r, st = call

    def devices(env, nthreads=-1, count=1):
        if env is None:
            monkeypatch.delenv("GCRE_DEVICES", raising=False)
        else:
            monkeypatch.setenv("GCRE_DEVICES", env)
        st.lib.stub_set_device_count(count)
        r.call(PP, process_paths_args(r, problem, nthreads=nthreads))
        assert st.lib.stub_scalar(6) == 0
        return st.devices()

    assert devices(None) == [0]
    assert devices("") == [0]
    assert devices(None, nthreads=8) == [0]
    assert devices("all", count=5) == [0, 1, 2, 3, 4]
    assert devices("all", count=70) == list(range(64))
    assert devices("2,0,1") == [2, 0, 1]
    assert devices("2,0,1", nthreads=2) == [2, 0]
    assert devices("2,0,1", nthreads=1) == [2]
    assert devices("2,0,1", nthreads=-1) == [2, 0, 1]
    assert devices("2,0,1", nthreads=3) == [2, 0, 1]
    assert devices("all", nthreads=3, count=8) == [0, 1, 2]
    assert devices("0,0,0", nthreads=1) == [0]
    assert devices(",".join(str(i % 8) for i in range(70))) == [i % 8 for i in range(64)]


def check_result_list(out, results=RESULTS):
    assert out.type == VECSXP and out.names == ["lst1", "lst2", "lst3", "lst4", "lst5"]
    for lst, res in zip(out.value, results):
        if res is None:
            assert lst is None
            continue
        sc, s, t, ca, ct, nm = res
        m = len(sc)
        assert lst.type == VECSXP and lst.names == FIELDS
        scores, ids, test, cases, ctrls, debug = lst.value
        assert scores.type == REALSXP and scores.dim is None
        np.testing.assert_array_equal(scores.value.view(np.uint64), np.asarray(sc, np.float64).view(np.uint64))
        assert ids.type == INTSXP and ids.dim == [m, 2] and len(ids.value) == 2 * m
        np.testing.assert_array_equal(ids.value[:m], np.asarray(s, np.int64) + 1)     # column-major: first column = src + 1
        np.testing.assert_array_equal(ids.value[m:], np.asarray(t, np.int64) + 1)
        assert test.type == REALSXP
        np.testing.assert_array_equal(test.value.view(np.uint64), np.asarray(nm, np.float32).astype(np.float64).view(np.uint64))
        assert cases.type == REALSXP and ctrls.type == REALSXP
        np.testing.assert_array_equal(cases.value, np.asarray(ca, np.float64))
        np.testing.assert_array_equal(ctrls.value, np.asarray(ct, np.float64))
        assert debug.type == STRSXP
        assert debug.value == [f"[debug] {a}:{b} {c}/{d}" for a, b, c, d in zip(s, t, ca, ct)]


def test_result_lists_and_one_free_per_result(call, problem):
    r, st = call
    out = r.call(PP, process_paths_args(r, problem))
    check_result_list(out)
    # widening f32 -> f64 is exact, and nothing like 0.1f -> 0.1 happened on the way
    assert out["lst1"]["TestScores"].value[0] == float(np.float32(0.1)) != 0.1
    assert out["lst1"]["ids"].value[2] == 2147483647
    assert [st.lib.stub_handed_out(i) for i in range(5)] == [1, 1, 1, 0, 1]
    assert [st.lib.stub_freed(i) for i in range(5)] == [1, 1, 1, 0, 1]
    assert r.protect_depth() == 0


def test_every_allocation_failure_frees_every_result_once(call, problem):
    """R's allocation-failure / interrupt exits, stood in for by 'the N-th allocation from now on fails': for every
    allocation of a whole call, the call ends through Rf_error; if the backend had been called by then, each result with
    n >= 0 was freed exactly once (R_ExecWithCleanup's longjmp road), never twice."""
    r, st = call
    args = process_paths_args(r, problem)
    a0 = r.lib.mock_alloc_count()
    assert r.call_raw(PP, args) is not None
    in_call = r.lib.mock_alloc_count() - a0     # allocations of one normal call
    in_build = r.lib.mock_exec_allocs()         # those of build_result_list alone
    assert 0 < in_build < in_call
    # lists + names + 8 objects, 1 dim vector, 6 + m names and strings per level; 5 + 2 for the outer list
    assert in_build == 7 + sum(9 + 6 + len(res[0]) for res in RESULTS if res is not None)
    before = in_call - in_build                 # coerced copies and R_alloc blocks; nothing is allocated after the build
    for nth in range(1, in_call + 1):
        st.lib.stub_reset_counters()
        r.lib.mock_fail_alloc(nth)
        assert r.call_raw(PP, args) is None, nth
        assert "stand-in allocation fault" in r.error_message()
        assert r.protect_depth() == 0, nth
        handed = [st.lib.stub_handed_out(i) for i in range(5)]
        freed = [st.lib.stub_freed(i) for i in range(5)]
        if nth <= before:                       # failed while unmarshalling: the backend was never called
            assert st.lib.stub_calls() == 0 and handed == freed == [0] * 5, nth
        else:
            assert st.lib.stub_calls() == 1 and handed == [1, 1, 1, 0, 1] and freed == handed, (nth, freed)
        assert st.lib.stub_double_frees() == 0 and st.lib.stub_foreign_frees() == 0, nth
    r.lib.mock_fail_alloc(in_call + 1)          # one past the last allocation: the call succeeds
    assert r.call_raw(PP, args) is not None
    r.lib.mock_fail_alloc(0)


def test_errors_of_the_backend_and_of_the_shim(call, problem):
    r, st = call
    p = problem
    st.lib.stub_set_return(-3, b"device 1: out of memory (stand-in)")
    with pytest.raises(RError, match=r"^geneticsCRE: device 1: out of memory \(stand-in\)$"):
        r.call(PP, process_paths_args(r, p))
    assert st.lib.stub_calls() == 1 and [st.lib.stub_freed(i) for i in range(5)] == [0] * 5
    st.lib.stub_set_return(-4, b"")
    with pytest.raises(RError, match="^geneticsCRE: gcre_process_paths_devices failed$"):
        r.call(PP, process_paths_args(r, p))
    st.lib.stub_set_return(0, b"")
    st.lib.stub_reset_counters()
    # wrong column counts: the shim's own messages, the backend is not called
    n = p.n_cases + p.n_ctrls
    for pos, bad, msg in ((28, np.zeros((p.data1.shape[0], n + 1), np.int32), "data matrices must have"),
                          (29, np.zeros((p.data2.shape[0], n - 1), np.int32), "data matrices must have"),
                          (35, np.ones((130, n + 2), np.int32), "perm_cases must have")):
        args = process_paths_args(r, p)
        args[pos] = r.int_matrix(bad)
        with pytest.raises(RError, match=msg):
            r.call(PP, args)
        assert r.protect_depth() == 0
    assert st.lib.stub_calls() == 0
    # a count/location entry shorter than c(count, location)
    args = process_paths_args(r, p)
    args[2] = r.named_list([("0", r.ints([1]))])
    with pytest.raises(RError, match="count_locs entries must be"):
        r.call(PP, args)
    assert st.lib.stub_calls() == 0


def networks():
    """Two signed_network draws; the second is sparse enough that many targets have no outgoing edge."""
    out = []
    for seed, genes, edges in ((5, 40, 120), (6, 60, 45)):
        g, src, trg, sign = synth.signed_network(genes, edges, np.random.default_rng(seed))
        out.append((g, src, trg, sign))
    return out


@pytest.mark.parametrize("net", [0, 1])
def test_get_matching_list_and_get_rels3_with_double_inputs(call, net):
    r, _ = call
    g, src, trg, sign = networks()[net]
    lv = build_level_tables(g, src, trg, sign)
    want = count_locations(trg, src)
    if net == 1:
        assert (0, -1) in want.values(), "this network must have a target without an outgoing edge"
    # getUidsCountsLocations: rle of the sorted sources, handed over as doubles
    change = np.flatnonzero(np.r_[True, src[1:] != src[:-1]])
    lengths = np.diff(np.r_[change, len(src)])
    ml = r.call("_geneticsCRE_getMatchingList", [r.reals(src[change]), r.reals(lengths), r.reals(change)])
    assert r.protect_depth() == 0
    assert ml.type == VECSXP and ml.names == [str(int(u)) for u in src[change]]
    found = {u: cl for u, cl in want.items() if cl != (0, -1)}
    assert list(found) == [int(n) for n in ml.names]
    for name, e in zip(ml.names, ml.value):
        assert e.type == INTSXP and tuple(e.value.tolist()) == found[int(name)]
    # getRels3 on the list R would pass: the found entries as integer pairs, the appended c(0, -1) as doubles
    items = [(str(u), r.reals([0.0, -1.0]) if cl == (0, -1) else r.ints(cl)) for u, cl in want.items()]
    df = r.call("_geneticsCRE_getRels3", [r.reals(src), r.reals(trg), r.reals(sign), r.named_list(items)])
    assert r.protect_depth() == 0
    assert df.type == VECSXP and df.names == ["srcuid", "trguid", "sign", "trguid2", "sign2"]
    assert df.klass == ["data.frame"]
    n = len(lv.rels3["srcuid"])
    assert n > 0
    np.testing.assert_array_equal(df.row_names, [NA_INTEGER, -n])      # compact row names c(NA, -n)
    for name, col in zip(df.names, df.value):
        assert col.type == INTSXP and col.dim is None
        np.testing.assert_array_equal(col.value, lv.rels3[name], err_msg=name)
