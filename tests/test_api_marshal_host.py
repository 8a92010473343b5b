"""What the Python binding hands the library, checked without one: a recording stand-in takes the place of libgcre_hip.so.

1. ``api._set_lists`` / ``api._set_input``: the exact arrays of both input forms of a set list.
2. Every set entry passes the same ``gcre_set_input`` for the same input (``_DpInput`` packs its rows the same way).
3. Arming observers in ``JoinExec.join`` and ``process_paths``: all checked, then set in order, a refusal takes back.
4. Freeing observers: once, not after the context is gone, and ``__del__`` never raises.

The cases whose id ends in ``pair_form_new`` give an ``(off, members)`` pair to an entry that read it as two sets before the
entries shared one parser; everything else holds for the binding as it was before that.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from geneticscre_amd import api

N = 65                   # patients: two words, one bit in the second
N_CASES = 3
H_CTX = 1                # the context handle the entries pass on

ROWS = np.zeros((4, N), np.int8)
ROWS[0, [0, 64]] = 1
ROWS[1, 63] = 1
ROWS[2, 64] = 1
PACKED = np.array([[1, 1], [1 << 63, 0], [0, 1], [0, 0]], dtype=np.uint64)
ROW_FORMS = {"2d": ROWS, "flat": ROWS.reshape(-1).astype(np.int32)}

OFF = np.array([0, 2, 3, 5], np.int64)
MEMBERS = np.array([0, 1, 2, 3, -1], np.int32)
FLAT_SIGNS = np.array([1, -1, 1, -1, 1], np.int32)
# form -> (sets, signs, expected off, expected members, expected signs)
SET_FORMS = {
    "none": ([], [], [0], [], []),
    "one_empty": ([[]], [[]], [0, 0], [], []),
    "lists": ([[0, 1], [2], [3, -1]], [[1, -1], [1], [-1, 1]], OFF, MEMBERS, FLAT_SIGNS),
    "pair": ((OFF.copy(), MEMBERS.copy()), FLAT_SIGNS.copy(), OFF, MEMBERS, FLAT_SIGNS),
}


def _copy(addr, count, dtype):
    if not count:
        return np.zeros(0, dtype)
    return np.frombuffer(ctypes.string_at(addr, count * np.dtype(dtype).itemsize), dtype=dtype).copy()


def snapshot(inp):
    """The fields of a gcre_set_input and copies of the arrays it points at, with the lengths it states."""
    off = _copy(inp.set_off, inp.n_sets + 1, np.int64)
    words = (inp.n_cols + 63) // 64
    return SimpleNamespace(n_sets=inp.n_sets, n_rows=inp.n_rows, n_cols=inp.n_cols, set_off=off,
                           members=_copy(inp.members, int(off[-1]), np.int32),
                           signs=None if not inp.signs else _copy(inp.signs, int(off[-1]), np.int32),
                           rows=_copy(inp.rows, inp.n_rows * words, np.uint64).reshape(inp.n_rows, words))


class Recorder:
    """In place of libgcre_hip.so: every ``gcre_*`` attribute is a function that notes its call and returns GCRE_OK (a new
    handle from ``*_create``).  ``refuse``: setters that answer GCRE_ERR_ARG to a handle; ``broken``: functions that raise."""

    def __init__(self):
        self.calls, self.inputs, self.refuse, self.broken, self.handles = [], [], set(), set(), 100

    def __getattr__(self, name):
        if not name.startswith("gcre_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name,) + args)
            for a in args:
                if isinstance(getattr(a, "_obj", None), api.gcre_set_input):
                    self.inputs.append((name, snapshot(a._obj)))
            if name in self.broken:
                raise RuntimeError(name + " is broken")
            if name == "gcre_last_error":
                return b"refused by the stand-in"
            if name.endswith("_create"):
                self.handles += 1
                return self.handles
            if name in self.refuse and args[-1] is not None:
                return api.GCRE_ERR_ARG
            return api.GCRE_OK
        return call

    def named(self, *parts):
        return [c for c in self.calls if any(p in c[0] for p in parts)]


@pytest.fixture
def lib(monkeypatch):
    rec = Recorder()
    for name in [k for k in vars(api) if k.startswith("_") and k.endswith("_lib") and k != "_feature_lib"] + ["load_library"]:
        monkeypatch.setattr(api, name, lambda rec=rec: rec)
    monkeypatch.setattr(api, "_feature_lib", lambda feature: rec)
    return rec


def context(lib, handle=H_CTX):
    ex = api.JoinExec.__new__(api.JoinExec)
    ex.method, ex.num_cases, ex.num_ctrls, ex.iters, ex._h, ex._lib = 1, N_CASES, N - N_CASES, 4, handle, lib
    return ex


def assert_exact(got, want, dtype, what):
    assert isinstance(got, np.ndarray) and got.dtype == dtype and got.flags["C_CONTIGUOUS"], what
    want = np.asarray(want, dtype=dtype)
    assert got.shape == want.shape and np.array_equal(got, want), (what, got, want)


# ---- 1. the parser and the packer ------------------------------------------------------------------------------------


@pytest.mark.parametrize("form", SET_FORMS)
@pytest.mark.parametrize("signed", [False, True])
def test_set_lists_exact_arrays(form, signed):
    sets, signs, off, members, flat = SET_FORMS[form]
    S, got_off, got_members, got_signs = api._set_lists(sets, signs if signed else None)
    assert S == len(off) - 1 and isinstance(S, int)
    assert_exact(got_off, off, np.int64, "off")
    assert_exact(got_members, members, np.int32, "members")
    if signed:
        assert_exact(got_signs, flat, np.int32, "signs")
    else:
        assert got_signs is None


def test_pack_carriers_bit_64_lands_in_word_1():
    for rows in ROW_FORMS.values():
        assert_exact(api.pack_carriers(rows, N), PACKED, np.uint64, "packed rows")
    one = np.zeros((1, N), np.int8)
    one[0, 64] = 1
    assert api.pack_carriers(one, N).tolist() == [[0, 1]]


SET_INPUT_CASES = [pytest.param(f, r, s, id=f"{f}-{r}-{'signed' if s else 'unsigned'}" + ("-pair_form_new" if f == "pair" else ""))
                   for f in SET_FORMS for r in ROW_FORMS for s in (False, True)]


@pytest.mark.parametrize("form,rows,signed", SET_INPUT_CASES)
def test_set_input_exact_arrays(form, rows, signed):
    sets, signs, off, members, flat = SET_FORMS[form]
    inp, keep = api._set_input(sets, ROW_FORMS[rows], signs if signed else None, N)
    assert isinstance(inp, api.gcre_set_input) and len(keep) == 4
    assert_exact(keep[0], off, np.int64, "off")
    assert_exact(keep[1], members, np.int32, "members")
    if signed:
        assert_exact(keep[2], flat, np.int32, "signs")
    else:
        assert keep[2] is None
    assert_exact(keep[3], PACKED, np.uint64, "packed rows")
    assert (inp.n_sets, inp.n_rows, inp.n_cols) == (len(off) - 1, 4, N)
    # the struct points into the arrays returned beside it
    assert inp.set_off == keep[0].ctypes.data and inp.rows == keep[3].ctypes.data
    assert inp.signs == (keep[2].ctypes.data if signed else None)
    if len(members):
        assert inp.members == keep[1].ctypes.data
    got = snapshot(inp)
    assert np.array_equal(got.set_off, off) and np.array_equal(got.members, members) and np.array_equal(got.rows, PACKED)
    assert (got.signs is None) if not signed else np.array_equal(got.signs, flat)


def test_both_forms_give_identical_arrays():
    a = api._set_lists(SET_FORMS["lists"][0], SET_FORMS["lists"][1])
    b = api._set_lists(SET_FORMS["pair"][0], SET_FORMS["pair"][1])
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


WRONG_SIGNS = {"lists": (SET_FORMS["lists"][0], [[1, 1], [1], [1]]), "lists_too_few": (SET_FORMS["lists"][0], [[1, 1], [1]]),
               "pair": (SET_FORMS["pair"][0], [1, 1, 1])}


@pytest.mark.parametrize("case", WRONG_SIGNS)
def test_set_lists_refuses_signs_of_the_wrong_shape(case):
    sets, signs = WRONG_SIGNS[case]
    with pytest.raises(ValueError, match="^signs: one sign per member of every set$"):
        api._set_lists(sets, signs)


@pytest.mark.parametrize("case", [pytest.param(c, id=c + ("-pair_form_new" if c == "pair" else "")) for c in WRONG_SIGNS])
def test_set_input_refuses_signs_of_the_wrong_shape(case):
    sets, signs = WRONG_SIGNS[case]
    with pytest.raises(ValueError, match="^signs: one sign per member of every set$"):
        api._set_input(sets, ROWS, signs, N)


# ---- 2. every set entry hands the library the same struct ------------------------------------------------------------


def _stepdown(ex, S, sets, rows, signs):
    return api.ExceedCounts(ex, np.arange(S, dtype=np.float64), perm_counts=True).stepdown(sets, rows, signs)


# entry -> (the library function that receives the struct, whether signs are passed on, the call)
ENTRIES = {
    "score_sets": ("gcre_score_sets", True, lambda ex, S, sets, rows, signs: ex.score_sets(sets, rows, signs)),
    "score_sets_family": ("gcre_score_sets", True, lambda ex, S, sets, rows, signs: ex.score_sets(sets, rows, signs, family=True)),
    "score_sets_given": ("gcre_score_sets_given", True,
                         lambda ex, S, sets, rows, signs: ex.score_sets(sets, rows, signs, which=list(range(S))[::-1],
                                                                        given=[1, -1, 1] if S == 3 else [-1] * S)),
    "family_tests": ("gcre_score_sets_family", True, lambda ex, S, sets, rows, signs: ex.family_tests(sets, rows, signs, kmax=True, null=True)),
    "minp_tests": ("gcre_score_sets_minp", True, lambda ex, S, sets, rows, signs: ex.minp_tests(sets, rows, signs, min_count=True, counts=True)),
    "competitive_tests": ("gcre_score_sets_compete", True,
                          lambda ex, S, sets, rows, signs: ex.competitive_tests(sets, rows, signs, bins=[0, 0, 1, -1], draws=3,
                                                                                null=True, picks=True)),
    "set_overlap": ("gcre_set_overlap", False, lambda ex, S, sets, rows, signs: ex.set_overlap(sets, rows)),
    "clump_sets": ("gcre_clump_sets", False, lambda ex, S, sets, rows, signs: ex.clump_sets(sets, rows, list(range(S))[:2])),
    "patient_counts": ("gcre_set_patient_counts", True,
                       lambda ex, S, sets, rows, signs: ex.patient_counts(sets, rows, by_sign=True, signs=signs)),
    "stepdown": ("gcre_exceed_stepdown", True, _stepdown),
}
TOOK_PAIRS_BEFORE = {"score_sets_given", "clump_sets", "patient_counts"}
ENTRY_CASES = [pytest.param(e, f, r, s, id=f"{e}-{f}-{r}-{'signed' if s else 'unsigned'}" +
                            ("-pair_form_new" if f == "pair" and e not in TOOK_PAIRS_BEFORE else ""))
               for e in ENTRIES for f in SET_FORMS for r in ROW_FORMS for s in (False, True)]


@pytest.mark.parametrize("entry,form,rows,signed", ENTRY_CASES)
def test_every_set_entry_passes_the_same_struct(lib, entry, form, rows, signed):
    symbol, passes_signs, call = ENTRIES[entry]
    sets, signs, off, members, flat = SET_FORMS[form]
    ex = context(lib)
    call(ex, len(off) - 1, sets, ROW_FORMS[rows], signs if signed else None)
    assert [name for name, _ in lib.inputs] == [symbol]
    got = lib.inputs[0][1]
    assert (got.n_sets, got.n_rows, got.n_cols) == (len(off) - 1, 4, N)
    assert_exact(got.set_off, off, np.int64, "set_off")
    assert_exact(got.members, members, np.int32, "members")
    assert_exact(got.rows, PACKED, np.uint64, "rows")
    if signed and passes_signs:
        assert_exact(got.signs, flat, np.int32, "signs")
    else:
        assert got.signs is None
    first = [c for c in lib.calls if c[0] == symbol][0]
    assert first[1] == (ex._h if entry != "stepdown" else lib.handles)      # the context, or the counters' own handle


@pytest.mark.parametrize("rows", ROW_FORMS)
def test_dp_input_packs_its_rows_like_pack_carriers(rows):
    d = api._DpInput(1, N_CASES, N - N_CASES, [[0, 1], [2]], ROW_FORMS[rows], None, None, 0, 0)
    assert_exact(d.rows, PACKED, np.uint64, "rows")
    assert d.rows.tobytes() == api.pack_carriers(ROW_FORMS[rows], N).tobytes()
    assert d.c.n_rows == 4 and d.c.rows == d.rows.ctypes.data


# ---- 3. arming ------------------------------------------------------------------------------------------------------


# tally, exceed, hits: each fits ``join_uids()`` and every level of ``tiny_problem()``
MAKE = (lambda ex: api.GeneTally(ex, 2, np.array([[0]], np.int32), np.array([[1]], np.int32)),
        lambda ex: api.ExceedCounts(ex, [1.0, 2.0]),
        lambda ex: api.HitList(ex, 1.0, cap=8))


def observers(ex):
    return tuple(make(ex) for make in MAKE)


def join_uids():
    return SimpleNamespace(path_length=2, count=np.array([1], np.int32), location=np.array([0], np.int64),
                           signs=np.array([1], np.int32))


def tiny_problem():
    levels = SimpleNamespace(uids={k: join_uids() for k in api.LEVEL_INDEX},
                             data_inds={k: np.array([0], np.int32) for k in ("1a", "1b", "2", "3")})
    return SimpleNamespace(levels=levels, data1=np.zeros((1, N), np.int32), data2=np.zeros((1, N), np.int32),
                           value_table=np.zeros((N_CASES + 1, N - N_CASES + 1)), perm_cases=np.zeros((0, 0), np.int32),
                           path_length=4, top_k=5, method="method1", n_cases=N_CASES, n_ctrls=N - N_CASES, iterations=4)


P0, P1 = SimpleNamespace(_h=21), SimpleNamespace(_h=22)


def run_join(ex, t, x, h):
    return ex.join(join_uids(), P0, P1, tally=t, exceed=x, hits=h)


def run_process_paths(ex, t, x, h):
    return api.process_paths(tiny_problem(), exec_=ex, tallies={"4": t}, exceeds={"4": x}, hits={"4": h})


# how -> (the call, its three setters in arming order, the leading setter arguments, the entry behind them)
ARMING = {
    "join": (run_join, ("gcre_join_set_tally", "gcre_join_set_exceed", "gcre_join_set_hits"), (H_CTX,), "gcre_join"),
    "process_paths": (run_process_paths, ("gcre_process_paths_set_tally", "gcre_process_paths_set_exceed",
                                          "gcre_process_paths_set_hits"), (H_CTX, api.LEVEL_INDEX["4"]), "gcre_process_paths"),
}


@pytest.mark.parametrize("how", ARMING)
def test_observers_are_armed_in_order_before_the_entry(lib, how):
    run, setters, lead, entry = ARMING[how]
    ex = context(lib)
    obs = observers(ex)
    lib.calls.clear()
    run(ex, *obs)
    got = [c for c in lib.calls if "_set_" in c[0] and c[0] != "gcre_set_top_k" or c[0] == entry]
    assert [c[0] for c in got] == list(setters) + [entry]
    assert [c[1:] for c in got[:3]] == [lead + (o._h,) for o in obs]
    assert got[3][1] == H_CTX


@pytest.mark.parametrize("how", ARMING)
def test_a_refused_setter_takes_back_what_was_armed(lib, how):
    run, setters, lead, entry = ARMING[how]
    ex = context(lib)
    t, x, h = observers(ex)
    lib.refuse.add(setters[1])
    lib.calls.clear()
    with pytest.raises(api.GcreError, match="refused by the stand-in"):
        run(ex, t, x, h)
    assert [c for c in lib.calls if "_set_" in c[0] and c[0] != "gcre_set_top_k"] == [
        (setters[0],) + lead + (t._h,), (setters[1],) + lead + (x._h,), (setters[0],) + lead + (None,)]
    assert not lib.named(setters[2]) and not [c for c in lib.calls if c[0] in (entry, "gcre_join_uids")]
    assert t._h and x._h and h._h                     # (refused, not freed)


@pytest.mark.parametrize("how", ARMING)
@pytest.mark.parametrize("stranger,text", [(0, "gene tally does not"), (1, "exceedance counts do not"), (2, "hit list does not")])
def test_an_observer_of_another_context_stops_the_call_before_any_setter(lib, how, stranger, text):
    run, setters, lead, entry = ARMING[how]
    ex, other = context(lib), context(lib, handle=2)
    obs = list(observers(ex))
    obs[stranger] = MAKE[stranger](other)
    lib.calls.clear()
    with pytest.raises(api.GcreError, match=f"^{text} belong to this context$"):
        run(ex, *obs)
    assert [c for c in lib.calls if c[0] != "gcre_set_top_k"] == []
    # a freed one is refused the same way
    obs = list(observers(ex))
    obs[stranger].free()
    lib.calls.clear()
    with pytest.raises(api.GcreError, match=f"^{text} belong to this context$"):
        run(ex, *obs)
    assert [c for c in lib.calls if c[0] != "gcre_set_top_k"] == []


@pytest.mark.parametrize("how", ARMING)
def test_the_tally_tables_are_checked_before_any_setter(lib, how):
    run, setters, lead, entry = ARMING[how]
    ex = context(lib)
    _, x, h = observers(ex)
    wrong = api.GeneTally(ex, 2, np.array([[0], [1]], np.int32), None)        # two rows for one uid row
    lib.calls.clear()
    with pytest.raises(api.GcreError, match="genes0 has 2 rows, the join index has 1 uid rows"):
        run(ex, wrong, x, h)
    assert [c for c in lib.calls if c[0] != "gcre_set_top_k"] == []


def test_process_paths_messages(lib):
    ex = context(lib)
    t, x, h = observers(ex)
    p = tiny_problem()
    lib.calls.clear()
    with pytest.raises(api.GcreError, match=r"^process_paths: no level '7' \(levels are 1a, 1b, 2, 3, 4, 5\)$"):
        api.process_paths(p, exec_=ex, tallies={"4": t}, exceeds={"7": x})
    assert [c for c in lib.calls if c[0] != "gcre_set_top_k"] == []
    for kw, text in ((dict(tallies={"4": t}), "gene tallies live on a context; pass the JoinExec they were made on as exec_"),
                     (dict(exceeds={"4": x}), "exceedance counts live on a context; pass the JoinExec they were made on as exec_"),
                     (dict(hits={"4": h}), "hit lists live on a context; pass the JoinExec they were made on as exec_")):
        with pytest.raises(api.GcreError, match="^process_paths: " + text + "$"):
            api.process_paths(p, **kw)


# ---- 4. freeing -----------------------------------------------------------------------------------------------------


FREE = {0: "gcre_gene_tally_free", 1: "gcre_exceed_free", 2: "gcre_hits_free"}


@pytest.mark.parametrize("which", FREE)
def test_free_calls_the_free_function_once(lib, which):
    ex = context(lib)
    o = MAKE[which](ex)
    handle = o._h
    o.free()
    o.free()
    o.__del__()
    assert lib.named("_free") == [(FREE[which], handle)] and o._h is None


@pytest.mark.parametrize("which", FREE)
def test_free_after_the_context_is_gone_calls_nothing(lib, which):
    ex = context(lib)
    o = MAKE[which](ex)
    ex._h = None                                      # (what close() leaves: the library freed the object with its context)
    o.free()
    assert lib.named("_free") == [] and o._h is None


@pytest.mark.parametrize("which", FREE)
def test_del_swallows_what_free_raises(lib, which):
    ex = context(lib)
    o = MAKE[which](ex)
    lib.broken.add(FREE[which])
    with pytest.raises(RuntimeError, match="is broken"):
        o.free()
    o = MAKE[which](ex)
    o.__del__()                                       # the same failure, not raised
    assert len(lib.named(FREE[which])) == 2
