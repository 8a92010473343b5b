"""The .Call road without R: ctypes binding of the stand-in R runtime (tests/r_mock) that is linked with the shim, and the
39 arguments of ProcessPaths built the way GWASPA builds them in R (R/ProcessPaths.R:204-269, getUidsCountsLocations
R/PathMethods.R:133-152): which vectors are integer and which double, named count/location lists, column-major matrices.
Shared by tests/test_r_shim_host.py (recording backend) and tests/test_gpu_r_shim.py (the real library)."""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np

from geneticscre_amd import build as _build
from geneticscre_amd.uids import count_locations

NILSXP, CHARSXP, INTSXP, REALSXP, STRSXP, VECSXP = 0, 9, 13, 14, 16, 19
NA_INTEGER = -2 ** 31


class RError(RuntimeError):
    """Rf_error reached the top of a .Call."""


class RObj:
    """A walked R object: ``value`` is an int32 / float64 array in storage order, a list of str, or a list of RObj / None."""

    def __init__(self, type_, value, names, dim, klass, row_names):
        self.type, self.value, self.names, self.dim, self.klass, self.row_names = type_, value, names, dim, klass, row_names

    def __getitem__(self, name):
        return self.value[self.names.index(name)]

    def matrix(self) -> np.ndarray:
        """The logical matrix of a column-major vector with a dim attribute."""
        return self.value.reshape(tuple(self.dim), order="F")


class RMock:
    """One loaded copy of shim + stand-in runtime.  ``tag`` names the copy (the shim binds its backend once per copy)."""

    def __init__(self, tag: str = ""):
        self.path, self.stub_path = _build.build_r_mock(tag=tag)
        L = self.lib = ctypes.CDLL(self.path)
        P, I, LG, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_char_p
        for name, res, args in [
                ("mock_load", None, []), ("mock_int_vector", P, [P, LG]), ("mock_real_vector", P, [P, LG]),
                ("mock_int_matrix", P, [P, I, I]), ("mock_real_matrix", P, [P, I, I]), ("mock_string", P, [S]),
                ("mock_list", P, [LG]), ("mock_list_set", P, [P, LG, S, P]), ("mock_registered_count", I, []),
                ("mock_registered_name", S, [I]), ("mock_registered_nargs", I, [I]), ("mock_dynamic_symbols", I, []),
                ("mock_call", P, [S, P, I]), ("mock_error_message", S, []), ("mock_protect_depth", I, []),
                ("mock_alloc_count", LG, []), ("mock_exec_allocs", LG, []), ("mock_fail_alloc", None, [LG]),
                ("mock_reset", None, []), ("mock_typeof", I, [P]), ("mock_length", LG, [P]), ("mock_data", P, [P]),
                ("mock_elt", P, [P, LG]), ("mock_attr", P, [P, S])]:
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        L.mock_load()   # R_init_geneticsCRE: the shim registers its routines

    # ---- objects ----
    def _made(self, h):
        if not h:
            raise RError(self.lib.mock_error_message().decode())
        return h

    def ints(self, v):
        a = np.ascontiguousarray(v, dtype=np.int32).reshape(-1)
        return self._made(self.lib.mock_int_vector(a.ctypes.data, len(a)))

    def reals(self, v):
        a = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        return self._made(self.lib.mock_real_vector(a.ctypes.data, len(a)))

    def int_matrix(self, m):
        """``m``: the logical 2-d matrix.  It is handed over as R stores it, column-major."""
        m = np.asarray(m, dtype=np.int32)
        f = np.ascontiguousarray(m.T).reshape(-1)   # C order of the transpose = column-major storage of m
        return self._made(self.lib.mock_int_matrix(f.ctypes.data, m.shape[0], m.shape[1]))

    def real_matrix(self, m):
        m = np.asarray(m, dtype=np.float64)
        f = np.ascontiguousarray(m.T).reshape(-1)
        return self._made(self.lib.mock_real_matrix(f.ctypes.data, m.shape[0], m.shape[1]))

    def string(self, s: str):
        return self._made(self.lib.mock_string(s.encode()))

    def named_list(self, items):
        """items: [(name or None, object handle)]"""
        lst = self._made(self.lib.mock_list(len(items)))
        for i, (name, h) in enumerate(items):
            self._made(self.lib.mock_list_set(lst, i, None if name is None else str(name).encode(), h))
        return lst

    # ---- .Call ----
    def registered(self):
        return [(self.lib.mock_registered_name(i).decode(), self.lib.mock_registered_nargs(i))
                for i in range(self.lib.mock_registered_count())]

    def call_raw(self, name: str, args: List[int]) -> Optional[int]:
        """The registered routine through its recorded pointer; None when it left through Rf_error."""
        arr = (ctypes.c_void_p * max(len(args), 1))(*args)
        return self.lib.mock_call(name.encode(), arr, len(args))

    def call(self, name: str, args: List[int]) -> "RObj":
        h = self.call_raw(name, args)
        if not h:
            raise RError(self.error_message())
        return self.walk(h)

    def error_message(self) -> str:
        return self.lib.mock_error_message().decode()

    def protect_depth(self) -> int:
        return self.lib.mock_protect_depth()

    def reset(self) -> None:
        self.lib.mock_reset()

    # ---- results ----
    def walk(self, h) -> Optional[RObj]:
        L = self.lib
        t, n = L.mock_typeof(h), L.mock_length(h)
        if t == NILSXP:
            return None
        if t == CHARSXP:
            return ctypes.string_at(L.mock_data(h), n).decode()
        if t in (INTSXP, REALSXP):
            ct, dt = (ctypes.c_int32, np.int32) if t == INTSXP else (ctypes.c_double, np.float64)
            value = np.array(ctypes.cast(L.mock_data(h), ctypes.POINTER(ct))[0:n], dtype=dt) if n else np.zeros(0, dt)
        elif t in (STRSXP, VECSXP):
            value = [self.walk(L.mock_elt(h, i)) for i in range(n)]
        else:
            raise TypeError(f"unexpected SEXP type {t}")

        def attr(which):
            a = L.mock_attr(h, which)
            return self.walk(a) if a else None
        names, dim, klass, rn = attr(b"names"), attr(b"dim"), attr(b"class"), attr(b"row.names")
        return RObj(t, value, names.value if names else None, dim.value.tolist() if dim else None,
                    klass.value if klass else None, rn.value if rn else None)


# ---- the arguments R builds -------------------------------------------------------------------------------------------

def count_loc_list(r: RMock, rels1_trgs, rels2_srcs):
    """getUidsCountsLocations (R/PathMethods.R:133-152) as an R object: list "uid" -> c(count, location).  The entries
    getMatchingList made are integer pairs; the ones R appends for targets without an outgoing relation are c(0, -1),
    doubles."""
    items = []
    for uid, (c, l) in count_locations(rels1_trgs, rels2_srcs).items():
        items.append((str(uid), r.reals([0.0, -1.0]) if (c, l) == (0, -1) else r.ints([c, l])))
    return r.named_list(items)


LEVELS = ("1a", "1b", "2", "3", "4", "5")


def process_paths_args(r: RMock, p, perm_cases=None, nthreads=-1, method: Optional[str] = None, all_double: bool = False):
    """The 39 arguments of .Call("_geneticsCRE_ProcessPaths", ...) for a synth.Problem, typed as R/ProcessPaths.R types them:
    uids are integer columns of data frames; rep(1, n) sign vectors (levels 1a, 1b) and the third-gene signs (4, 5) are
    doubles, Rels$sign (2, 3) integer; match(...) - 1 index vectors are doubles; data, value table and permuted cases are
    matrices; the scalars are doubles, method a string.  ``all_double``: every numeric vector a double (what a caller
    gets whose data frames hold numeric columns).  ``perm_cases``: the K x n matrix, or an array with no elements for
    matrix(0, 0, 0); default the problem's."""
    lv = p.levels
    u = lv.uids
    src = u["3"].src                       # Rels$srcuid, sorted
    r3src = lv.rels3["srcuid"]             # Rels3$srcuid
    vec = r.reals if all_double else r.ints
    # (Rels1 targets, Rels2 sources) of the six getUidsCountsLocations calls, R/ProcessPaths.R:218-256
    cl_in = {"1a": (u["1a"].src, u["1a"].src), "1b": (u["1b"].src, u["1b"].src), "2": (u["2"].src, src),
             "3": (u["3"].trg, src), "4": (u["4"].trg, src), "5": (u["5"].trg, r3src)}
    double_signs = {"1a", "1b", "4", "5"}
    args = []
    for k in LEVELS:
        args += [vec(u[k].src), vec(u[k].trg), count_loc_list(r, *cl_in[k]),
                 r.reals(u[k].signs) if (k in double_signs or all_double) else r.ints(u[k].signs)]
    args += [r.reals(lv.data_inds[k]) for k in ("1a", "1b", "2", "3")]
    pc = p.perm_cases if perm_cases is None else np.asarray(perm_cases)
    if pc.size == 0:
        pc_obj = r.real_matrix(np.zeros((0, 0)))      # matrix(0, 0, 0): a 0 x 0 double matrix
    else:
        pc_obj = r.real_matrix(pc) if all_double else r.int_matrix(pc)
    args += [r.real_matrix(p.data1) if all_double else r.int_matrix(p.data1),
             r.real_matrix(p.data2) if all_double else r.int_matrix(p.data2),
             r.real_matrix(p.value_table),
             r.reals([p.n_cases]), r.reals([p.n_ctrls]), r.reals([p.top_k]), r.reals([p.iterations]), pc_obj,
             r.string(p.method if method is None else method), r.reals([p.path_length]), r.reals([nthreads])]
    assert len(args) == 39
    return args
