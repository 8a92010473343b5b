"""The whole .Call road on the GPU (pytest -m gpu, real MI355X): _geneticsCRE_ProcessPaths called through the stand-in R
runtime of tests/r_mock with the 39 arguments built as R builds them (tests/r_call.py: doubles where R passes doubles,
named count/location lists, column-major matrices) and GCRE_HIP_LIB pointing at the real libgcre_hip.so.  The five lists
against the CPU oracle, bit for bit.  The runtime is our reading of "Writing R Extensions", not R."""
import dataclasses
import os

import numpy as np
import pytest

import oracle
from geneticscre_amd import api
from geneticscre_amd.synth import make_problem
from helpers import small_table
from r_call import INTSXP, REALSXP, RMock, process_paths_args

pytestmark = pytest.mark.gpu

PP = "_geneticsCRE_ProcessPaths"


@pytest.fixture(scope="module")
def r():
    """A copy of shim + runtime of its own (the host tests bind theirs to the recording backend), bound to the real library
    at its first call."""
    api.load_library()
    rm = RMock(tag="_gpu")
    old = os.environ.get("GCRE_HIP_LIB")
    os.environ["GCRE_HIP_LIB"] = api.lib_path()
    try:   # getRels3 resolves the backend (load_abi); the shim keeps the handle
        rm.call("_geneticsCRE_getRels3", [rm.ints([0]), rm.ints([1]), rm.ints([1]), rm.named_list([("1", rm.reals([0, -1]))])])
    finally:
        if old is None:
            del os.environ["GCRE_HIP_LIB"]
        else:
            os.environ["GCRE_HIP_LIB"] = old
    return rm


def assert_lists_equal_oracle(out, want, path_length):
    assert out.names == ["lst1", "lst2", "lst3", "lst4", "lst5"]
    for lvl in range(1, 6):
        lst = out.value[lvl - 1]
        if lvl > path_length:
            assert lst is None, f"lst{lvl} above path_length must be NULL"
            continue
        w = want[f"lst{lvl}"]
        m = len(w.scores)
        assert lst.names == ["scores", "ids", "TestScores", "cases", "controls", "debug"]
        np.testing.assert_array_equal(lst["scores"].value.view(np.uint64), w.scores.view(np.uint64), err_msg=f"lst{lvl}")
        ids = lst["ids"]
        assert ids.type == INTSXP and ids.dim == [m, 2]
        np.testing.assert_array_equal(ids.matrix()[:, 0], w.src.astype(np.int64) + 1, err_msg=f"lst{lvl}")
        np.testing.assert_array_equal(ids.matrix()[:, 1], w.trg.astype(np.int64) + 1, err_msg=f"lst{lvl}")
        assert lst["TestScores"].type == REALSXP
        np.testing.assert_array_equal(lst["TestScores"].value.view(np.uint64), w.null.astype(np.float64).view(np.uint64),
                                      err_msg=f"lst{lvl}")
        assert lst["cases"].type == REALSXP and lst["controls"].type == REALSXP
        np.testing.assert_array_equal(lst["cases"].value, w.cases.astype(np.float64))
        np.testing.assert_array_equal(lst["controls"].value, w.ctrls.astype(np.float64))
        assert lst["debug"].value == [f"[debug] {a}:{b} {c}/{d}" for a, b, c, d in
                                      zip(w.src.tolist(), w.trg.tolist(), w.cases.tolist(), w.ctrls.tolist())]


@pytest.mark.parametrize("patients", [(33, 41), (65, 65)])      # two mask words, ragged; three words
@pytest.mark.parametrize("path_length", [3, 5])
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_dot_call_process_paths_equals_the_oracle(r, method, path_length, patients, monkeypatch):
    """K = 130 with 130, 50 (rows reused) and 200 (truncated: the column-major `used < nrow` road) label rows, K = 0 with
    matrix(0, 0, 0); GCRE_DEVICES unset, "0,0", and "0,0,0" capped to one device by nthreads = 1: the same lists every time."""
    nc, nt = patients
    genes, edges = (70, 260) if path_length == 5 else (45, 130)
    base = make_problem(genes, edges, nc, nt, 200, path_length, method=method, top_k=11, seed=21, table=small_table(nc, nt, 5))
    rows = base.perm_cases
    device_settings = [(None, -1), ("0,0", -1), ("0,0,0", 1)]          # (GCRE_DEVICES, nthreads)
    for K, pc in [(130, rows[:130]), (130, rows[:50]), (130, rows), (0, np.zeros((0, 0), np.int32))]:
        p = dataclasses.replace(base, iterations=K, perm_cases=pc)
        want = oracle.process_paths(p, order="canonical")
        for env, nthreads in device_settings:
            if env is None:
                monkeypatch.delenv("GCRE_DEVICES", raising=False)
            else:
                monkeypatch.setenv("GCRE_DEVICES", env)
            r.reset()
            out = r.call(PP, process_paths_args(r, p, nthreads=nthreads))
            assert r.protect_depth() == 0
            assert_lists_equal_oracle(out, want, path_length)
            for lvl in range(1, path_length + 1):
                assert len(out.value[lvl - 1]["TestScores"].value) == K
