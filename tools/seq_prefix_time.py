"""Time of the sequential p-values of the two adaptive set tests (gcre_score_sets_prefix_sequential,
gcre_score_sets_dose_sequential: k_seq_prefix_null between the step rows and the batches) beside the
resident calls they extend.

    python tools/seq_prefix_time.py [--what call] [--methods 1,2] [--runs N] [--hits H] [--max-perms P] [--resident K]

GCRE_SEQ_STATS is set: the library writes the number of batches and the active count behind every batch to stderr, one line
per slab.
  call       the variable-threshold geometry: 25,000 + 25,000 patients, 200 sets of 50 genes, every gene a cut (10,000 step
             rows); a tenth of the genes lean towards the cases, so that some sets run far.  N calls with --hits and
             --max-perms after a warm-up: the wall time of the library call, how many sets stopped, the permutations used;
             with --resident K also gcre_score_sets_prefix on a context that holds K permutations of the same seed
  dose       the multi-hit geometry of tools/sequential_time.py (1,000 five-gene paths plus 100 sets of 200 genes), levels 1
             to 4, the same way against gcre_score_sets_dose
  first      one batch with every set active (max_perms = 4,096, hits above it) and gcre_score_sets_prefix on a context
             with as many permutations, three times each in turn, for a run of its own under rocprofv3 --kernel-trace
             --stats (k_seq_prefix_null against k_prefix_null on the same rows)
  stats      --dir D --label L: the *_kernel_stats.csv files below D as rows of one csv with a leading "Run" column
  fuzz       tests/test_gpu_seq_prefix.fuzz_case for --cases cases against the definition: one summary line
One JSON line per item."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("GCRE_QUIET", "1")
os.environ["GCRE_SEQ_STATS"] = "1"
import numpy as np  # noqa: E402

from geneticscre_amd import api  # noqa: E402
import sequential_time as st  # noqa: E402

N_CASES, N_CTRLS = st.N_CASES, st.N_CTRLS
POOL, N_SETS, SET_SIZE = 2000, 200, 50
LEVELS = (1, 2, 3, 4)
SEED = st.SEED


def prefix_problem():
    """(packed rows uint64 [POOL][W], (off, members), signs): 200 sets of 50 genes; a tenth of the genes are carried 1.6 times
    as often by the cases."""
    rng = np.random.default_rng(25)
    n = N_CASES + N_CTRLS
    freq = rng.uniform(0.002, 0.02, size=(POOL, 1)).astype(np.float32)
    lean = np.where(rng.random((POOL, 1)) < 0.1, 1.6, 1.0).astype(np.float32)
    rows = rng.random((POOL, n), dtype=np.float32) < np.where(np.arange(n)[None, :] < N_CASES, freq * lean, freq)
    sets = [rng.choice(POOL, size=SET_SIZE, replace=False).tolist() for _ in range(N_SETS)]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    off = np.zeros(len(sets) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in sets])
    return api.pack_carriers(rows, n), (off, np.concatenate(sets).astype(np.int32)), np.concatenate(signs).astype(np.int32)


class Caller:
    """The two sequential entries and the two resident ones on packed rows, as a C caller reaches them (no packing in the time)."""

    def __init__(self, ex, packed, sets, signs, dose):
        self.ex, self.lib, self.dose = ex, api._feature_lib("seq_prefix"), dose
        api._feature_lib("prefix")
        api._feature_lib("dose")
        off, members = sets
        self.S = len(off) - 1
        self.keep = (np.ascontiguousarray(off, np.int64), np.ascontiguousarray(members, np.int32), np.ascontiguousarray(signs, np.int32), packed)
        self.inp = api.gcre_set_input(self.S, api._ptr(self.keep[0]), api._ptr(self.keep[1]), api._ptr(self.keep[2]), api._ptr(packed),
                                      packed.shape[0], N_CASES + N_CTRLS)
        self.lv = np.array(LEVELS, np.int32)

    def check(self, rc):
        if rc != api.GCRE_OK:
            raise api.GcreError(self.ex._lib.gcre_last_error(self.ex._h).decode())

    def sequential(self, hits, max_perms):
        out, seq = np.zeros(self.S, api.SET_SCORE), np.zeros(self.S, api.SEQ_SCORE)
        n_out = ctypes.c_int64(0)
        if self.dose:
            rec = np.zeros(self.S, api.DOSE_SCORE)
            self.check(self.lib.gcre_score_sets_dose_sequential(self.ex._h, ctypes.byref(self.inp), api._ptr(self.lv), len(self.lv), SEED, None,
                                                                None, 0, 0, int(hits), int(max_perms), api._ptr(out), self.S,
                                                                ctypes.byref(n_out), api._ptr(rec), api._ptr(seq), None))
        else:
            rec = np.zeros(self.S, api.PREFIX_SCORE)
            self.check(self.lib.gcre_score_sets_prefix_sequential(self.ex._h, ctypes.byref(self.inp), None, SEED, None, None, 0, 0, int(hits),
                                                                  int(max_perms), api._ptr(out), self.S, ctypes.byref(n_out), api._ptr(rec),
                                                                  api._ptr(seq), None))
        return rec, seq

    def resident(self):
        out = np.zeros(self.S, api.SET_SCORE)
        n_out = ctypes.c_int64(0)
        if self.dose:
            rec = np.zeros(self.S, api.DOSE_SCORE)
            self.check(self.lib.gcre_score_sets_dose(self.ex._h, ctypes.byref(self.inp), api._ptr(self.lv), len(self.lv), api._ptr(out), self.S,
                                                     ctypes.byref(n_out), api._ptr(rec), None, None, None))
        else:
            rec = np.zeros(self.S, api.PREFIX_SCORE)
            self.check(self.lib.gcre_score_sets_prefix(self.ex._h, ctypes.byref(self.inp), None, api._ptr(out), self.S, ctypes.byref(n_out),
                                                       api._ptr(rec), None, None, None))
        return rec


def shape(what, method, sets, dose) -> dict:
    S = len(sets[0]) - 1
    return {"tool": "seq_prefix_time", "what": what, "method": method, "n_cases": N_CASES, "n_ctrls": N_CTRLS, "sets": S,
            "step_rows": S * len(LEVELS) if dose else int(len(sets[1]))}


def call(what, method, runs, hits, max_perms, resident, prob, dose) -> None:
    packed, sets, signs = prob
    ex = st.context(method)
    c = Caller(ex, packed, sets, signs, dose)
    c.sequential(1, 512)                                                                # warm-up: code objects
    ms = []
    before = ex.seq_prefix_launches()
    for _ in range(runs):
        t0 = time.perf_counter()
        rec, seq = c.sequential(hits, max_perms)
        ms.append((time.perf_counter() - t0) * 1e3)
    launches = (ex.seq_prefix_launches() - before) // runs
    ex.close()
    stopped = seq["stopped"] != 0
    line = shape(what, method, sets, dose)
    line.update({"hits": hits, "max_perms": max_perms, "call_ms": [round(t, 2) for t in ms], "call_median_ms": round(float(np.median(ms)), 2),
                 "batches": (launches - 3) // 3, "stopped": int(stopped.sum()), "not_stopped": int((~stopped).sum()),
                 "perms_used_total": int(seq["n_perm"].sum()), "perms_used_median": int(np.median(seq["n_perm"])),
                 "smallest_p": float((seq["n_hit"] / seq["n_perm"]).min())})
    for K in resident:
        full = st.context(method, K)
        cf = Caller(full, packed, sets, signs, dose)
        rs = []
        for _ in range(runs):
            t0 = time.perf_counter()
            want = cf.resident()
            rs.append((time.perf_counter() - t0) * 1e3)
        full.close()
        line[f"resident_{K}"] = {"mask_gb": round(K * 2 * ((N_CASES + N_CTRLS + 255) // 256 * 4) * 4 / 1e9, 2), "call_ms": [round(t, 2) for t in rs],
                                 "call_median_ms": round(float(np.median(rs)), 2)}
        if K == max_perms:
            assert np.array_equal(want["n_ge"][~stopped], seq["n_hit"][~stopped]) and (want["n_ge"][stopped] >= hits).all()
            line[f"resident_{K}"]["hits_equal_n_ge_where_not_stopped"] = True
    print(json.dumps(line), flush=True)


def first(method, prob) -> None:
    packed, sets, signs = prob
    ex = st.context(method)
    full = st.context(method, 4096)
    c, cf = Caller(ex, packed, sets, signs, False), Caller(full, packed, sets, signs, False)
    for _ in range(3):
        _, seq = c.sequential(1 << 30, 4096)
        want = cf.resident()
        assert np.array_equal(want["n_ge"], seq["n_hit"])
    ex.close()
    full.close()
    line = shape("first", method, sets, False)
    line.update({"perms": 4096, "hits_equal_n_ge": True})
    print(json.dumps(line), flush=True)


def fuzz(cases: int) -> None:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["GCRE_SEQ_PREFIX_FUZZ_CASES"] = str(cases)
    import pytest
    t0 = time.perf_counter()
    rc = pytest.main(["-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_seq_prefix.py"), "-k", "fuzz"])
    print(json.dumps({"tool": "seq_prefix_time", "what": "fuzz", "cases": cases, "failures": 0 if rc == 0 else "see above",
                      "seconds": round(time.perf_counter() - t0, 1)}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="call")
    ap.add_argument("--methods", default="1,2")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--hits", type=int, default=20)
    ap.add_argument("--max-perms", type=int, default=10**6)
    ap.add_argument("--resident", default="")
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--dir", default=".")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="seq_prefix_kernel_stats.csv")
    a = ap.parse_args()
    resident = [int(x) for x in a.resident.split(",") if x]
    for what in [w for w in a.what.split(",") if w]:
        if what == "fuzz":
            fuzz(a.cases)
            continue
        if what == "stats":
            st.stats(a.dir, a.label, a.out)
            continue
        prob = st.problem() if what == "dose" else prefix_problem()
        for m in [int(x) for x in a.methods.split(",") if x]:
            if what in ("call", "dose"):
                call(what, m, a.runs, a.hits, a.max_perms, resident, prob, what == "dose")
            elif what == "first":
                first(m, prob)
            else:
                raise SystemExit(f"unknown item {what!r}")


if __name__ == "__main__":
    main()
