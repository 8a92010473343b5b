"""Time of the weighted sequential p-values (gcre_score_sets_sequential_weighted: k_seq_weighted_search,
k_seq_weighted_write, k_seq_null, k_seq_retire) beside what it joins: the uniform sequential call and the
resident road through gcre_generate_weighted_masks.

    python tools/seq_weighted_time.py --what call [--strata 1,4] [--methods 1] [--runs N] [--hits H] [--max-perms P]

The geometry and the sets are tools/sequential_time.py's (25,000 + 25,000 patients, 1,000 five-gene paths plus 100 sets of 200
genes); the odds and the strata tools/weighted_time.py's (``report.case_odds`` on two Gaussian covariates; patient q is of
stratum q mod S).  GCRE_SEQ_STATS is set: the library writes the batches and the active count behind every batch to stderr,
one line per call.
  call       a warm-up and N weighted calls and N uniform calls with --hits and --max-perms in one process: the wall time of
             each library call, how many sets stopped, the permutations used, the batches
  resident   once: a context that holds --max-perms permutations, generate_weighted_permutations, gcre_score_sets -- the road
             the weighted sequential call replaces; the hits of every set that did not stop must equal its n_ge
  search     for a run of its own under rocprofv3 --kernel-trace --stats: --runs times generate_weighted_permutations on a
             context of --perms permutations (k_weighted_search), and --runs weighted sequential calls in which nothing stops
             (hits above max_perms = --perms), so that k_seq_weighted_search draws the same permutations with the same odds
  first      for a run under rocprofv3: three weighted calls of one batch (max_perms = 4,096, nothing stops)
  stats      --dir D --label L: the *_kernel_stats.csv files below D as rows of one csv with a leading "Run" column
  fuzz       tests/test_gpu_seq_weighted.fuzz_case for --cases cases: one summary line
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
import weighted_time as wt  # noqa: E402

SEED = st.SEED


class Caller(st.Caller):
    """gcre_score_sets_sequential_weighted on packed rows, as a C caller reaches it (no packing in the time)."""

    def __init__(self, ex, packed, sets, signs, odds, strata):
        super().__init__(ex, packed, sets, signs)
        self.wlib = api._feature_lib("sequential_weighted")
        self.odds = np.ascontiguousarray(odds, np.float64)
        self.strata = None if strata is None else np.ascontiguousarray(strata, np.int32)
        self.n_strata = 0 if strata is None else int(self.strata.max()) + 1

    def weighted(self, hits, max_perms):
        out, seq = np.zeros(self.S, api.SET_SCORE), np.zeros(self.S, api.SEQ_SCORE)
        n_out = ctypes.c_int64(0)
        self.check(self.wlib.gcre_score_sets_sequential_weighted(self.ex._h, ctypes.byref(self.inp), SEED, api._ptr(self.odds),
                                                                 api._ptr(self.strata), self.n_strata, 1 << 20, int(hits), int(max_perms),
                                                                 api._ptr(out), self.S, ctypes.byref(n_out), api._ptr(seq)))
        return out, seq


def shape(method, sets, S) -> dict:
    line = st.shape(method, sets)
    line.update({"tool": "seq_weighted_time", "strata": S, "odds": "fitted"})
    return line


def summary(seq, ms, launches, per_batch) -> dict:
    stopped = seq["stopped"] != 0
    return {"call_ms": [round(t, 2) for t in ms], "call_median_ms": round(float(np.median(ms)), 2), "batches": launches // per_batch,
            "stopped": int(stopped.sum()), "not_stopped": int((~stopped).sum()), "perms_used_total": int(seq["n_perm"].sum()),
            "perms_used_median": int(np.median(seq["n_perm"])), "smallest_p": float((seq["n_hit"] / seq["n_perm"]).min())}


def call(method, S, runs, hits, max_perms, prob) -> None:
    packed, sets, signs = prob
    odds, strata = wt.inputs(st.N_CASES, st.N_CTRLS, S, "fitted")
    ex = st.context(method)
    c = Caller(ex, packed, sets, signs, odds, strata)
    c.weighted(1, 512)                                                                  # warm-up: code objects
    c.sequential(1, 512)
    line = shape(method, sets, S)
    line.update({"what": "call", "hits": hits, "max_perms": max_perms})
    for name, fn, per_batch in (("weighted", c.weighted, 4), ("uniform", c.sequential, 3)):
        ms = []
        before = ex.sequential_launches()
        for _ in range(runs):
            t0 = time.perf_counter()
            rec, seq = fn(hits, max_perms)
            ms.append((time.perf_counter() - t0) * 1e3)
        line[name] = summary(seq, ms, (ex.sequential_launches() - before) // runs, per_batch)
    ex.close()
    print(json.dumps(line), flush=True)


def resident(method, S, hits, max_perms, prob) -> None:
    packed, sets, signs = prob
    odds, strata = wt.inputs(st.N_CASES, st.N_CTRLS, S, "fitted")
    t0 = time.perf_counter()
    full = api.JoinExec(method, st.N_CASES, st.N_CTRLS, max_perms)
    full.set_value_table(st.corner())
    t1 = time.perf_counter()
    full.generate_weighted_permutations(SEED, odds, strata)
    t2 = time.perf_counter()
    cf = Caller(full, packed, sets, signs, odds, strata)
    want = cf.plain()
    t3 = time.perf_counter()
    rec, seq = cf.weighted(hits, max_perms)
    full.close()
    stopped = seq["stopped"] != 0
    assert np.array_equal(want["n_ge"][~stopped], seq["n_hit"][~stopped]) and (want["n_ge"][stopped] >= hits).all()
    line = shape(method, sets, S)
    line.update({"what": "resident", "perms": max_perms, "context_s": round(t1 - t0, 3), "generate_weighted_s": round(t2 - t1, 3),
                 "score_sets_s": round(t3 - t2, 3), "road_s": round(t3 - t0, 3), "hits_equal_n_ge_where_not_stopped": True,
                 "not_stopped": int((~stopped).sum())})
    print(json.dumps(line), flush=True)


def search(method, S, runs, perms, prob) -> None:
    packed, sets, signs = prob
    odds, strata = wt.inputs(st.N_CASES, st.N_CTRLS, S, "fitted")
    full = api.JoinExec(method, st.N_CASES, st.N_CTRLS, perms)
    full.set_value_table(st.corner())
    few = (sets[0][:17], sets[1][:sets[0][16]])
    c = Caller(full, packed, few, signs[:sets[0][16]], odds, strata)
    ms_w, ms_s = [], []
    for _ in range(runs):                                                               # alternating: the same machine state for both
        t0 = time.perf_counter()
        full.generate_weighted_permutations(SEED, odds, strata)
        ms_w.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        rec, seq = c.weighted(1 << 30, perms)
        ms_s.append((time.perf_counter() - t0) * 1e3)
    assert not seq["stopped"].any()
    full.close()
    line = shape(method, sets, S)
    line.update({"what": "search", "perms": perms, "runs": runs, "generate_weighted_ms": [round(t, 1) for t in ms_w],
                 "weighted_sequential_ms": [round(t, 1) for t in ms_s], "pairs": perms * S})
    print(json.dumps(line), flush=True)


def first(method, S, prob) -> None:
    packed, sets, signs = prob
    odds, strata = wt.inputs(st.N_CASES, st.N_CTRLS, S, "fitted")
    ex = st.context(method)
    c = Caller(ex, packed, sets, signs, odds, strata)
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        c.weighted(1 << 30, 4096)
        ms.append((time.perf_counter() - t0) * 1e3)
    ex.close()
    line = shape(method, sets, S)
    line.update({"what": "first", "perms": 4096, "call_ms": [round(t, 2) for t in ms]})
    print(json.dumps(line), flush=True)


def fuzz(cases: int) -> None:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_seq_weighted as T
    t0 = time.perf_counter()
    sets = stopped = 0
    for i in range(cases):
        what, bad, ref = T.fuzz_case(i)
        if bad is not None:
            raise SystemExit(f"{what}: {bad}")
        sets += int((ref["n_hit"] >= 0).sum())
        stopped += int(ref["stopped"].sum())
    print(json.dumps({"tool": "seq_weighted_time", "what": "fuzz", "cases": cases, "valid_sets": sets, "stopped": stopped, "failures": 0,
                      "seconds": round(time.perf_counter() - t0, 1)}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="call")
    ap.add_argument("--methods", default="1")
    ap.add_argument("--strata", default="1,4")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--hits", type=int, default=20)
    ap.add_argument("--max-perms", type=int, default=10**6)
    ap.add_argument("--perms", type=int, default=100000)
    ap.add_argument("--cases", type=int, default=200)
    ap.add_argument("--dir", default=".")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="seq_weighted_kernel_stats.csv")
    a = ap.parse_args()
    items = [w for w in a.what.split(",") if w]
    prob = st.problem() if set(items) & {"call", "resident", "search", "first"} else None
    for what in items:
        if what == "fuzz":
            fuzz(a.cases)
            continue
        if what == "stats":
            st.stats(a.dir, a.label, a.out)
            continue
        for m in [int(x) for x in a.methods.split(",") if x]:
            for S in [int(x) for x in a.strata.split(",") if x]:
                if what == "call":
                    call(m, S, a.runs, a.hits, a.max_perms, prob)
                elif what == "resident":
                    resident(m, S, a.hits, a.max_perms, prob)
                elif what == "search":
                    search(m, S, a.runs, a.perms, prob)
                elif what == "first":
                    first(m, S, prob)
                else:
                    raise SystemExit(f"unknown item {what!r}")


if __name__ == "__main__":
    main()
