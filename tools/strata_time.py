"""Time of the stratified set scores (gcre_score_sets_strata: k_strata_masks, k_strata_check, k_strata_rows, k_strata_observed,
k_strata_null) beside k_set_null on the same sets in the same run.

    python tools/strata_time.py [--what call] [--methods 1,2] [--strata 2,4] [--runs N] [--perms 100000]

The geometry: 25,000 + 25,000 patients, a pool of 2,000 gene rows carried by 0.8 % to 6 % of the patients; 1,000 paths of 3 to 5
genes and 100 sets of 200 genes; 100,000 permutations drawn inside S strata of equal size (patient q is of stratum q mod S), every
stratum with the library's value table of its own cases and controls.
  call       N calls of the C entry after a warm-up (packed rows: the wall time of the library call, gcre_score_sets' own stage
             for the records included), and N calls of gcre_score_sets on the same context
  kernel     a warm-up and one call of each, for a run of its own under rocprofv3 --kernel-trace --stats
  reference  report.strata_reference on a slice (the first paths and the first set of 200, a few permutations) at the full
             geometry: equal to the device's numbers
  fuzz       tests/test_gpu_strata.test_seeded_fuzz's loop for --cases cases: one summary line
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
os.environ.setdefault("GCRE_QUIET", "1")
import numpy as np  # noqa: E402

from geneticscre_amd import api, report  # noqa: E402

N_CASES, N_CTRLS, N_ROWS = 25000, 25000, 2000
PATHS, LARGE = 1000, (100, 200)
SEED = 5


def problem():
    """(packed rows uint64 [N_ROWS][W], sets, signs): rows of 1 / 16 to 1 / 128 carriers (the AND of 4 to 7 random words)."""
    rng = np.random.default_rng(19)
    n = N_CASES + N_CTRLS
    W = (n + 63) // 64
    packed = np.full((N_ROWS, W), 0xFFFFFFFFFFFFFFFF, np.uint64)
    depth = rng.integers(4, 8, N_ROWS)
    for k in range(7):
        r = rng.integers(0, 2**64, size=(N_ROWS, W), dtype=np.uint64)
        packed &= np.where((depth > k)[:, None], r, np.uint64(0xFFFFFFFFFFFFFFFF))
    packed[:, -1] &= np.uint64((1 << (n % 64)) - 1) if n % 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    sets = [rng.choice(N_ROWS, size=int(rng.integers(3, 6)), replace=False).tolist() for _ in range(PATHS)]
    sets += [rng.choice(N_ROWS, size=LARGE[1], replace=False).tolist() for _ in range(LARGE[0])]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    return packed, sets, signs


def strata_of(S: int) -> np.ndarray:
    return (np.arange(N_CASES + N_CTRLS) % S).astype(np.int32)


_TABLES: dict = {}


def stratum_tables(strata: np.ndarray):
    """The library's value table of every stratum's own cases and controls (one per size, kept for the run)."""
    S = int(strata.max()) + 1
    sizes = [(int((strata[:N_CASES] == s).sum()), int((strata[N_CASES:] == s).sum())) for s in range(S)]
    for sz in sizes:
        if sz not in _TABLES:
            _TABLES[sz] = api.values_table(*sz)
    return [_TABLES[sz] for sz in sizes]


class Caller:
    """gcre_score_sets_strata and gcre_score_sets on packed rows, as a C caller reaches them, on one context whose masks keep
    the strata."""

    def __init__(self, method, packed, sets, signs, perms, strata, tables):
        self.ex = api.JoinExec(method, N_CASES, N_CTRLS, perms)
        self.ex.set_value_table(tables[0])                    # (only gcre_score_sets' own records read it; smaller than the cohort)
        if perms:
            self.ex.generate_permutations(SEED, strata)
        self.lib = api._strata_lib()
        self.packed = packed
        self.K = perms
        self.S = len(sets)
        self.off = np.zeros(self.S + 1, np.int64)
        self.off[1:] = np.cumsum([len(s) for s in sets])
        self.members = np.ascontiguousarray(np.concatenate(sets), np.int32)
        self.sg = np.ascontiguousarray(np.concatenate(signs), np.int32)
        self.inp = api.gcre_set_input(self.S, api._ptr(self.off), api._ptr(self.members), api._ptr(self.sg), api._ptr(self.packed),
                                      self.packed.shape[0], N_CASES + N_CTRLS)
        self.strata = np.ascontiguousarray(strata, np.int32)
        self.NS = int(strata.max()) + 1
        self.nrow = np.array([t.shape[0] for t in tables], np.int32)
        self.ncol = np.array([t.shape[1] for t in tables], np.int32)
        self.toff = np.concatenate([[0], np.cumsum([t.size for t in tables])[:-1]]).astype(np.int64)
        self.flat = np.ascontiguousarray(np.concatenate([t.reshape(-1) for t in tables]))

    def strata_call(self, null=False, family=True):
        out = np.zeros(self.S, api.SET_SCORE)
        sr = np.zeros(self.S, api.STRATA_SCORE)
        fam = np.zeros(max(self.K, 1), np.float64) if family else None
        nul = np.zeros((self.S, max(self.K, 1)), np.float64) if null else None
        n_out = ctypes.c_int64(0)
        rc = self.lib.gcre_score_sets_strata(self.ex._h, ctypes.byref(self.inp), api._ptr(self.strata), self.NS, api._ptr(self.flat),
                                             api._ptr(self.nrow), api._ptr(self.ncol), api._ptr(self.toff), api._ptr(out), self.S,
                                             ctypes.byref(n_out), api._ptr(sr), None, None, api._ptr(nul), api._ptr(fam))
        if rc != api.GCRE_OK:
            raise api.GcreError(self.ex._lib.gcre_last_error(self.ex._h).decode())
        return out, sr, fam, nul

    def score_sets(self):
        out = np.zeros(self.S, api.SET_SCORE)
        n_out = ctypes.c_int64(0)
        rc = api._sets_lib().gcre_score_sets(self.ex._h, ctypes.byref(self.inp), api._ptr(out), self.S, ctypes.byref(n_out), None)
        if rc != api.GCRE_OK:
            raise api.GcreError(self.ex._lib.gcre_last_error(self.ex._h).decode())
        return out


def shape(method: int, S: int, perms: int) -> dict:
    w32p = 2 * (((N_CASES + N_CTRLS + 63) // 64 + 3) // 4 * 4)
    sets = PATHS + LARGE[0]
    return {"tool": "strata_time", "method": method, "strata": S, "n_cases": N_CASES, "n_ctrls": N_CTRLS, "pool_rows": N_ROWS, "paths": PATHS,
            "sets": list(LARGE), "perms": perms, "stratum_row_bytes": sets * S * method * w32p * 4,
            "rows_kernel_bytes": sets * method * w32p * 4 * (1 + S) + S * w32p * 4}


def call(method, S, runs, perms, prob) -> None:
    strata = strata_of(S)
    t0 = time.perf_counter()
    tables = stratum_tables(strata)
    table_s = time.perf_counter() - t0
    c = Caller(method, *prob, perms, strata, tables)
    c.strata_call()                                              # warm-up: code objects
    ms, ps = [], []
    before = c.ex.strata_launches()
    for _ in range(runs):
        t0 = time.perf_counter()
        rec, sr, fam, _ = c.strata_call()
        ms.append((time.perf_counter() - t0) * 1e3)
    launches = (c.ex.strata_launches() - before) // runs
    c.score_sets()
    for _ in range(runs):
        t0 = time.perf_counter()
        plain = c.score_sets()
        ps.append((time.perf_counter() - t0) * 1e3)
    c.ex.close()
    assert (sr["n_ge"] >= 0).all() and (sr["n_ge"] <= perms).all() and rec.tobytes() == plain.tobytes()
    line = shape(method, S, perms)
    line.update({"what": "call", "tables_host_s": round(table_s, 1), "call_ms": [round(t, 2) for t in ms],
                 "call_median_ms": round(float(np.median(ms)), 2), "launches_per_call": launches,
                 "score_sets_ms": [round(t, 2) for t in ps], "score_sets_median_ms": round(float(np.median(ps)), 2),
                 "median_stratified_p": float(np.median(sr["n_ge"] / max(perms, 1))), "median_pooled_p": float(np.median(plain["pvalue"]))})
    print(json.dumps(line), flush=True)


def kernel(method, S, perms, prob) -> None:
    strata = strata_of(S)
    c = Caller(method, *prob, perms, strata, stratum_tables(strata))
    c.strata_call()
    c.strata_call()
    c.score_sets()
    c.ex.close()
    line = shape(method, S, perms)
    line["what"] = "kernel"
    print(json.dumps(line), flush=True)


def reference(method, S, prob) -> None:
    """The first 3 paths and the first set of 200, 8 permutations: the definition on unpacked rows, against the device's."""
    packed, sets, signs = prob
    n = N_CASES + N_CTRLS
    keep = [0, 1, 2, PATHS]
    K = 8
    strata = strata_of(S)
    tables = stratum_tables(strata)
    c = Caller(method, packed, [sets[s] for s in keep], [signs[s] for s in keep], K, strata, tables)
    rec, sr, fam, nul = c.strata_call(null=True)
    c.ex.close()
    t0 = time.perf_counter()
    rows = np.unique(np.concatenate([np.asarray(sets[s]) for s in keep]))
    dense = np.unpackbits(packed[rows].view(np.uint8), axis=1, bitorder="little")[:, :n]
    lists = [np.searchsorted(rows, np.asarray(sets[s])).tolist() for s in keep]
    masks = report.permutation_masks(N_CASES, N_CTRLS, K, SEED, strata)
    ref = report.strata_reference(lists, dense, [signs[s] for s in keep], N_CASES, strata, tables, masks, method)
    sec = time.perf_counter() - t0
    assert np.array_equal(ref["score"].view(np.uint64), sr["score"].view(np.uint64)) and np.array_equal(ref["n_ge"], sr["n_ge"])
    assert np.array_equal(ref["null_scores"].view(np.uint64), nul.view(np.uint64))
    line = shape(method, S, K)
    line.update({"what": "reference", "slice_sets": keep, "slice_perms": K, "slice_seconds": round(sec, 2), "equal_to_device": True})
    print(json.dumps(line), flush=True)


def fuzz(cases: int) -> None:
    import subprocess
    t0 = time.perf_counter()
    env = dict(os.environ, GCRE_STRATA_FUZZ_CASES=str(cases))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_strata.py"),
                        "-k", "test_seeded_fuzz"], env=env, capture_output=True, text=True)
    summary = [ln for ln in r.stdout.splitlines() if ln.startswith("strata fuzz:")]
    print(json.dumps({"tool": "strata_time", "what": "fuzz", "cases": cases, "exit": r.returncode, "summary": summary,
                      "seconds": round(time.perf_counter() - t0, 1)}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="call")
    ap.add_argument("--methods", default="1,2")
    ap.add_argument("--strata", default="2,4")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--perms", type=int, default=100000)
    ap.add_argument("--cases", type=int, default=200)
    a = ap.parse_args()
    methods = [int(m) for m in a.methods.split(",") if m]
    strata = [int(s) for s in a.strata.split(",") if s]
    items = [w for w in a.what.split(",") if w]
    prob = problem() if set(items) & {"call", "kernel", "reference"} else None
    for what in items:
        if what == "fuzz":
            fuzz(a.cases)
            continue
        for m in methods:
            for S in strata:
                if what == "call":
                    call(m, S, a.runs, a.perms, prob)
                elif what == "kernel":
                    kernel(m, S, a.perms, prob)
                elif what == "reference":
                    reference(m, S, prob)
                else:
                    raise SystemExit(f"unknown item {what!r}")


if __name__ == "__main__":
    main()
