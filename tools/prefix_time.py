"""Time of the variable-threshold set tests (gcre_score_sets_prefix: k_prefix_rows, k_prefix_pick, k_prefix_null; DESIGN.md
§3.18) beside what it replaces.

    python tools/prefix_time.py [--what call] [--methods 1,2] [--runs N] [--perms K]

The geometry: 25,000 + 25,000 patients, 100,000 permutations, a pool of 2,000 genes carried by 0.02 % to 0.2 % of the patients,
200 sets of 50 genes in ascending order of carrier total, every member a cut: 10,000 steps.
  call       N calls of the C entry after a warm-up (packed rows: the wall time of the library call); in the same run
             gcre_score_sets on the 10,000 step sets written out (the parent's k_set_null on the same rows, and the host stage
             that builds them), and the emulation on a slice -- family_tests(null=True) on the step sets of the first
             ``--slice`` sets plus the numpy maximum, equal to the call's numbers, its time scaled to the 200 sets
  kernel     a warm-up, one call and one gcre_score_sets on the step sets, for a run of its own under rocprofv3
             --kernel-trace --stats (k_prefix_null against k_set_null, k_prefix_rows against its bytes)
  fuzz       tests/test_gpu_prefix.test_seeded_fuzz for --cases cases: one summary line
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
import numpy as np  # noqa: E402

from geneticscre_amd import api, report  # noqa: E402

N_CASES, N_CTRLS, PERMS = 25000, 25000, 100000
POOL, N_SETS, SET_SIZE = 2000, 200, 50
HBM_TB_S = 8.0       # the device's peak: the bound of k_prefix_rows is stated against it


def problem():
    """(packed rows uint64 [POOL][W], sets, signs): every set's genes in ascending order of carrier total (ties by row)."""
    rng = np.random.default_rng(18)
    n = N_CASES + N_CTRLS
    rows = rng.random((POOL, n), dtype=np.float32) < rng.uniform(0.0002, 0.002, size=(POOL, 1)).astype(np.float32)
    tot = rows.sum(axis=1)
    sets = []
    for _ in range(N_SETS):
        g = np.sort(rng.choice(POOL, size=SET_SIZE, replace=False))
        sets.append(g[np.argsort(tot[g], kind="stable")].tolist())
    signs = [rng.choice([-1, 1], size=SET_SIZE).tolist() for _ in sets]
    return api.pack_carriers(rows, n), sets, signs


class Caller:
    """gcre_score_sets_prefix and gcre_score_sets on packed rows, as a C caller reaches them."""

    def __init__(self, method, perms, packed):
        from decorated_time import corner_table
        self.ex = api.JoinExec(method, N_CASES, N_CTRLS, perms)
        self.ex.set_value_table(corner_table(N_CASES, N_CTRLS, 6000))
        self.ex.generate_permutations(1)
        self.lib = api._prefix_lib()
        self.packed = packed

    def lists(self, sets, signs):
        S = len(sets)
        off = np.zeros(S + 1, np.int64)
        off[1:] = np.cumsum([len(s) for s in sets])
        members = np.ascontiguousarray(np.concatenate(sets), np.int32)
        sg = np.ascontiguousarray(np.concatenate(signs), np.int32)
        inp = api.gcre_set_input(S, api._ptr(off), api._ptr(members), api._ptr(sg), api._ptr(self.packed), self.packed.shape[0],
                                 N_CASES + N_CTRLS)
        return S, inp, (off, members, sg)

    def check(self, rc):
        if rc != api.GCRE_OK:
            raise api.GcreError(self.ex._lib.gcre_last_error(self.ex._h).decode())

    def prefix(self, sets, signs, family=False, null=False):
        S, inp, keep = self.lists(sets, signs)
        out, px = np.zeros(S, api.SET_SCORE), np.zeros(S, api.PREFIX_SCORE)
        fam = np.zeros(self.ex.iters, np.float32) if family else None
        nul = np.zeros((S, self.ex.iters), np.float32) if null else None
        n_out = ctypes.c_int64(0)
        self.check(self.lib.gcre_score_sets_prefix(self.ex._h, ctypes.byref(inp), None, api._ptr(out), S, ctypes.byref(n_out), api._ptr(px),
                                                   api._ptr(fam), api._ptr(nul), None))
        return out, px, fam, nul

    def plain(self, sets, signs, family=False):
        S, inp, keep = self.lists(sets, signs)
        out = np.zeros(S, api.SET_SCORE)
        fam = np.zeros(self.ex.iters, np.float32) if family else None
        n_out = ctypes.c_int64(0)
        self.check(self.lib.gcre_score_sets(self.ex._h, ctypes.byref(inp), api._ptr(out), S, ctypes.byref(n_out), api._ptr(fam)))
        return out, fam


def shape(method: int, perms: int) -> dict:
    W = (N_CASES + N_CTRLS + 63) // 64
    w32p = 2 * ((W + 3) // 4 * 4)
    steps = N_SETS * SET_SIZE
    read, written = steps * 2 * W * 4, steps * method * w32p * 4
    return {"tool": "prefix_time", "method": method, "n_cases": N_CASES, "n_ctrls": N_CTRLS, "perms": perms, "sets": N_SETS,
            "genes_per_set": SET_SIZE, "steps": steps, "rows_read_bytes": read, "rows_written_bytes": written,
            "rows_bound_us": round((read + written) / (HBM_TB_S * 1e12) * 1e6, 1),
            "host_union_rows_mb": round(steps * method * w32p * 4 / 1e6, 1), "null_matrix_gb": round(steps * perms * 4 / 1e9, 2)}


def call(method, runs, perms, n_slice, prob) -> None:
    packed, sets, signs = prob
    c = Caller(method, perms, packed)
    c.prefix(sets[:4], signs[:4])                                # warm-up: code objects
    ms = []
    before = c.ex.prefix_launches()
    for _ in range(runs):
        t0 = time.perf_counter()
        rec, px, fam, _ = c.prefix(sets, signs, family=True)
        ms.append((time.perf_counter() - t0) * 1e3)
    launches = (c.ex.prefix_launches() - before) // runs
    st, sg, owner = report.prefix_sets(sets, signs, None)
    c.plain(st[:4], sg[:4])
    ems = []
    for _ in range(runs):
        t0 = time.perf_counter()
        srec, sfam = c.plain(st, sg, family=True)
        ems.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(sfam.view(np.uint32), fam.view(np.uint32))          # the family maximum over the step sets, bit for bit
    # the emulation on a slice: the null matrix of the step sets of the first sets, then numpy
    k = int(owner.searchsorted(n_slice))
    t0 = time.perf_counter()
    frec, _, null = c.ex.family_tests(st[:k], np.unpackbits(packed.view(np.uint8), axis=1, bitorder="little")[:, :N_CASES + N_CTRLS],
                                      sg[:k], null=True)
    ref = report.prefix_reference(frec["score"], null, owner[:k], n_slice, np.ones(n_slice, bool))
    sec = time.perf_counter() - t0
    assert np.array_equal(ref["n_ge"], px["n_ge"][:n_slice]) and np.array_equal(ref["best_step"], px["best_step"][:n_slice])
    assert np.array_equal(ref["score"].view(np.uint64), px["score"][:n_slice].view(np.uint64))
    c.ex.close()
    line = shape(method, perms)
    line.update({"what": "call", "call_ms": [round(t, 2) for t in ms], "call_median_ms": round(float(np.median(ms)), 2),
                 "launches_per_call": launches, "score_sets_on_step_sets_ms": [round(t, 2) for t in ems],
                 "score_sets_on_step_sets_median_ms": round(float(np.median(ems)), 2),
                 "emulation_slice_sets": n_slice, "emulation_slice_seconds": round(sec, 2), "emulation_equal_to_device": True,
                 "emulation_scaled_seconds": round(sec * N_SETS / n_slice, 1),
                 "best_genes_median": float(np.median(px["best_members"])), "p_adaptive_median": float(np.median(px["n_ge"]) / perms),
                 "p_nominal_median": float(np.median(rec["n_ge"]) / perms)})
    print(json.dumps(line), flush=True)


def kernel(method, perms, prob) -> None:
    packed, sets, signs = prob
    c = Caller(method, perms, packed)
    c.prefix(sets[:4], signs[:4])
    c.prefix(sets, signs, family=True)
    st, sg, _ = report.prefix_sets(sets, signs, None)
    c.plain(st, sg, family=True)
    c.ex.close()
    line = shape(method, perms)
    line["what"] = "kernel"
    print(json.dumps(line), flush=True)


def fuzz(cases: int) -> None:
    import pytest
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_prefix as T
    os.environ["GCRE_PREFIX_FUZZ_CASES"] = str(cases)
    t0 = time.perf_counter()
    mp = pytest.MonkeyPatch()
    try:
        T.test_seeded_fuzz(mp)
    finally:
        mp.undo()
    print(json.dumps({"tool": "prefix_time", "what": "fuzz", "cases": cases, "failures": 0,
                      "seconds": round(time.perf_counter() - t0, 1)}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="call")
    ap.add_argument("--methods", default="1,2")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--perms", type=int, default=PERMS)
    ap.add_argument("--slice", type=int, default=10)
    ap.add_argument("--cases", type=int, default=300)
    a = ap.parse_args()
    items = [w for w in a.what.split(",") if w]
    prob = problem() if set(items) & {"call", "kernel"} else None
    for what in items:
        if what == "fuzz":
            fuzz(a.cases)
            continue
        for m in [int(x) for x in a.methods.split(",") if x]:
            if what == "call":
                call(m, a.runs, a.perms, a.slice, prob)
            elif what == "kernel":
                kernel(m, a.perms, prob)
            else:
                raise SystemExit(f"unknown item {what!r}")


if __name__ == "__main__":
    main()
