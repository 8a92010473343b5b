"""Time of the competitive set tests (gcre_score_sets_compete: k_compete_null) beside the bytes its random
row loads gather and the measured gather rates (tools/row_gather_rate.hip, profiles/r02_row_gather_rate.txt: 20 to 32 TB/s for
1-KB wave-loads of an L2-resident table).

    python tools/compete_time.py [--what call] [--methods 1,2] [--runs N] [--draws 10000]

The geometry: a pool of 17,000 gene rows at 25,000 + 25,000 patients (6,256 bytes a row, 106 MB: Infinity Cache, not L2),
carrier frequencies 0.8 % to 6 % in ten ``report.carrier_bins``; 1,000 sets of 5 genes and 100 sets of 200 genes; 10,000 draws.
  call       N calls of the C entry after a warm-up (packed rows: the wall time of the library call, upload of the pool included)
  kernel     a warm-up and one call, for a run of its own under rocprofv3 --kernel-trace --stats
  reference  report.competitive_reference on a slice (the first sets of both sizes, a few draws) at the full geometry: equal to
             the device's numbers for the same draws, and its time scaled to the whole problem
  fuzz       tests/test_gpu_compete.fuzz_case for --cases cases against the reference: one summary line
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

N_CASES, N_CTRLS, N_ROWS, N_BINS = 25000, 25000, 17000, 10
SMALL, LARGE = (1000, 5), (100, 200)
GATHER_TB_S = (20.0, 32.0)      # profiles/r02_row_gather_rate.txt


def problem():
    """(packed rows uint64 [N_ROWS][W], bins, sets, signs): rows of 1 / 16 to 1 / 128 carriers (the AND of 4 to 7 random words)."""
    rng = np.random.default_rng(17)
    n = N_CASES + N_CTRLS
    W = (n + 63) // 64
    packed = np.full((N_ROWS, W), 0xFFFFFFFFFFFFFFFF, np.uint64)
    depth = rng.integers(4, 8, N_ROWS)
    for k in range(7):
        r = rng.integers(0, 2**64, size=(N_ROWS, W), dtype=np.uint64)
        packed &= np.where((depth > k)[:, None], r, np.uint64(0xFFFFFFFFFFFFFFFF))
    packed[:, -1] &= np.uint64((1 << (n % 64)) - 1) if n % 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    tot = (np.bitwise_count(packed) if hasattr(np, "bitwise_count") else np.unpackbits(packed.view(np.uint8), axis=1)).sum(axis=1, dtype=np.int64)
    order = np.argsort(tot, kind="stable")
    bins = np.zeros(N_ROWS, np.int32)
    bins[order] = (np.arange(N_ROWS) * N_BINS // N_ROWS).astype(np.int32)
    sets = [rng.choice(N_ROWS, size=k, replace=False).tolist() for cnt, k in (SMALL, LARGE) for _ in range(cnt)]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    return packed, bins, sets, signs


class Caller:
    """gcre_score_sets_compete on packed rows, as a C caller reaches it."""

    def __init__(self, method, packed, bins, sets, signs):
        self.ex = api.JoinExec(method, N_CASES, N_CTRLS, 0)
        self.ex.set_value_table(api.values_table(N_CASES, N_CTRLS))
        self.lib = api._compete_lib()
        self.packed, self.bins = packed, np.ascontiguousarray(bins, np.int32)
        self.lists(sets, signs)

    def lists(self, sets, signs):
        self.S = len(sets)
        self.off = np.zeros(self.S + 1, np.int64)
        self.off[1:] = np.cumsum([len(s) for s in sets])
        self.members = np.ascontiguousarray(np.concatenate(sets), np.int32)
        self.sg = np.ascontiguousarray(np.concatenate(signs), np.int32)
        self.inp = api.gcre_set_input(self.S, api._ptr(self.off), api._ptr(self.members), api._ptr(self.sg), api._ptr(self.packed),
                                      self.packed.shape[0], N_CASES + N_CTRLS)

    def __call__(self, draws, seed=1, null=False):
        out = np.zeros(self.S, api.SET_SCORE)
        ge = np.zeros(self.S, np.int64)
        nul = np.zeros((self.S, draws), np.float64) if null else None
        n_out = ctypes.c_int64(0)
        rc = self.lib.gcre_score_sets_compete(self.ex._h, ctypes.byref(self.inp), api._ptr(self.bins), N_BINS, draws, seed, api._ptr(out),
                                              self.S, ctypes.byref(n_out), api._ptr(ge), api._ptr(nul), None)
        if rc != api.GCRE_OK:
            raise api.GcreError(self.ex._lib.gcre_last_error(self.ex._h).decode())
        return (out, ge, nul) if null else (out, ge)


def shape(method: int, draws: int) -> dict:
    row_bytes = ((N_CASES + N_CTRLS + 63) // 64 + 1) // 2 * 16
    rows = (SMALL[0] * SMALL[1] + LARGE[0] * LARGE[1]) * draws
    return {"tool": "compete_time", "method": method, "n_cases": N_CASES, "n_ctrls": N_CTRLS, "pool_rows": N_ROWS, "bins": N_BINS,
            "sets": [list(SMALL), list(LARGE)], "draws": draws, "row_bytes": row_bytes, "pool_mb": round(N_ROWS * row_bytes / 1e6, 1),
            "gathered_rows": rows, "gathered_bytes": rows * row_bytes,
            "gather_bound_us": [round(rows * row_bytes / (r * 1e12) * 1e6, 1) for r in GATHER_TB_S]}


def call(method, runs, draws, prob) -> None:
    c = Caller(method, *prob)
    c(16)                                                        # warm-up: code objects
    ms = []
    before = c.ex.compete_launches()
    for _ in range(runs):
        t0 = time.perf_counter()
        rec, ge = c(draws)
        ms.append((time.perf_counter() - t0) * 1e3)
    launches = (c.ex.compete_launches() - before) // runs
    t0 = time.perf_counter()
    c(0)
    base = (time.perf_counter() - t0) * 1e3                      # the same call without a draw: score_sets' own stages
    c.ex.close()
    assert (ge >= 0).all() and (ge <= draws).all()
    line = shape(method, draws)
    line.update({"what": "call", "call_ms": [round(t, 2) for t in ms], "call_median_ms": round(float(np.median(ms)), 2),
                 "call_without_draws_ms": round(base, 2), "launches_per_call": launches,
                 "p_small_median": float(np.median(ge[:SMALL[0]]) / draws), "p_large_median": float(np.median(ge[SMALL[0]:]) / draws)})
    print(json.dumps(line), flush=True)


def kernel(method, draws, prob) -> None:
    c = Caller(method, *prob)
    c(16)
    c(draws)
    c.ex.close()
    line = shape(method, draws)
    line["what"] = "kernel"
    print(json.dumps(line), flush=True)


def reference(method, draws, prob) -> None:
    """The first 3 sets of 5 and the first set of 200 (kept at their indices: the streams are keyed by them), 8 draws."""
    packed, bins, sets, signs = prob
    n = N_CASES + N_CTRLS
    keep = [0, 1, 2, SMALL[0]]
    B = 8
    c = Caller(method, packed, bins, sets, signs)
    rec, ge, nul = c(B, seed=3, null=True)
    c.ex.close()
    VT = api.values_table(N_CASES, N_CTRLS)
    t0 = time.perf_counter()
    used = 0
    bn, pools = report._compete_pools(bins, N_ROWS)
    for s in keep:      # competitive_reference's steps for set s at its own index, on the rows its draws touch
        pk = report._compete_draws(sets[s], bn, pools, s, np.arange(B), 3, 64)
        rows = np.unique(np.concatenate([pk.ravel(), np.asarray(sets[s])]))
        dense = np.unpackbits(packed[rows].view(np.uint8), axis=1, bitorder="little")[:, :n]
        lists = np.searchsorted(rows, np.vstack([np.asarray(sets[s])[None, :], pk])).tolist()
        sc = report.competitive_reference(lists, dense, [signs[s]] * (B + 1), None, 0, 3, N_CASES, VT, method)["obs"]
        assert sc[0] == rec["score"][s] and np.array_equal(sc[1:].view(np.uint64), nul[s].view(np.uint64)), s
        used += len(rows)
    sec = time.perf_counter() - t0
    rows = sum(len(sets[s]) for s in keep) * B
    line = shape(method, draws)
    line.update({"what": "reference", "slice_sets": keep, "slice_draws": B, "slice_rows": rows, "slice_seconds": round(sec, 2),
                 "equal_to_device": True, "scaled_hours": round(sec / rows * line["gathered_rows"] / 3600.0, 1), "rows_used": used})
    print(json.dumps(line), flush=True)


def fuzz(cases: int) -> None:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_compete as T
    t0 = time.perf_counter()
    seen = {"method": set(), "slab": set(), "attempts": set(), "B": set(), "n": set(), "largest_set": set()}
    os.environ.pop("GCRE_COMPETE_MAX_MB", None)
    for case in range(cases):
        method, nc, nt, sets, rows, signs, bins, VT, B, slab, attempts, what = T.fuzz_case(case)
        os.environ.pop("GCRE_COMPETE_SLAB_DRAWS", None)
        if slab:
            os.environ["GCRE_COMPETE_SLAB_DRAWS"] = str(slab)
        os.environ["GCRE_COMPETE_ATTEMPTS"] = str(attempts)
        ref = report.competitive_reference(sets, rows, signs, bins, B, 1000 + case, nc, VT, method, attempts=attempts)
        ex = T.open_context(method, nc, nt, VT)
        try:
            got = ex.competitive_tests(sets, rows, signs, bins=bins, draws=B, seed=1000 + case, null=True, picks=True)
            T.assert_equal_reference(got, ref, B, what)
        finally:
            ex.close()
        for k, v in (("method", method), ("slab", slab), ("attempts", attempts), ("B", B), ("n", nc + nt),
                     ("largest_set", max(len(s) for s in sets))):
            seen[k].add(v)
    os.environ.pop("GCRE_COMPETE_SLAB_DRAWS", None)
    os.environ.pop("GCRE_COMPETE_ATTEMPTS", None)
    print(json.dumps({"tool": "compete_time", "what": "fuzz", "cases": cases, "failures": 0, "seconds": round(time.perf_counter() - t0, 1),
                      **{k: sorted(v) for k, v in seen.items()}}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="call")
    ap.add_argument("--methods", default="1,2")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--draws", type=int, default=10000)
    ap.add_argument("--cases", type=int, default=300)
    a = ap.parse_args()
    methods = [int(m) for m in a.methods.split(",") if m]
    items = [w for w in a.what.split(",") if w]
    prob = problem() if set(items) & {"call", "kernel", "reference"} else None
    for what in items:
        if what == "fuzz":
            fuzz(a.cases)
            continue
        for m in methods:
            if what == "call":
                call(m, a.runs, a.draws, prob)
            elif what == "kernel":
                kernel(m, a.draws, prob)
            elif what == "reference":
                reference(m, a.draws, prob)
            else:
                raise SystemExit(f"unknown item {what!r}")


if __name__ == "__main__":
    main()
