"""Time of the split-half stability counts (gcre_score_sets_subsample: k_subsample_masks, k_subsample_null)
beside k_set_null on the same sets in the same run, and beside the bytes k_subsample_masks writes.

    python tools/subsample_time.py [--what call] [--methods 1,2] [--runs N] [--draws 100000]

The geometry: 25,000 + 25,000 patients, a pool of 2,000 gene rows carried by 0.8 % to 6 % of the patients; 1,000 paths of 3 to 5
genes and 100 sets of 200 genes; 100,000 draws of half the cases and half the controls, both halves scored, 2 cuts; and, for
k_set_null, 100,000 permutations on a context of its own.
  call       N calls of the C entry after a warm-up (packed rows: the wall time of the library call, gcre_score_sets' own stage
             for the records included), and N calls of gcre_score_sets with the permutations
  kernel     a warm-up and one call of each, for a run of its own under rocprofv3 --kernel-trace --stats
  split      four calls for such a trace: both halves / half A only, with the 2 cuts / without cuts -- what the second table's
             look-ups and the compares cost
  reference  report.subsample_reference on a slice (the first paths and the first set of 200, a few draws) at the full
             geometry: equal to the device's numbers for the same draws, and its time scaled to the whole problem
  fuzz       tests/test_gpu_subsample.fuzz_case for --cases cases against the reference: one summary line
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
M_CASES, M_CTRLS = N_CASES // 2, N_CTRLS // 2
PATHS, LARGE = 1000, (100, 200)
CUTS = (2.0, 4.0)
HBM_TB_S = 8.0


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


class Caller:
    """gcre_score_sets_subsample (perms == 0) or gcre_score_sets with permutations (perms > 0) on packed rows, as a C caller
    reaches them."""

    def __init__(self, method, packed, sets, signs, perms=0, tables=None):
        self.ex = api.JoinExec(method, N_CASES, N_CTRLS, perms)
        self.ex.set_value_table(tables["full"])
        if perms:
            self.ex.generate_permutations(5, None)
        self.lib = api._subsample_lib()
        self.packed = packed
        self.ta, self.tb = tables["a"], tables["b"]
        self.S = len(sets)
        self.off = np.zeros(self.S + 1, np.int64)
        self.off[1:] = np.cumsum([len(s) for s in sets])
        self.members = np.ascontiguousarray(np.concatenate(sets), np.int32)
        self.sg = np.ascontiguousarray(np.concatenate(signs), np.int32)
        self.inp = api.gcre_set_input(self.S, api._ptr(self.off), api._ptr(self.members), api._ptr(self.sg), api._ptr(self.packed),
                                      self.packed.shape[0], N_CASES + N_CTRLS)
        self.cuts = np.ascontiguousarray(np.tile(np.asarray(CUTS, np.float64), (self.S, 1)))

    def subsample(self, draws, seed=1, scores=False, half_b=True, cuts=True):
        out = np.zeros(self.S, api.SET_SCORE)
        cnt = [np.zeros((self.S, len(CUTS)), np.int64) if cuts and (h == 0 or half_b) else None for h in range(3)]
        sc = [np.zeros((self.S, draws), np.float64) if scores and (h == 0 or half_b) else None for h in range(2)]
        tb = self.tb if half_b else None
        n_out = ctypes.c_int64(0)
        rc = self.lib.gcre_score_sets_subsample(self.ex._h, ctypes.byref(self.inp), M_CASES, M_CTRLS, draws, seed, api._ptr(self.ta),
                                                self.ta.shape[0], self.ta.shape[1], api._ptr(tb), self.tb.shape[0], self.tb.shape[1],
                                                api._ptr(self.cuts) if cuts else None, len(CUTS) if cuts else 0, api._ptr(out), self.S,
                                                ctypes.byref(n_out), api._ptr(cnt[0]), api._ptr(cnt[1]), api._ptr(cnt[2]),
                                                api._ptr(sc[0]), api._ptr(sc[1]))
        if rc != api.GCRE_OK:
            raise api.GcreError(self.ex._lib.gcre_last_error(self.ex._h).decode())
        return out, cnt, sc

    def score_sets(self):
        out = np.zeros(self.S, api.SET_SCORE)
        n_out = ctypes.c_int64(0)
        rc = api._sets_lib().gcre_score_sets(self.ex._h, ctypes.byref(self.inp), api._ptr(out), self.S, ctypes.byref(n_out), None)
        if rc != api.GCRE_OK:
            raise api.GcreError(self.ex._lib.gcre_last_error(self.ex._h).decode())
        return out


def tables():
    return {"full": api.values_table(N_CASES, N_CTRLS), "a": api.values_table(M_CASES, M_CTRLS),
            "b": api.values_table(N_CASES - M_CASES, N_CTRLS - M_CTRLS)}


def shape(method: int, draws: int) -> dict:
    w32p = 2 * (((N_CASES + N_CTRLS + 63) // 64 + 3) // 4 * 4)
    kpad = (draws + 511) // 512 * 512
    mask_bytes = w32p * 4 * kpad
    return {"tool": "subsample_time", "method": method, "n_cases": N_CASES, "n_ctrls": N_CTRLS, "m_cases": M_CASES, "m_ctrls": M_CTRLS,
            "pool_rows": N_ROWS, "paths": PATHS, "sets": list(LARGE), "draws": draws, "cuts": list(CUTS), "mask_bytes": mask_bytes,
            "mask_write_bound_us": round(mask_bytes / (HBM_TB_S * 1e12) * 1e6, 1),
            "word_draw_pairs": (PATHS + LARGE[0]) * (2 if method == 2 else 1) * w32p * kpad}


def call(method, runs, draws, prob, tabs) -> None:
    c = Caller(method, *prob, tables=tabs)
    c.subsample(512)                                             # warm-up: code objects
    ms = []
    before = c.ex.subsample_launches()
    for _ in range(runs):
        t0 = time.perf_counter()
        rec, cnt, _ = c.subsample(draws)
        ms.append((time.perf_counter() - t0) * 1e3)
    launches = (c.ex.subsample_launches() - before) // runs
    t0 = time.perf_counter()
    c.subsample(0)
    base = (time.perf_counter() - t0) * 1e3                      # the same call without a draw: score_sets' own stages
    c.ex.close()
    assert all((x >= 0).all() and (x <= draws).all() for x in cnt) and (cnt[2] <= cnt[0]).all() and (cnt[2] <= cnt[1]).all()
    p = Caller(method, *prob, perms=draws, tables=tabs)
    p.score_sets()
    ps = []
    for _ in range(runs):
        t0 = time.perf_counter()
        p.score_sets()
        ps.append((time.perf_counter() - t0) * 1e3)
    p.ex.close()
    cols, per_half = report.stability_columns({"n_a": cnt[0], "n_b": cnt[1], "n_both": cnt[2]}, rec["valid"], draws)
    line = shape(method, draws)
    line.update({"what": "call", "call_ms": [round(t, 2) for t in ms], "call_median_ms": round(float(np.median(ms)), 2),
                 "call_without_draws_ms": round(base, 2), "launches_per_call": launches,
                 "score_sets_with_permutations_ms": [round(t, 2) for t in ps], "score_sets_median_ms": round(float(np.median(ps)), 2),
                 "per_half_selected": [round(float(x), 2) for x in per_half],
                 "stability_both_median": [float(np.median(cols[f"StabilityBoth.{j}"])) for j in range(len(CUTS))]})
    print(json.dumps(line), flush=True)


def kernel(method, draws, prob, tabs) -> None:
    c = Caller(method, *prob, tables=tabs)
    c.subsample(512)
    c.subsample(draws)
    c.ex.close()
    p = Caller(method, *prob, perms=draws, tables=tabs)
    p.score_sets()
    p.ex.close()
    line = shape(method, draws)
    line["what"] = "kernel"
    print(json.dumps(line), flush=True)


def split(method, draws, prob, tabs) -> None:
    """Where k_subsample_null's time goes, for a kernel trace: after the warm-up, the full call, then half A only, then both
    halves without cuts, then half A only without cuts -- four launches of the kernel at the full geometry, in this order."""
    c = Caller(method, *prob, tables=tabs)
    c.subsample(512)
    order = [(True, True), (False, True), (True, False), (False, False)]
    for half_b, cuts in order:
        c.subsample(draws, half_b=half_b, cuts=cuts)
    c.ex.close()
    line = shape(method, draws)
    line.update({"what": "split", "order": [{"half_b": h, "cuts": k} for h, k in order]})
    print(json.dumps(line), flush=True)


def reference(method, draws, prob, tabs) -> None:
    """The first 3 paths and the first set of 200, 8 draws: the definition on unpacked rows, against the device's scores."""
    packed, sets, signs = prob
    n = N_CASES + N_CTRLS
    keep = [0, 1, 2, PATHS]
    B = 8
    c = Caller(method, packed, sets, signs, tables=tabs)
    rec, cnt, sc = c.subsample(B, seed=3, scores=True)
    c.ex.close()
    t0 = time.perf_counter()
    rows = np.unique(np.concatenate([np.asarray(sets[s]) for s in keep]))
    dense = np.unpackbits(packed[rows].view(np.uint8), axis=1, bitorder="little")[:, :n]
    lists = [np.searchsorted(rows, np.asarray(sets[s])).tolist() for s in keep]
    ref = report.subsample_reference(lists, dense, [signs[s] for s in keep], N_CASES, M_CASES, M_CTRLS, B, 3, tabs["a"], tabs["b"],
                                     list(CUTS), method)
    sec = time.perf_counter() - t0
    for i, s in enumerate(keep):
        assert np.array_equal(ref["scores_a"][i].view(np.uint64), sc[0][s].view(np.uint64)), s
        assert np.array_equal(ref["scores_b"][i].view(np.uint64), sc[1][s].view(np.uint64)), s
        assert ref["n_a"][i].tolist() == cnt[0][s].tolist() and ref["n_both"][i].tolist() == cnt[2][s].tolist(), s
    pairs = len(keep) * B
    line = shape(method, draws)
    line.update({"what": "reference", "slice_sets": keep, "slice_draws": B, "slice_seconds": round(sec, 2), "equal_to_device": True,
                 "scaled_hours": round(sec / pairs * (PATHS + LARGE[0]) * draws / 3600.0, 1)})
    print(json.dumps(line), flush=True)


def fuzz(cases: int) -> None:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_subsample as T
    t0 = time.perf_counter()
    seen = {"method": set(), "slab": set(), "B": set(), "n": set(), "cuts": set(), "half_b": set(), "sets": set()}
    os.environ.pop("GCRE_SUBSAMPLE_MAX_MB", None)
    for case in range(cases):
        method, nc, nt, ma, mt, sets, rows, signs, TA, TB, cuts, B, slab, what = T.fuzz_case(case)
        os.environ.pop("GCRE_SUBSAMPLE_SLAB_DRAWS", None)
        if slab:
            os.environ["GCRE_SUBSAMPLE_SLAB_DRAWS"] = str(slab)
        ex = T.open_context(method, nc, nt, T.small_table(nc, nt, case))
        try:
            T.run_and_compare(ex, method, nc, sets, rows, signs, ma, mt, B, 1000 + case, TA, TB, cuts, what)
        finally:
            ex.close()
        for k, v in (("method", method), ("slab", slab), ("B", B), ("n", nc + nt), ("cuts", 0 if cuts is None else cuts.shape[1]),
                     ("half_b", TB is not False), ("sets", len(sets))):
            seen[k].add(v)
    os.environ.pop("GCRE_SUBSAMPLE_SLAB_DRAWS", None)
    print(json.dumps({"tool": "subsample_time", "what": "fuzz", "cases": cases, "failures": 0, "seconds": round(time.perf_counter() - t0, 1),
                      **{k: sorted(v) for k, v in seen.items()}}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="call")
    ap.add_argument("--methods", default="1,2")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--draws", type=int, default=100000)
    ap.add_argument("--cases", type=int, default=300)
    a = ap.parse_args()
    methods = [int(m) for m in a.methods.split(",") if m]
    items = [w for w in a.what.split(",") if w]
    full = set(items) & {"call", "kernel", "split", "reference"}
    prob = problem() if full else None
    tabs = tables() if full else None
    for what in items:
        if what == "fuzz":
            fuzz(a.cases)
            continue
        for m in methods:
            if what == "call":
                call(m, a.runs, a.draws, prob, tabs)
            elif what == "kernel":
                kernel(m, a.draws, prob, tabs)
            elif what == "split":
                split(m, a.draws, prob, tabs)
            elif what == "reference":
                reference(m, a.draws, prob, tabs)
            else:
                raise SystemExit(f"unknown item {what!r}")


if __name__ == "__main__":
    main()
