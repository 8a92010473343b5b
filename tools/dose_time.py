"""Time of the multi-hit set tests (gcre_score_sets_dose: k_dose_rows, then the prefix stage's kernels) beside
what it replaces.

    python tools/dose_time.py [--what call] [--methods 1,2] [--runs N] [--perms K]

The geometry: 25,000 + 25,000 patients, 100,000 permutations, a pool of 2,000 genes carried by 0.2 % to 2 % of the patients,
1,000 paths of five genes plus 100 sets of 200 genes, levels 1, 2, 3, 4: 4,400 level rows.
  call       N calls of the C entry after a warm-up (packed rows: the wall time of the library call); in the same run
             gcre_score_sets on the 4,400 level sets written out by report.dose_sets (k_set_null on the same rows, and the
             host stage that uploads them), and the numpy definition on a slice -- dose_sets and family_tests(null=True) on the
             first ``--slice`` sets plus report.prefix_reference, equal to the call's numbers, its time scaled to all sets
  kernel     a warm-up, one call, one gcre_score_sets_prefix on the same sets with four cuts each (k_prefix_rows writes as
             many rows from the same members) and one gcre_score_sets on the level sets, for a run of its own under rocprofv3
             --kernel-trace --stats (k_dose_rows against k_prefix_rows and against its bytes, k_prefix_null against k_set_null)
  stats      --dir D --label L: the *_kernel_stats.csv files below D as rows of one csv with a leading "Run" column
  fuzz       tests/test_gpu_dose.test_seeded_fuzz for --cases cases: one summary line
One JSON line per item."""
from __future__ import annotations

import argparse
import csv
import ctypes
import glob
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
POOL, N_PATHS, PATH_SIZE, N_BIG, BIG_SIZE = 2000, 1000, 5, 100, 200
LEVELS = [1, 2, 3, 4]
HBM_TB_S = 8.0       # the device's peak: the bound of k_dose_rows is stated against it


def problem():
    """(packed rows uint64 [POOL][W], sets, signs, cuts): the paths first, then the large sets; ``cuts`` four per set, evenly
    spaced, for the prefix stage's builder on the same members."""
    rng = np.random.default_rng(20)
    n = N_CASES + N_CTRLS
    rows = rng.random((POOL, n), dtype=np.float32) < rng.uniform(0.002, 0.02, size=(POOL, 1)).astype(np.float32)
    sets = [rng.choice(POOL, size=PATH_SIZE, replace=False).tolist() for _ in range(N_PATHS)]
    sets += [rng.choice(POOL, size=BIG_SIZE, replace=False).tolist() for _ in range(N_BIG)]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    cuts = []
    for s in sets:
        c = np.zeros(len(s), np.uint8)
        c[[len(s) * (k + 1) // 4 - 1 for k in range(4)]] = 1
        if len(s) == PATH_SIZE:
            c[:] = [0, 1, 1, 1, 1]
        cuts.append(c.tolist())
    return api.pack_carriers(rows, n), sets, signs, cuts


class Caller:
    """gcre_score_sets_dose, gcre_score_sets_prefix and gcre_score_sets on packed rows, as a C caller reaches them."""

    def __init__(self, method, perms, packed):
        from decorated_time import corner_table
        self.ex = api.JoinExec(method, N_CASES, N_CTRLS, perms)
        self.ex.set_value_table(corner_table(N_CASES, N_CTRLS, 6000))
        self.ex.generate_permutations(1)
        self.lib = api._dose_lib()
        api._prefix_lib()
        self.packed = packed

    def lists(self, sets, signs, packed=None):
        packed = self.packed if packed is None else packed
        S = len(sets)
        off = np.zeros(S + 1, np.int64)
        off[1:] = np.cumsum([len(s) for s in sets])
        members = np.ascontiguousarray(np.concatenate(sets), np.int32)
        sg = np.ascontiguousarray(np.concatenate(signs), np.int32)
        inp = api.gcre_set_input(S, api._ptr(off), api._ptr(members), api._ptr(sg), api._ptr(packed), packed.shape[0], N_CASES + N_CTRLS)
        return S, inp, (off, members, sg, packed)

    def check(self, rc):
        if rc != api.GCRE_OK:
            raise api.GcreError(self.ex._lib.gcre_last_error(self.ex._h).decode())

    def dose(self, sets, signs, family=False):
        S, inp, keep = self.lists(sets, signs)
        out, ds = np.zeros(S, api.SET_SCORE), np.zeros(S, api.DOSE_SCORE)
        lv = np.asarray(LEVELS, np.int32)
        fam = np.zeros(self.ex.iters, np.float32) if family else None
        n_out = ctypes.c_int64(0)
        self.check(self.lib.gcre_score_sets_dose(self.ex._h, ctypes.byref(inp), api._ptr(lv), len(lv), api._ptr(out), S, ctypes.byref(n_out),
                                                 api._ptr(ds), api._ptr(fam), None, None))
        return out, ds, fam

    def prefix(self, sets, signs, cuts):
        S, inp, keep = self.lists(sets, signs)
        out, px = np.zeros(S, api.SET_SCORE), np.zeros(S, api.PREFIX_SCORE)
        ct = np.ascontiguousarray(np.concatenate(cuts), np.uint8)
        n_out = ctypes.c_int64(0)
        self.check(self.lib.gcre_score_sets_prefix(self.ex._h, ctypes.byref(inp), api._ptr(ct), api._ptr(out), S, ctypes.byref(n_out),
                                                   api._ptr(px), None, None, None))
        return out, px

    def plain(self, sets, signs, packed, family=False):
        S, inp, keep = self.lists(sets, signs, packed)
        out = np.zeros(S, api.SET_SCORE)
        fam = np.zeros(self.ex.iters, np.float32) if family else None
        n_out = ctypes.c_int64(0)
        self.check(self.lib.gcre_score_sets(self.ex._h, ctypes.byref(inp), api._ptr(out), S, ctypes.byref(n_out), api._ptr(fam)))
        return out, fam


def unpacked(packed):
    return np.unpackbits(packed.view(np.uint8), axis=1, bitorder="little")[:, :N_CASES + N_CTRLS]


def shape(method: int, perms: int, sets) -> dict:
    W = (N_CASES + N_CTRLS + 63) // 64
    w32p = 2 * ((W + 3) // 4 * 4)
    members = sum(len(s) for s in sets)
    rows = len(sets) * len(LEVELS)
    read, written = members * 2 * W * 4, rows * method * w32p * 4
    return {"tool": "dose_time", "method": method, "n_cases": N_CASES, "n_ctrls": N_CTRLS, "perms": perms, "sets": len(sets),
            "members": members, "levels": LEVELS, "level_rows": rows, "rows_read_bytes": read, "rows_written_bytes": written,
            "rows_bound_us": round((read + written) / (HBM_TB_S * 1e12) * 1e6, 1),
            "host_level_rows_mb": round(written / 1e6, 1), "null_matrix_gb": round(rows * perms * 4 / 1e9, 2)}


def level_sets(method, packed, sets, signs):
    """The level sets written out (report.dose_sets) and their rows, packed."""
    lrows, lsets, lsigns, owner = report.dose_sets(sets, unpacked(packed), signs, LEVELS, method == 2)
    return api.pack_carriers(lrows, N_CASES + N_CTRLS), lsets, lsigns, owner


def call(method, runs, perms, n_slice, prob) -> None:
    packed, sets, signs, cuts = prob
    c = Caller(method, perms, packed)
    c.dose(sets[:4], signs[:4])                                  # warm-up: code objects
    ms = []
    before = c.ex.dose_launches()
    for _ in range(runs):
        t0 = time.perf_counter()
        rec, ds, fam = c.dose(sets, signs, family=True)
        ms.append((time.perf_counter() - t0) * 1e3)
    launches = (c.ex.dose_launches() - before) // runs
    lpacked, lsets, lsigns, owner = level_sets(method, packed, sets, signs)
    c.plain(lsets[:4], lsigns[:4], lpacked)
    ems = []
    for _ in range(runs):
        t0 = time.perf_counter()
        srec, sfam = c.plain(lsets, lsigns, lpacked, family=True)
        ems.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(sfam.view(np.uint32), fam.view(np.uint32))          # the family maximum over the level sets, bit for bit
    L = len(LEVELS)
    best = np.array([np.nanargmax(srec["score"][s * L:s * L + L]) for s in range(len(sets))])
    assert np.array_equal(best, ds["best_index"])
    # the numpy definition on a slice: the level rows of the first sets, their null matrix, then numpy
    data = unpacked(packed)
    t0 = time.perf_counter()
    r2, s2, g2, o2 = report.dose_sets(sets[:n_slice], data, signs[:n_slice], LEVELS, method == 2)
    frec, _, null = c.ex.family_tests(s2, r2, g2, null=True)
    ref = report.prefix_reference(frec["score"], null, o2, n_slice, np.ones(n_slice, bool))
    sec = time.perf_counter() - t0
    assert np.array_equal(ref["n_ge"], ds["n_ge"][:n_slice]) and np.array_equal(ref["best_step"], ds["best_index"][:n_slice])
    assert np.array_equal(ref["score"].view(np.uint64), ds["score"][:n_slice].view(np.uint64))
    c.ex.close()
    line = shape(method, perms, sets)
    line.update({"what": "call", "call_ms": [round(t, 2) for t in ms], "call_median_ms": round(float(np.median(ms)), 2),
                 "launches_per_call": launches, "score_sets_on_level_sets_ms": [round(t, 2) for t in ems],
                 "score_sets_on_level_sets_median_ms": round(float(np.median(ems)), 2),
                 "definition_slice_sets": n_slice, "definition_slice_seconds": round(sec, 2), "definition_equal_to_device": True,
                 "definition_scaled_seconds": round(sec * len(sets) / n_slice, 1),
                 "best_level_counts": np.bincount(ds["best_level"], minlength=5)[1:5].tolist(),
                 "p_multi_hit_median": float(np.median(ds["n_ge"]) / perms), "p_nominal_median": float(np.median(rec["n_ge"]) / perms)})
    print(json.dumps(line), flush=True)


def kernel(method, perms, prob) -> None:
    packed, sets, signs, cuts = prob
    c = Caller(method, perms, packed)
    c.dose(sets[:4], signs[:4])
    c.dose(sets, signs, family=True)
    c.prefix(sets, signs, cuts)
    lpacked, lsets, lsigns, _ = level_sets(method, packed, sets, signs)
    c.plain(lsets, lsigns, lpacked, family=True)
    c.ex.close()
    line = shape(method, perms, sets)
    line["what"] = "kernel"
    print(json.dumps(line), flush=True)


def stats(directory: str, label: str, out: str) -> None:
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    new = not os.path.exists(out)
    with open(out, "a", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_ALL)
        for path in files:
            rows = list(csv.reader(open(path)))
            if new:
                w.writerow(["Run"] + rows[0])
                new = False
            for r in rows[1:]:
                w.writerow([label] + r)
    print(json.dumps({"tool": "dose_time", "what": "stats", "files": len(files), "out": out}), flush=True)


def fuzz(cases: int) -> None:
    import pytest
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_dose as T
    os.environ["GCRE_DOSE_FUZZ_CASES"] = str(cases)
    t0 = time.perf_counter()
    mp = pytest.MonkeyPatch()
    try:
        T.test_seeded_fuzz(mp)
    finally:
        mp.undo()
    print(json.dumps({"tool": "dose_time", "what": "fuzz", "cases": cases, "failures": 0,
                      "seconds": round(time.perf_counter() - t0, 1)}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="call")
    ap.add_argument("--methods", default="1,2")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--perms", type=int, default=PERMS)
    ap.add_argument("--slice", type=int, default=20)
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--dir", default=".")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="dose_kernel_stats.csv")
    a = ap.parse_args()
    items = [w for w in a.what.split(",") if w]
    prob = problem() if set(items) & {"call", "kernel"} else None
    for what in items:
        if what == "fuzz":
            fuzz(a.cases)
            continue
        if what == "stats":
            stats(a.dir, a.label, a.out)
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
