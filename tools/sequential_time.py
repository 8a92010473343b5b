"""Time of the sequential permutation p-values (gcre_score_sets_sequential: k_seq_masks, k_seq_null, k_seq_retire; DESIGN.md
§3.21) beside what it replaces.

    python tools/sequential_time.py [--what call] [--methods 1,2] [--runs N] [--hits H] [--max-perms P]

The geometry: 25,000 + 25,000 patients, a pool of 2,000 genes carried by 0.2 % to 2 % of the patients, 1,000 paths of five genes
plus 100 sets of 200 genes.  GCRE_SEQ_STATS is set: the library writes the number of batches and the active count behind every
batch to stderr, one line per call.
  call       N calls with --hits and --max-perms after a warm-up: the wall time of the library call, how many sets stopped, the
             permutations used; with --resident K also gcre_score_sets on a context that holds K permutations of the same
             seed (the fixed-K cost), whose n_ge must equal the hits of every set that did not stop when K = max_perms
  first      one batch with every set active (max_perms = 4,096) and gcre_score_sets on a context with as many permutations,
             three times each, for a run of its own under rocprofv3 --kernel-trace --stats (k_seq_null against k_set_null)
  masks      100,000 permutations with every set active to the end (hits above them) and subsample_tests with 100,000 draws,
             for a run under rocprofv3 (k_seq_masks against k_subsample_masks)
  stats      --dir D --label L: the *_kernel_stats.csv files below D as rows of one csv with a leading "Run" column
  fuzz       tests/test_gpu_sequential.fuzz_case for --cases cases: one summary line
--planted N adds N one-gene sets carried by 500 cases and no control: no permutation reaches them, they run to --max-perms.
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

N_CASES, N_CTRLS = 25000, 25000
POOL, N_PATHS, PATH_SIZE, N_BIG, BIG_SIZE = 2000, 1000, 5, 100, 200
SEED = 1


def problem(planted=0):
    """(packed rows uint64 [POOL][W], (off, members), signs): the paths first, then the large sets (tools/dose_time.py's); then
    ``planted`` one-gene sets whose gene is carried by 500 cases and no control: no permutation reaches them."""
    rng = np.random.default_rng(20)
    n = N_CASES + N_CTRLS
    rows = rng.random((POOL, n), dtype=np.float32) < rng.uniform(0.002, 0.02, size=(POOL, 1)).astype(np.float32)
    sets = [rng.choice(POOL, size=PATH_SIZE, replace=False).tolist() for _ in range(N_PATHS)]
    sets += [rng.choice(POOL, size=BIG_SIZE, replace=False).tolist() for _ in range(N_BIG)]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    if planted:
        extra = np.zeros((planted, n), bool)
        for k in range(planted):
            extra[k, 500 * k:500 * (k + 1)] = True
            sets.append([POOL + k])
            signs.append([1])
        rows = np.concatenate([rows, extra])
    off = np.zeros(len(sets) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in sets])
    return api.pack_carriers(rows, n), (off, np.concatenate(sets).astype(np.int32)), np.concatenate(signs).astype(np.int32)


def corner():
    from decorated_time import corner_table
    return corner_table(N_CASES, N_CTRLS, 6000)


def context(method, perms=0):
    ex = api.JoinExec(method, N_CASES, N_CTRLS, perms)
    ex.set_value_table(corner())
    if perms > 0:
        ex.generate_permutations(SEED)
    return ex


class Caller:
    """gcre_score_sets_sequential and gcre_score_sets on packed rows, as a C caller reaches them (no packing in the time)."""

    def __init__(self, ex, packed, sets, signs):
        self.ex, self.lib = ex, api._feature_lib("sequential")
        off, members = sets
        self.S = len(off) - 1
        self.keep = (np.ascontiguousarray(off, np.int64), np.ascontiguousarray(members, np.int32), np.ascontiguousarray(signs, np.int32), packed)
        self.inp = api.gcre_set_input(self.S, api._ptr(self.keep[0]), api._ptr(self.keep[1]), api._ptr(self.keep[2]), api._ptr(packed),
                                      packed.shape[0], N_CASES + N_CTRLS)

    def check(self, rc):
        if rc != api.GCRE_OK:
            raise api.GcreError(self.ex._lib.gcre_last_error(self.ex._h).decode())

    def sequential(self, hits, max_perms):
        out, seq = np.zeros(self.S, api.SET_SCORE), np.zeros(self.S, api.SEQ_SCORE)
        n_out = ctypes.c_int64(0)
        self.check(self.lib.gcre_score_sets_sequential(self.ex._h, ctypes.byref(self.inp), SEED, None, 0, int(hits), int(max_perms), api._ptr(out),
                                                       self.S, ctypes.byref(n_out), api._ptr(seq)))
        return out, seq

    def plain(self):
        out = np.zeros(self.S, api.SET_SCORE)
        n_out = ctypes.c_int64(0)
        self.check(self.lib.gcre_score_sets(self.ex._h, ctypes.byref(self.inp), api._ptr(out), self.S, ctypes.byref(n_out), None))
        return out


def shape(method, sets) -> dict:
    return {"tool": "sequential_time", "method": method, "n_cases": N_CASES, "n_ctrls": N_CTRLS, "sets": len(sets[0]) - 1,
            "members": int(len(sets[1]))}


def call(method, runs, hits, max_perms, resident, prob) -> None:
    packed, sets, signs = prob
    ex = context(method)
    c = Caller(ex, packed, sets, signs)
    c.sequential(1, 512)                                                                # warm-up: code objects
    ms = []
    before = ex.sequential_launches()
    for _ in range(runs):
        t0 = time.perf_counter()
        rec, seq = c.sequential(hits, max_perms)
        ms.append((time.perf_counter() - t0) * 1e3)
    launches = (ex.sequential_launches() - before) // runs
    ex.close()
    stopped = seq["stopped"] != 0
    line = shape(method, sets)
    line.update({"what": "call", "hits": hits, "max_perms": max_perms, "call_ms": [round(t, 2) for t in ms],
                 "call_median_ms": round(float(np.median(ms)), 2), "batches": launches // 3, "stopped": int(stopped.sum()),
                 "not_stopped": int((~stopped).sum()), "perms_used_total": int(seq["n_perm"].sum()),
                 "perms_used_median": int(np.median(seq["n_perm"])), "fixed_k_set_perms": int(len(seq)) * int(max_perms),
                 "smallest_p": float((seq["n_hit"] / seq["n_perm"]).min())})
    if resident > 0:
        full = context(method, resident)
        cf = Caller(full, packed, sets, signs)
        rs = []
        for _ in range(runs):
            t0 = time.perf_counter()
            want = cf.plain()
            rs.append((time.perf_counter() - t0) * 1e3)
        full.close()
        line.update({"resident_perms": resident, "resident_mask_gb": round(resident * 2 * ((N_CASES + N_CTRLS + 255) // 256 * 4) * 4 / 1e9, 2),
                     "score_sets_ms": [round(t, 2) for t in rs], "score_sets_median_ms": round(float(np.median(rs)), 2)})
        if resident == max_perms:
            assert np.array_equal(want["n_ge"][~stopped], seq["n_hit"][~stopped])
            assert (want["n_ge"][stopped] >= hits).all()
            line["hits_equal_n_ge_where_not_stopped"] = True
    print(json.dumps(line), flush=True)


def first(method, prob) -> None:
    packed, sets, signs = prob
    ex = context(method)
    c = Caller(ex, packed, sets, signs)
    for _ in range(3):
        c.sequential(1 << 30, 4096)
    ex.close()
    full = context(method, 4096)
    cf = Caller(full, packed, sets, signs)
    for _ in range(3):
        cf.plain()
    full.close()
    line = shape(method, sets)
    line.update({"what": "first", "perms": 4096})
    print(json.dumps(line), flush=True)


def masks(method, prob) -> None:
    packed, sets, signs = prob
    ex = context(method)
    few = (sets[0][:17], sets[1][:sets[0][16]])
    c = Caller(ex, packed, few, signs[:sets[0][16]])
    t0 = time.perf_counter()
    c.sequential(1 << 30, 100000)
    seq_s = time.perf_counter() - t0
    rows = np.unpackbits(packed.view(np.uint8), axis=1, bitorder="little")[:, :N_CASES + N_CTRLS]
    per_set = [signs[few[0][i]:few[0][i + 1]].tolist() for i in range(16)]
    t0 = time.perf_counter()
    ex.subsample_tests([few[1][few[0][i]:few[0][i + 1]].tolist() for i in range(16)], rows, per_set, draws=100000, seed=SEED, cuts=[1.0],
                       table_a=corner(), table_b=False)
    sub_s = time.perf_counter() - t0
    ex.close()
    line = shape(method, sets)
    line.update({"what": "masks", "perms": 100000, "mix64_per_call": 100000 * (N_CASES + N_CTRLS + 1),
                 "sequential_call_s": round(seq_s, 3), "subsample_call_s": round(sub_s, 3)})
    print(json.dumps(line), flush=True)


def fuzz(cases: int) -> None:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_sequential as T
    t0 = time.perf_counter()
    sets = stopped = 0
    for i in range(cases):
        what, bad, ref = T.fuzz_case(i)
        if bad is not None:
            raise SystemExit(f"{what}: {bad}")
        sets += int((ref["n_hit"] >= 0).sum())
        stopped += int(ref["stopped"].sum())
    print(json.dumps({"tool": "sequential_time", "what": "fuzz", "cases": cases, "valid_sets": sets, "stopped": stopped, "failures": 0,
                      "seconds": round(time.perf_counter() - t0, 1)}), flush=True)


def stats(directory: str, label: str, out: str) -> None:
    """The *_kernel_stats.csv files below ``directory`` as rows of one csv with a leading "Run" column (tools/dose_time.py's)."""
    import csv
    import glob
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
    print(json.dumps({"tool": "sequential_time", "what": "stats", "files": len(files), "out": out}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="call")
    ap.add_argument("--methods", default="1,2")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--hits", type=int, default=20)
    ap.add_argument("--max-perms", type=int, default=10**6)
    ap.add_argument("--resident", type=int, default=0)
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--planted", type=int, default=0)
    ap.add_argument("--dir", default=".")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="sequential_kernel_stats.csv")
    a = ap.parse_args()
    items = [w for w in a.what.split(",") if w]
    prob = problem(a.planted) if set(items) & {"call", "first", "masks"} else None
    for what in items:
        if what == "fuzz":
            fuzz(a.cases)
            continue
        if what == "stats":
            stats(a.dir, a.label, a.out)
            continue
        for m in [int(x) for x in a.methods.split(",") if x]:
            if what == "call":
                call(m, a.runs, a.hits, a.max_perms, a.resident, prob)
            elif what == "first":
                first(m, prob)
            elif what == "masks":
                masks(m, prob)
            else:
                raise SystemExit(f"unknown item {what!r}")


if __name__ == "__main__":
    main()
