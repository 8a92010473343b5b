#!/usr/bin/env python3
"""Finds the CLASS_CASES of tests/test_gpu_seq_prefix.py on the CPU, in the manner of tools/sequential_seeds.py: for every
configuration -- statistic (prefix, dose), method, cohort, strata -- the first trial of its ``make_input`` and a max_perms for
which ``report.adaptive_sequential_reference`` alone puts at least one set into every class the batches can treat differently:
stopped inside the first batch, in a later one, on the last permutation of a batch, at max_perms exactly; never stopped with
and without a hit.  max_perms is taken from the positions at which sets stop under a longer limit, and is no multiple of the
batch, so that the two boundary classes are met by different sets and the last tile is partly live.  No GPU needed.

    python tools/seq_prefix_seeds.py [trials [processes]]
"""
from __future__ import annotations

import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_sequential as t  # noqa: E402
import test_gpu_seq_prefix as tp  # noqa: E402


def search(config, trials):
    for trial in range(trials):
        p = tp.problem(*config, trial)
        tp._NULLS.clear()
        valid = p[-1]
        far = tp.reference(p, t.HITS, t.P_MAX)
        at = sorted({int(x) for x, s in zip(far["n_perm"], far["stopped"]) if s and x > t.CAP and x % t.CAP}, reverse=True)
        for max_perms in at:
            found = t.classes_of(tp.reference(p, t.HITS, max_perms), valid, max_perms, t.CAP)
            if all(v > 0 for v in found.values()):
                return trial, max_perms, found
    return None


def _search(args):
    return search(*args)


def main():
    trials = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    procs = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    print("CLASS_CASES = {")
    with multiprocessing.Pool(procs) as pool:
        hits = pool.map(_search, [(config, trials) for config in tp.CONFIGS], chunksize=1)
    for config, hit in zip(tp.CONFIGS, hits):
        if hit is None:
            print(f"    # {config}: nothing in {trials} trials")
            continue
        trial, max_perms, found = hit
        print(f"    {config}: ({trial}, {max_perms}),   # {found}", flush=True)
    print("}")


if __name__ == "__main__":
    main()
