#!/usr/bin/env python3
"""Finds the CLASS_CASES of tests/test_gpu_sequential.py on the CPU: for every configuration the first trial of its
``make_input`` and a max_perms for which the numpy reference alone puts at least one set into every class the batches can
treat differently -- stopped inside the first batch, in a later one, on the last permutation of a batch, at max_perms exactly;
never stopped with and without a hit.  max_perms is taken from the positions at which sets stop under a longer limit, and is
no multiple of the batch, so that the two boundary classes are met by different sets.  No GPU needed.

    python tools/sequential_seeds.py [trials]
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from geneticscre_amd import report  # noqa: E402
import test_gpu_sequential as t  # noqa: E402


def search(config, trials):
    method, nc, nt, ns = config
    for trial in range(trials):
        rows, sets, signs, strata, VT, obs, null, valid = t.problem(method, nc, nt, ns, trial)
        t._NULLS.clear()
        far = report.sequential_reference(null, obs, valid, t.HITS, t.P_MAX)
        at = sorted({int(x) for x, s in zip(far["n_perm"], far["stopped"]) if s and x > t.CAP and x % t.CAP}, reverse=True)
        for max_perms in at:
            ref = report.sequential_reference(null, obs, valid, t.HITS, max_perms)
            found = t.classes_of(ref, valid, max_perms, t.CAP)
            if all(v > 0 for v in found.values()):
                return trial, max_perms, found
    return None


def main():
    trials = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    print("CLASS_CASES = {")
    for config in t.CONFIGS:
        hit = search(config, trials)
        if hit is None:
            print(f"    # {config}: nothing in {trials} trials")
            continue
        trial, max_perms, found = hit
        print(f"    {config}: ({trial}, {max_perms}),   # {found}")
    print("}")


if __name__ == "__main__":
    main()
