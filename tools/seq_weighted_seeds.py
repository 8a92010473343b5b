#!/usr/bin/env python3
"""Finds the constants of tests/test_gpu_seq_weighted.py on the CPU, from the numpy reference alone (the thresholds are the
library's host code; no GPU needed):

* CLASS_CASES -- for every configuration the first trial of ``make_input`` and a max_perms for which a set falls into every
  class of ``classes_of`` (as tools/sequential_seeds.py finds them for the uniform call), nothing is left over, and the accepted
  attempts hold even ones, odd ones and one >= 8;
* LEFT_OVER -- for the six-patient cohort a (seed, max_attempts, max_perms, hits) whose first left-over permutation R lies
  behind the first 512-permutation batch, inside a batch and not on its edge, with every early set stopped in front of R and
  the set planted on the cases still active there, under both methods;
* LEFT_AT_ZERO, LEFT_AT_ZERO_ONE -- seeds whose permutation 0 is left over, at the smallest max_attempts the estimate admits.

    python tools/seq_weighted_seeds.py [trials [method,cases,controls,strata]]
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from geneticscre_amd import api, report  # noqa: E402
import test_gpu_sequential as t  # noqa: E402
import test_gpu_seq_weighted as w  # noqa: E402


def search(config, trials):
    method, nc, nt, ns = config
    for trial in range(trials):
        rows, sets, signs, strata, odds, VT, obs, null, valid, att = w.problem(method, nc, nt, ns, trial)
        w._NULLS.clear()
        far = report.weighted_sequential_reference(null, obs, valid, w.HITS, w.P_MAX, att)
        if far["first_left_over"] is not None:
            continue
        at = sorted({int(x) for x, s in zip(far["n_perm"], far["stopped"]) if s and x > w.CAP and x % w.CAP}, reverse=True)
        for max_perms in at:
            ref = report.weighted_sequential_reference(null, obs, valid, w.HITS, max_perms, att)
            found = t.classes_of(ref, valid, max_perms, w.CAP)
            a = att[:max_perms]
            if all(v > 0 for v in found.values()) and (a % 2 == 0).any() and (a % 2 == 1).any() and (a >= 8).any():
                return trial, max_perms, found
    return None


def left_over(seeds, max_perms=3000):
    """... and, so that the cut batch itself retires a set, an early set that stops behind permutation 512."""
    rows, early, esigns, planted = w.six_patients()
    both, bsigns = early + [planted], esigns + [[1]]
    for cap, hits in ((c, h) for c in range(14, 22) for h in (200, 150, 250)):
        for seed in range(seeds):
            ok = True
            for method in (1, 2):
                _, ref, _ = w.six_reference(method, early, esigns, rows, w.SIX, seed, cap, hits, max_perms)
                R = ref["first_left_over"]
                if R is None or not 512 < R < max_perms or R % 512 == 0 or ref["refused"] or ref["n_perm"][0] != hits or \
                        not (ref["n_perm"] > 512).any():
                    ok = False
                    break
                _, bref, _ = w.six_reference(method, both, bsigns, rows, w.SIX, seed, cap, hits, max_perms)
                if not (bref["refused"] and bref["n_active"] == 1 and bref["stopped"][-1] == 0):
                    ok = False
                    break
            if ok:
                return seed, cap, max_perms, hits, R
    return None


def left_at_zero(odds, cap, seeds):
    thr, exp = api.weighted_thresholds(odds, 3, 3)
    assert exp[0] <= cap, exp
    for seed in range(seeds):
        _, att = report.weighted_masks(thr, 3, 3, 1, seed, max_attempts=cap)
        if att[0, 0] == report.WEIGHTED_NONE:
            return seed
    return None


def main():
    trials = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    only = tuple(int(x) for x in sys.argv[2].split(",")) if len(sys.argv) > 2 else None      # one configuration: "2,33,31,3"
    print("CLASS_CASES = {")
    for config in t.CONFIGS:
        if only is not None and config != only:
            continue
        hit = search(config, trials)
        if hit is None:
            print(f"    # {config}: nothing in {trials} trials")
            continue
        trial, max_perms, found = hit
        print(f"    {config}: ({trial}, {max_perms}),   # {found}")
    print("}")
    print("LEFT_OVER =", left_over(400), "  # (seed, max_attempts, max_perms, hits, R)")
    print("LEFT_AT_ZERO =", (left_at_zero(w.SIX, 3, 100), 3))
    print("LEFT_AT_ZERO_ONE =", left_at_zero(w.LEFT_ONE_ODDS, 1, 100))


if __name__ == "__main__":
    main()
