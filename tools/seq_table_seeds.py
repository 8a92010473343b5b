#!/usr/bin/env python3
"""Finds the SEQ_TABLE_CASES of tests/helpers.py on the CPU: for every sequential entry, table family, variant and method the
first (table seed, trial of make_input) for which the numpy definitions alone hold what tests/test_seq_tables_host.py asks of
that family (``asked``), at 5 hits and 3,000 permutations.  Then, per entry, one case gets a max_perms at which one of its
sets stops exactly -- taken from the stop positions beyond the first 512-permutation batch, the case still holding what its
family asks -- and one case is replaced by the first seed and trial in which a set stops on a multiple of the 512-permutation
batch, so that over the entry's cases every class of ``test_gpu_sequential.classes_of`` is met.  It prints the dict and, per
entry and method, what the union of the cases still lacks of ``asked_of_all``.  No GPU needed.

    python tools/seq_table_seeds.py [seeds] [trials]
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import helpers  # noqa: E402
import test_seq_tables_host as h  # noqa: E402
import test_gpu_sequential as t  # noqa: E402


def holds(entry, family, method, spec):
    c = h.build(entry, family, method, spec)
    got = h.provoked(c)
    h._BUILT.clear()
    return all(got[name] for name in h.asked(entry, family, spec[1], method)), c


def search(entry, family, variant, method, seeds, trials):
    for trial in range(trials):
        for seed in range(seeds):
            spec = (seed, variant, trial, h.P_MAX)
            if holds(entry, family, method, spec)[0]:
                return spec
    return None


def with_a_stop_at_max_perms(entry, found):
    """One case of the entry cut at a set's own stop position; returns (key, index, spec) or None."""
    for (e, family, method), specs in found.items():
        if e != entry:
            continue
        for i, spec in enumerate(specs):
            _, c = holds(entry, family, method, spec)
            at = sorted({int(x) for x, s, v in zip(c.ref["n_perm"], c.ref["stopped"], c.valid) if v and s and x > h.CAP and x % h.CAP},
                        reverse=True)
            for max_perms in at:
                cut = spec[:3] + (max_perms,)
                ok, cc = holds(entry, family, method, cut)
                if ok and t.classes_of(cc.ref, cc.valid, max_perms, h.CAP)["stopped at max_perms"] > 0:
                    return (e, family, method), i, cut
    return None


def with_a_stop_on_a_batch_end(entry, found, seeds, trials):
    """A case of the entry, from any seed and trial, in which a set stops on a multiple of the batch: (key, index, spec)."""
    for trial in range(trials):
        for seed in range(seeds):
            for (e, family, method), specs in found.items():
                if e != entry:
                    continue
                for i, old in enumerate(specs):
                    if old[3] != h.P_MAX:
                        continue                                       # (the case cut at a stop position stays)
                    spec = (seed, old[1], trial, h.P_MAX)
                    ok, c = holds(entry, family, method, spec)
                    if ok and t.classes_of(c.ref, c.valid, h.P_MAX, h.CAP)["stopped on the last permutation of a batch"] > 0:
                        return (e, family, method), i, spec
    return None


def main():
    seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    trials = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    found = {}
    for entry in helpers.SEQ_ENTRIES:
        for family in h.FAMILIES:
            for method in h.METHODS:
                specs = []
                for variant in h.variants_of(entry, family, method):
                    spec = search(entry, family, variant, method, seeds, trials)
                    if spec is None:
                        print(f"# {(entry, family, method)} variant {variant}: nothing in {seeds} seeds x {trials} trials", flush=True)
                        continue
                    specs.append(spec)
                if specs:
                    found[(entry, family, method)] = specs
        hit = with_a_stop_at_max_perms(entry, found)
        if hit is None:
            print(f"# {entry}: no case with a set that stops at max_perms", flush=True)
        else:
            key, i, cut = hit
            found[key][i] = cut
        hit = with_a_stop_on_a_batch_end(entry, found, seeds, 10 * trials)
        if hit is None:
            print(f"# {entry}: no case with a set that stops on the last permutation of a batch", flush=True)
        else:
            key, i, spec = hit
            found[key][i] = spec
    print("SEQ_TABLE_CASES = {")
    for key, specs in found.items():
        print(f"    {key}: {specs},")
    print("}")
    for entry in helpers.SEQ_ENTRIES:
        for method in h.METHODS:
            union = {}
            for (e, family, m), specs in found.items():
                if e == entry and m == method:
                    for spec in specs:
                        for name, v in h.provoked(h.build(entry, family, method, spec)).items():
                            union[name] = union.get(name, False) or v
                        h._BUILT.clear()
            print(f"# {entry} method {method}: the union lacks {[n for n in h.asked_of_all(entry, method) if not union.get(n)]}")


if __name__ == "__main__":
    main()
