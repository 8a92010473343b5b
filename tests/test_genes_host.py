"""The per-gene best-path table, host side: the numpy definition (report.gene_best_reference) on a hand-worked join, the
slot tables (report.gene_tables) against the genes report.get_paths prints, the definition against the CPU oracle's
canonical top-k, the new C ABI names and the table checks that need no device.  No GPU needed."""
from __future__ import annotations

import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from geneticscre_amd import api, report, synth
from helpers import small_table

LEVELS = report.GENE_LEVELS          # the joins behind lst1 .. lst5


def test_reference_on_a_hand_worked_join():
    """Three uid rows join 2 + 1 + 3 = 6 paths.  Slots: 0 = A, 1 = B, 2 = C, 3 = D (D is on no row).

        ordinal  src  trg  genes0[src]  genes1[trg]  score
           0      0    4     A  B          C          2.5
           1      0    5     A  B          B  (twice)  7.0
           2      1    0     B  -          A          7.0   <- ties with ordinal 1
           3      2    1     C  -          -          1.0
           4      2    2     C  -          C  (twice)  9.0
           5      2    3     C  -          A          -inf  <- not a score

    A: paths 0, 1, 2 (5 does not count) -> 7.0 twice, the smaller ordinal 1.  B: 0, 1, 2 -> ordinal 1 again.
    C: 0, 3, 4 (5 does not count) -> 9.0 at ordinal 4.  D: nothing."""
    uids = SimpleNamespace(count=np.array([2, 1, 3], np.int32), location=np.array([4, 0, 1], np.int64))
    genes0 = np.array([[0, 1], [1, -1], [2, -1]], np.int32)
    genes1 = np.array([[0], [-1], [2], [0], [2], [1]], np.int32)
    scores = np.array([2.5, 7.0, 7.0, 1.0, 9.0, -np.inf])
    cases = np.array([10, 11, 12, 13, 14, 15], np.int32)
    ctrls = np.array([20, 21, 22, 23, 24, 25], np.int32)
    got = report.gene_best_reference(scores, cases, ctrls, uids, genes0, genes1, 4)
    assert got["score"].tolist() == [7.0, 7.0, 9.0, -np.inf]
    assert got["ordinal"].tolist() == [1, 1, 4, -1]
    assert got["src"].tolist() == [0, 0, 2, -1]
    assert got["trg"].tolist() == [5, 5, 2, -1]
    assert got["cases"].tolist() == [11, 11, 14, 0]
    assert got["ctrls"].tolist() == [21, 21, 24, 0]
    # a shard: only ordinals [2, 6) count.  A: path 2; B: path 2; C: path 4
    part = report.gene_best_reference(scores, cases, ctrls, uids, genes0, genes1, 4, shard=(2, 6))
    assert part["ordinal"].tolist() == [2, 2, 4, -1] and part["score"].tolist() == [7.0, 7.0, 9.0, -np.inf]
    # no genes0 table (levels 1 and 2): only genes1 counts.  A: paths 2 (5 is -inf); B: path 1; C: paths 0, 4
    only1 = report.gene_best_reference(scores, cases, ctrls, uids, None, genes1, 4)
    assert only1["ordinal"].tolist() == [2, 1, 4, -1]


def frames_of_synth(p):
    """The uid-valued frames get_paths indexes, for a synth problem: gene uid = rank in Ents; Ents2 = the source genes."""
    lv = p.levels
    rels = {"srcuid": lv.uids["3"].src, "trguid": lv.uids["3"].trg, "sign": lv.uids["3"].signs}
    return {"rels_data": {"srcuid": np.arange(len(p.data1))}, "rels_data2": {"srcuid": lv.uids["1b"].src}, "rels": rels,
            "rels3": lv.rels3}


PER_LEVEL = {1: ("rels_data2", "rels_data2"), 2: ("rels_data", "rels"), 3: ("rels", "rels"), 4: ("rels3", "rels"),
             5: ("rels3", "rels3")}


def joined_pairs(u):
    count = np.maximum(np.asarray(u.count, np.int64), 0)
    src = np.repeat(np.arange(len(count)), count)
    first = np.cumsum(count) - count
    trg = np.repeat(np.asarray(u.location, np.int64), count) + np.arange(count.sum()) - np.repeat(first, count)
    return src, trg


@pytest.mark.parametrize("seed", [3, 11])
def test_gene_tables_name_the_genes_get_paths_prints(seed):
    p = synth.make_problem(40, 110, 30, 34, 0, 5, seed=seed, table=small_table(64, 64, 1))
    n_genes, n_genes2 = len(p.data1), len(p.data2)
    tables = report.gene_tables(p.levels, n_genes, n_genes2)
    frames = frames_of_synth(p)
    ents2_uid = np.asarray(p.levels.uids["1b"].src)
    rng = np.random.default_rng(seed)
    for L, name in enumerate(LEVELS, start=1):
        src, trg = joined_pairs(p.levels.uids[name])
        assert len(src) > 0, name
        pick = rng.choice(len(src), size=min(len(src), 300), replace=False)
        ids = np.stack([src[pick] + 1, trg[pick] + 1], axis=1)
        f1, f2 = PER_LEVEL[L]
        paths, _ = report.get_paths(ids, L, frames[f1], frames[f2])
        g0, g1 = tables[name]
        api.check_gene_tables(report.gene_slots(name, n_genes, n_genes2), g0, g1, len(p.levels.uids[name].count), int(trg.max()))
        for k, i in enumerate(pick.tolist()):
            slots = set(g1[trg[i]].tolist()) | (set(g0[src[i]].tolist()) if g0 is not None else set())
            slots.discard(-1)
            uids = {int(ents2_uid[s]) for s in slots} if L == 1 else slots
            printed = {int(h) for h in paths[k].split(" -> ")}
            assert uids == printed, (name, i, uids, paths[k])
            assert len(paths[k].split(" -> ")) == L


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_reference_agrees_with_the_oracle_top_k(method):
    """Per level: the largest per-gene best IS the oracle's canonical best path (score bits, src, trg), and no top-k entry
    beats the best of a gene it runs through."""
    p = synth.make_problem(34, 80, 61, 70, 50, 5, method=method, top_k=9, seed=4242, table=small_table(131, 131, 8))
    want = oracle.process_paths(p, order="canonical")
    n_genes, n_genes2 = len(p.data1), len(p.data2)
    tables = report.gene_tables(p.levels, n_genes, n_genes2)
    for L, name in enumerate(LEVELS, start=1):
        r = want[f"lst{L}"]
        g0, g1 = tables[name]
        best = report.gene_best_reference(r.all_scores, r.all_cases, r.all_ctrls, p.levels.uids[name], g0, g1,
                                          report.gene_slots(name, n_genes, n_genes2))
        top = int(np.argmax(best["score"]))
        assert np.isfinite(best["score"][top])
        assert best["score"][top].view(np.uint64) == r.scores[-1].view(np.uint64), name
        # the canonical best path has the smallest ordinal among the paths of the largest score: every gene on it holds it
        a, b = int(r.src[-1]), int(r.trg[-1])
        on_it = set(g1[b].tolist()) | (set(g0[a].tolist()) if g0 is not None else set())
        on_it.discard(-1)
        assert on_it, name
        for g in on_it:
            assert (int(best["src"][g]), int(best["trg"][g])) == (a, b), (name, g)
            assert best["score"][g].view(np.uint64) == r.scores[-1].view(np.uint64)
            assert (int(best["cases"][g]), int(best["ctrls"][g])) == (int(r.cases[-1]), int(r.ctrls[-1]))
        for s, a, b in zip(r.scores.tolist(), r.src.tolist(), r.trg.tolist()):
            if a < 0:
                continue   # the sentinel of a level with fewer than top_k paths
            slots = set(g1[b].tolist()) | (set(g0[a].tolist()) if g0 is not None else set())
            slots.discard(-1)
            assert slots, name
            for g in slots:
                assert best["score"][g] >= s, (name, g)


def test_new_entry_points_are_declared_exported_and_abi_stays():
    names = ["gcre_gene_tally_create", "gcre_join_set_tally", "gcre_process_paths_set_tally", "gcre_gene_tally_read",
             "gcre_gene_tally_free"]
    for n in names:
        assert n in api.EXPORTS
    lib = api._genes_lib()
    assert lib.gcre_abi_version() == 4 and api.EXPECTED_ABI == 4
    out = subprocess.run(["nm", "-D", "--defined-only", api.lib_path()], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gcre_hip.h")).read()
    assert "#define GCRE_ABI_VERSION 4" in header


def test_bad_tables_are_refused_before_the_library_is_called():
    ok0 = np.array([[0, 1], [2, -1]], np.int32)
    ok1 = np.array([[3], [0], [1]], np.int32)
    g0, g1 = api.check_gene_tables(4, ok0, ok1, n_uids=2, max_loc=2)
    assert g0.dtype == np.int32 and g1.flags["C_CONTIGUOUS"]
    none0, same1 = api.check_gene_tables(4, None, ok1)
    assert none0 is None and np.array_equal(same1, ok1)
    with pytest.raises(api.GcreError, match="outside"):
        api.check_gene_tables(3, ok0, ok1)                       # slot 3 with 3 slots
    with pytest.raises(api.GcreError, match="outside"):
        api.check_gene_tables(4, np.array([[0, -2]], np.int32), ok1)
    with pytest.raises(api.GcreError, match="uid rows"):
        api.check_gene_tables(4, ok0, ok1, n_uids=3)             # wrong n_rows0
    with pytest.raises(api.GcreError, match="paths1 row"):
        api.check_gene_tables(4, ok0, ok1, n_uids=2, max_loc=3)  # the join reads a row the table lacks
    with pytest.raises(api.GcreError, match=r"\[rows\]"):
        api.check_gene_tables(4, np.zeros((2, 4), np.int32), ok1)   # four genes from one row
    with pytest.raises(api.GcreError, match=r"\[rows\]"):
        api.check_gene_tables(4, np.zeros(5, np.int32), ok1)
    with pytest.raises(api.GcreError, match="n_slots"):
        api.check_gene_tables(0, None, ok1)
    with pytest.raises(api.GcreError, match="integer"):
        api.check_gene_tables(4, ok0.astype(np.float64), ok1)
    # the several-device driver takes no tallies, and says so before it looks for a device
    with pytest.raises(api.GcreError, match="tallies"):
        api.process_paths_devices(None, devices=[0, 0], tallies={"2": object()})


def test_gene_summary_picks_one_row_per_gene():
    import pandas as pd
    df = pd.DataFrame({"Gene": ["A", "B", "A", "B", "C", "A"], "Lengths": [1, 1, 2, 2, 2, 3],
                       "Scores": [3.0, 5.0, 4.0, 5.0, 1.0, 4.0], "Pvalues": [0.5, 0.1, 0.2, 0.1, 0.9, 0.2],
                       "Cases": 0, "Controls": 0, "SignedPaths": "", "Paths": ""}, columns=report.GENE_COLUMNS)
    s = report.gene_summary(df)
    assert s["Gene"].tolist() == ["B", "A", "C"]
    assert s["Lengths"].tolist() == [1, 2, 2]            # B: equal p and score, the shorter; A: p 0.2, score 4.0, length 2 before 3
