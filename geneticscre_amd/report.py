"""What GWASPA does with the lists ProcessPaths returns, and the non-R front end around the device path.

  * ``get_paths``        id pairs -> "a -> b -> c" / "a (+) -> b (-) -> c (-)" strings  (R/PathMethods.R:2-131)
  * ``uid_to_symbol``    uid paths -> gene-symbol paths                                  (R/Utils.R:50-95)
  * ``results_table``    p-values, the GWASPA.Results columns and their order            (R/ProcessPaths.R:272-326)
  * ``preprocess_table`` / ``prepare_inputs``  the dataset and network filtering         (R/Utils.R:162-199, ProcessPaths.R:131-176)
  * ``decorated_table``  getDecoratedPvalues: the split-path table, permutations on the device  (R/DecoratedPvalue.R)
  * ``gwaspa``           the whole call, with the table / level tables / permutations built natively
  * ``score_paths``      permutation tests of paths and gene sets the caller names (k_set_null; beyond the reference)
  * ``check_best_paths`` checkBestPaths: rescore a GWASPA.Results table from the raw data   (R/CheckResults.R:2-89)
  * ``gene_tables`` / ``gene_best_reference`` / ``gene_results`` / ``gene_summary``  the per-gene best-path table: for
                         every gene the best path of each length through it, tallied on the device during the joins
                         (gcre_gene_tally; beyond the reference)
  * ``minp_reference`` / ``minp_columns``  Westfall-Young min-P over a family of given sets in plain numpy, and its columns
  * ``exceed_reference`` / ``fdr_columns``  null exceedance counts of a join in plain numpy, and the per-family error rate,
                         permutation FDR and q-values they give (gcre_exceed; beyond the reference)
  * ``false_count_columns``  k-FWER, the median and the (1 - alpha) bound of the number of false positives, from the same
                         counts kept per permutation
  * ``stepdown_reference`` / ``stepdown_columns``  step-down max-T p-values of a level's top rows: each row against the
                         null maxima of the paths that are not better rows (gcre_exceed_stepdown)
  * ``carrier_rows`` / ``overlap_reference`` / ``clump_rows`` / ``clump_paths``  which rows of a table are carried by the
                         same patients: pairwise carrier overlaps on the device (gcre_set_overlap), greedy clumping against
                         lead rows, and each row rescored without its lead's carriers (beyond the reference)

  * ``patient_counts_reference`` / ``patient_table``  who carries the findings: how many of a list of sets every patient
                         carries, per group of sets (gcre_set_patient_counts; beyond the reference)

  * ``burden_reference`` / ``burden_table`` / ``burden_test`` / ``replicate``  permutation p-values of per-patient loads:
                         do the cases carry more of a list of sets than the cases of a random relabelling -- gene-set
                         burden tests, replication in a second cohort (gcre_patient_burden)

  * ``subsample_masks`` / ``subsample_reference`` / ``stability_columns`` / ``stability_bound``  split-half stability: sets
                         scored on random halves of the cohort and on their complements, how often each half reaches a
                         cut-off (gcre_score_sets_subsample; beyond the reference)

  * ``permutation_masks`` / ``sequential_reference`` / ``sequential_columns``  sequential permutation p-values: the mask rule
                         of generate_permutations in numpy, every set stopped at its h-th exceedance
                         (gcre_score_sets_sequential; beyond the reference)

Host-side post-processing of <= top_k x 5 rows: string work, nothing here touches the scored path.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

POS, NEG = "(+)", "(-)"


def _next_dirs(prev: np.ndarray, sign: np.ndarray) -> np.ndarray:
    """dirs[j+1] from dirs[j] and the edge sign: (-) iff (sign==1 & prev (-)) | (sign==-1 & prev (+)); any other sign
    value leaves (+) (PathMethods.R:28-31 and its copies)."""
    neg = ((sign == 1) & prev) | ((sign == -1) & ~prev)
    return neg


def get_paths(ids: np.ndarray, path_length: int, rels1: Dict[str, np.ndarray], rels2: Dict[str, np.ndarray]
              ) -> Tuple[List[str], List[str]]:
    """getPaths (R/PathMethods.R:2-131).  ``ids`` is the 1-based [n][2] matrix of ``JoinResult.as_r_list()["ids"]``.

    rels1 / rels2 are the frames GWASPA passes per level (ProcessPaths.R:278-291): dicts with "srcuid" and, where the
    level needs them, "trguid", "sign", "trguid2", "sign2".  An id above nrow(rels2) names the sign-flipped copy
    of a path (the reference never emits one -- methods.h:245-247 is commented out -- but getPaths decodes it).
    Sentinel rows (ids (0,0), App. A-8) decode to "NA" the way R's out-of-range indexing does.
    """
    ids = np.asarray(ids, dtype=np.int64).reshape(-1, 2)
    i1, i2 = ids[:, 0] - 1, ids[:, 1] - 1
    n2 = len(rels2["srcuid"])
    pivot = len(rels1["srcuid"]) if path_length == 3 else n2           # PathMethods.R:43 uses nrow(Rels1)
    first_neg = ids[:, 1] > pivot
    i3 = np.where(ids[:, 1] > n2, i2 - n2, i2)

    def col(frame, name, idx):
        a = np.asarray(frame[name])
        ok = (idx >= 0) & (idx < len(a))
        out = np.where(ok, a[np.clip(idx, 0, max(len(a) - 1, 0))] if len(a) else 0, 0)
        return out, ok

    if path_length == 1:
        genes = [col(rels2, "srcuid", np.where(i2 >= n2, i2 - n2, i2))]
        signs = []
        first_neg = i2 >= n2
    elif path_length == 2:
        genes = [col(rels2, "srcuid", i3), col(rels2, "trguid", i3)]
        signs = [col(rels2, "sign", i3)]
    elif path_length == 3:
        genes = [col(rels1, "srcuid", i1), col(rels1, "trguid", i1), col(rels2, "trguid", i3)]
        signs = [col(rels1, "sign", i1), col(rels2, "sign", i3)]
    elif path_length == 4:
        genes = [col(rels1, "srcuid", i1), col(rels1, "trguid", i1), col(rels1, "trguid2", i1), col(rels2, "trguid", i3)]
        signs = [col(rels1, "sign", i1), col(rels1, "sign2", i1), col(rels2, "sign", i3)]
    elif path_length == 5:
        genes = [col(rels1, "srcuid", i1), col(rels1, "trguid", i1), col(rels1, "trguid2", i1),
                 col(rels2, "trguid", i3), col(rels2, "trguid2", i3)]
        signs = [col(rels1, "sign", i1), col(rels1, "sign2", i1), col(rels2, "sign", i3), col(rels2, "sign2", i3)]
    else:
        raise ValueError("path_length must be 1..5")

    dirs = [np.asarray(first_neg, dtype=bool)]
    for s, _ok in signs:
        dirs.append(_next_dirs(dirs[-1], s))

    def name(g, ok, r):
        return str(int(g[r])) if ok[r] else "NA"

    paths, signpaths = [], []
    for r in range(len(ids)):
        paths.append(" -> ".join(name(g, ok, r) for g, ok in genes))
        signpaths.append(" -> ".join(f"{name(g, ok, r)} {NEG if d[r] else POS}" for (g, ok), d in zip(genes, dirs)))
    return paths, signpaths


def uid_to_symbol(ents_uid: Sequence[int], ents_symbol: Sequence[str], paths: Sequence[str], signed: bool = False
                  ) -> List[str]:
    """Uid2Symbol / SignUid2SignSymbol (R/Utils.R:50-95): replace every uid by its symbol, "NA" when unknown."""
    table = {int(u): s for u, s in zip(ents_uid, ents_symbol)}
    out = []
    for p in paths:
        hops = []
        for hop in p.split(" -> "):
            if signed:
                uid, _, tag = hop.partition(" ")
                hops.append(f"{table.get(int(uid), 'NA') if uid != 'NA' else 'NA'} {tag}")
            else:
                hops.append(table.get(int(hop), "NA") if hop != "NA" else "NA")
        out.append(" -> ".join(hops))
    return out


COLUMNS = ["SignedPaths", "Paths", "Lengths", "Scores", "Pvalues", "Cases", "Controls"]


def results_table(level_results: Dict[str, object], path_length: int, frames: Dict[str, Dict[str, np.ndarray]],
                  ents: Tuple[Sequence[int], Sequence[str]], ents2: Tuple[Sequence[int], Sequence[str]]):
    """GWASPA.Results (R/ProcessPaths.R:272-326) as a pandas DataFrame.

    ``level_results`` is what ``api.process_paths`` returns ("lst1".."lst5" -> JoinResult); ``frames`` holds
    "rels_data", "rels_data2", "rels", "rels3" (uid-valued).  Rows are ordered by p-value ascending then score
    descending with R's stable ``order``; p-values compare the f64 score with the f32-rounded maxima (App. A-7).
    """
    import pandas as pd

    per_level = {1: ("rels_data2", "rels_data2"), 2: ("rels_data", "rels"), 3: ("rels", "rels"),
                 4: ("rels3", "rels"), 5: ("rels3", "rels3")}
    cols: Dict[str, list] = {c: [] for c in COLUMNS}
    for L in range(1, path_length + 1):
        lst = level_results[f"lst{L}"]
        r = lst.as_r_list()
        f1, f2 = per_level[L]
        paths, signpaths = get_paths(r["ids"], L, frames[f1], frames[f2])
        who = ents2 if L == 1 else ents
        cols["SignedPaths"] += uid_to_symbol(who[0], who[1], signpaths, signed=True)
        cols["Paths"] += uid_to_symbol(who[0], who[1], paths)
        cols["Lengths"] += [L] * len(paths)
        cols["Scores"] += r["scores"].tolist()
        cols["Pvalues"] += lst.pvalues().tolist()
        cols["Cases"] += r["cases"].tolist()
        cols["Controls"] += r["controls"].tolist()
    df = pd.DataFrame(cols, columns=COLUMNS)
    p = df["Pvalues"].to_numpy()
    order = np.lexsort((-df["Scores"].to_numpy(), np.where(np.isnan(p), np.inf, p)))   # order(): NA last, stable
    return df.iloc[order].reset_index(drop=True)


DECORATED_COLUMNS = ["SignedPaths", "Paths", "Subpaths1", "Subpaths1_Cases", "Subpaths1_Controls", "Subpaths2",
                     "Subpaths2_Cases", "Subpaths2_Controls", "Direction", "Lengths", "Scores", "Pvalues",
                     "DecoratedPvalues", "Cases", "Controls"]
DECORATED_PATH_LENGTH_WARNING = "Can only compute the Decorated P-values for pathLength > 1!"
# the decorated draws are keyed by gcre_mix64(seed ^ this tag), a stream apart from the permutation masks' (ProcessPaths.R
# uses one R RNG stream for both; any independent stream has the same distribution)
DECORATED_SEED_TAG = 0x6465636F72617465


def decorated_table(results_df, genes: Sequence[str], data: np.ndarray, n_cases: int, n_ctrls: int, signed: bool,
                    n_permutations: int, strata: Optional[Sequence[int]] = None, seed: int = 0, device: int = 0, *,
                    path_length: Optional[int] = None, exec_=None, table: Optional[np.ndarray] = None):
    """getDecoratedPvalues (R/DecoratedPvalue.R:48-193) over a GWASPA.Results frame: every path of length L >= 2 split at
    its 2(L-1) cut points, Forward then Backward, each split's decorated p-value drawn on the device (k_decorated_null).

    ``genes`` / ``data`` are the dataset after ``preprocess_table`` (the function looks genes up by symbol there, as R
    does after PreprocessTable); ``strata`` one id per patient column; ``signed`` selects method 2.  Rows follow
    ``results_df`` within each length, lengths 2, 3, ...; length-1 rows are dropped (ProcessPaths.R:334).  With
    ``path_length == 1`` it warns as GWASPA does and returns None.  ``exec_`` / ``table``: a JoinExec that already holds
    the value table (its iterations must be ``n_permutations``) and the table itself, to avoid building them twice.
    A path with an NA gene gets NaN; ``n_permutations == 0`` gives NaN everywhere (R: 0/0) and runs nothing on the device.
    Deviations from R (the random stream, the column copy of :97): INTEGRATION.md.
    """
    import pandas as pd
    from . import api

    if path_length == 1:
        warnings.warn(DECORATED_PATH_LENGTH_WARNING)
        return None
    method = 2 if signed else 1
    row_of: Dict[str, int] = {}
    for i, g in enumerate(genes):
        row_of.setdefault(g, i)
    lengths = results_df["Lengths"].to_numpy()
    top = int(lengths.max()) if len(lengths) else 1
    picked = [i for L in range(2, max(top, path_length or 0) + 1) for i in np.flatnonzero(lengths == L).tolist()]

    # SignedPaths "g1 (+) -> g2 (-)": gene = first word, sign = (+) or anything else (DecoratedPvalue.R:112-119)
    hops_of, paths, signs, used = [], [], [], {}
    for i in picked:
        hops = [h.split(" ") for h in str(results_df["SignedPaths"].iat[i]).split(" -> ")]
        names = [h[0] for h in hops]
        rows = []
        for g in names:
            r = row_of.get(g, -1) if g != "NA" else -1
            rows.append(-1 if r < 0 else used.setdefault(r, len(used)))
        hops_of.append(names)
        paths.append(rows)
        signs.append([1 if len(h) > 1 and h[1] == POS else -1 for h in hops])
    data = np.asarray(data)
    sub = data[list(used.keys())] if used else np.zeros((0, n_cases + n_ctrls), np.int32)

    if n_permutations == 0 or not paths:
        vt = api.values_table(n_cases, n_ctrls) if table is None else table
        rec, _ = api.decorated_splits(method, n_cases, n_ctrls, paths, sub, signs, vt, strata)
    else:
        ex = exec_
        if ex is None:
            ex = api.JoinExec(method, n_cases, n_ctrls, n_permutations, device=device)
            ex.set_value_table(api.values_table(n_cases, n_ctrls) if table is None else table)
        try:
            rec = ex.decorated_pvalues(paths, sub, signs, strata=strata, seed=seed)
        finally:
            if exec_ is None:
                ex.close()

    cols: Dict[str, list] = {c: [] for c in DECORATED_COLUMNS}
    for s in rec:
        i, names, j = picked[int(s["path"])], hops_of[int(s["path"])], int(s["j"])
        if s["direction"] == 0:
            sub1, gene2, direction = names[:j], names[j], "Forward"
        else:
            sub1, gene2, direction = names[j - 1:][::-1], names[j - 2], "Backward"
        # DecoratedBestPaths[, c(1,2,10,11,12,14,15)] <- the path's GWASPA.Results row (the intent of :97)
        for c in ("SignedPaths", "Paths", "Lengths", "Scores", "Pvalues", "Cases", "Controls"):
            cols[c].append(results_df[c].iat[i])
        cols["Subpaths1"].append(" -> ".join(sub1))
        cols["Subpaths1_Cases"].append(int(s["cases1"]))
        cols["Subpaths1_Controls"].append(int(s["ctrls1"]))
        cols["Subpaths2"].append(gene2)
        cols["Subpaths2_Cases"].append(int(s["cases2"]))
        cols["Subpaths2_Controls"].append(int(s["ctrls2"]))
        cols["Direction"].append(direction)
        cols["DecoratedPvalues"].append(float(s["pvalue"]))
    return pd.DataFrame(cols, columns=DECORATED_COLUMNS)


SCORE_PATHS_COLUMNS = ["SignedPaths", "Paths", "Lengths", "Scores", "Cases", "Controls", "NominalPvalues",
                       "FamilyPvalues", "Pvalues"]


def parse_sets(paths, genes: Sequence[str]) -> Tuple[List[List[str]], List[List[int]], List[List[int]]]:
    """(symbols, rows, signs) of every entry of ``paths``: a SignedPaths string "A (+) -> B (-)" (a hop whose tag is not
    "(+)" is (-), CheckResults.R:33-34), a Paths string "A -> B" (every gene (+)), or a sequence of symbols (a gene set,
    every gene (+)).  rows = the first row of ``genes`` holding the symbol, -1 for "NA" or a symbol not there."""
    row_of: Dict[str, int] = {}
    for i, g in enumerate(genes):
        row_of.setdefault(g, i)
    names, rows, signs = [], [], []
    for p in paths:
        if isinstance(p, str):
            hops = [h.split() for h in p.split(" -> ")]
            nm = [h[0] if h else "NA" for h in hops]
            sg = [1 if len(h) < 2 or h[1] == POS else -1 for h in hops]
        else:
            nm = [str(g) for g in p]
            sg = [1] * len(nm)
        names.append(nm)
        rows.append([row_of.get(g, -1) if g != "NA" else -1 for g in nm])
        signs.append(sg)
    return names, rows, signs


def _score_sets(rows, signs, data, n_cases, n_ctrls, method, n_permutations, strata, seed, device, family_inference=False,
                minp=False, case_odds=None):
    """score_sets on the rows the sets use, on a context of its own: (records, family maxima); with ``family_inference``
    family_tests instead: (records, family maxima, family records, kmax); with ``minp`` the MINP_SCORE records of
    minp_tests on the same context behind either."""
    from . import api
    used: Dict[int, int] = {}
    sets = [[-1 if r < 0 else used.setdefault(r, len(used)) for r in rs] for rs in rows]
    data = np.asarray(data)
    sub = data[list(used.keys())] if used else np.zeros((0, n_cases + n_ctrls), np.int32)
    ex = api.JoinExec(method, n_cases, n_ctrls, n_permutations, device=device)
    try:
        ex.set_value_table(api.values_table(n_cases, n_ctrls))
        if n_permutations > 0:
            _draw_permutations(ex, seed, strata, case_odds)
        more = (ex.minp_tests(sets, sub, signs)[1],) if minp else ()
        if family_inference:
            rec, fam, kmax = ex.family_tests(sets, sub, signs, kmax=True)
            return (rec, kmax[0], fam, kmax) + more
        return ex.score_sets(sets, sub, signs, family=True) + more
    finally:
        ex.close()


def _tail_pvalues(null: np.ndarray, scores: np.ndarray) -> np.ndarray:
    """#(null >= score) / len(null) for every score (R/ProcessPaths.R:316, f64 score against f32 maxima) by a sort and a
    binary search: the same numbers as JoinResult.pvalues."""
    t = np.sort(np.asarray(null, dtype=np.float32).astype(np.float64))
    if len(t) == 0:
        return np.full(len(scores), np.nan)
    return (len(t) - np.searchsorted(t, scores, side="left")) / len(t)


def score_paths(paths, genes: Sequence[str], data: np.ndarray, n_cases: int, n_ctrls: int, signed: bool = False,
                threshold: float = 0.05, n_permutations: int = 100, strata: Optional[Sequence[int]] = None, seed: int = 0,
                device: int = 0, gwaspa_out: Optional[Dict[str, object]] = None, minp: bool = False,
                competitive: int = 0, competitive_bins: int = 10, fixed: Optional[Sequence[str]] = None,
                stability: int = 0, stability_cuts=None, sequential: int = 0, sequential_hits: int = 20,
                stratified: bool = False, case_odds=None, sequential_weighted: bool = False, family_inference: bool = False):
    """Permutation tests of paths and gene sets the caller names (gcre_score_sets on the device): what GWASPA cannot
    answer for a cascade outside its top K, or for a KEGG / Reactome list.  ``paths`` as ``parse_sets`` reads them;
    genes are looked up after ``preprocess_table(threshold)``, as GWASPA and ``decorated_table`` do (a symbol not found is
    NA: the row gets NaN).  The masks are ``generate_permutations(seed, strata)``'s, the ones ``gwaspa`` draws from the
    same seed.

    Columns: ``Scores`` / ``Cases`` / ``Controls`` as GWASPA.Results counts them; ``NominalPvalues`` the set's own
    permutation p-value; ``FamilyPvalues`` max-T over the given paths (each score against the per-permutation maximum
    over all of them); ``Pvalues`` against the TestScores of ``gwaspa_out``'s level of the same length -- for a network
    path the number GWASPA would print, if the run had the same seed, strata and permutation count (NaN without
    ``gwaspa_out`` or outside its 1..pathLength).

    ``family_inference``: the FAMILY_COLUMNS of ``family_columns`` behind these (gcre_score_sets_family):
    step-down adjusted p-values, expected false positives, FDR and q-values, and k-FWER p-values over the given paths as
    one family.

    ``minp``: the MINP_COLUMNS of ``minp_columns`` behind all of these (gcre_score_sets_minp).
    ``FamilyPvalues`` is max-T on RAW scores: a path's score against the per-permutation maximum of every given set's null
    score, so in a family of paths of mixed length and gene sets the sets with the heaviest null tail own that maximum and
    decide everybody's p-value.  ``FamilyPvaluesMinP`` puts the sets on one scale first: every null score is replaced by the
    nominal p-value it would have got from its own set's null distribution, the per-permutation MINIMUM is taken over the
    family, and the path's ``NominalPvalues`` is held against it (Westfall & Young's min-P, from one set of permutations as
    Ge, Dudoit & Speed 2003 do it).  ``FamilyPvaluesMinPStepDown`` leaves out of that minimum the sets that are more
    significant than the path, and is then made monotone.  With K permutations a set whose ``NominalPvalues`` is 0 (no null
    score reaches it) gets 0 here too, as everywhere in this frame; and the smallest nominal p-value a permutation can
    show is 1 / K, so min-P over V sets needs K well above V before it can tell anything from 1.  ``minp=False`` returns
    exactly the frame without it.

    ``competitive`` > 0: the COMPETITIVE_COLUMNS behind all of these (gcre_score_sets_compete).  Every
    p-value above is self-contained: it permutes the labels and asks whether the set is associated with the phenotype at
    all, which one strong gene answers for every set that contains it.  ``CompetitivePvalues`` asks the competitive
    question instead: the share of ``competitive`` random gene sets of the same size, every gene replaced by one of the same
    ``carrier_bins(data, competitive_bins)`` bin of carrier frequency out of the whole preprocessed table, that score at
    least as high on the OBSERVED labels (drawn from ``seed``; n / K, so 0 when no draw reaches the set).  It is a rank among
    matched random sets conditional on the labels, one set at a time: not a family-wise statement, and nothing here corrects
    it over the paths.  ``fixed``: gene symbols that stay themselves in every draw of the sets that contain them -- "is this
    set anything beyond its known driver?"; the other sets are drawn from the full pool, so naming a gene changes only the
    sets it is in.  A bin must hold twice as many genes as a set draws from it: lower ``competitive_bins`` for large sets on
    a small table.  ``competitive=0`` returns exactly the frame without it.

    ``stability`` = B > 0: the columns of ``stability_columns`` behind all of these (gcre_score_sets_subsample; DESIGN.md
    §3.19).  Every p-value above is a statement under one null; none says how much a row depends on the particular patients
    of the cohort.  Each path is scored on B random halves of the cohort (half of the cases and half of the controls, drawn
    from ``seed``) and on the complementary halves, each half against the value table of its own size: ``StabilityA`` /
    ``StabilityB`` / ``StabilityBoth`` are the shares of the draws in which half A, half B and both reach the cut, and
    ``HalfReplication`` the share of half A's selections that the untouched half B confirms.  ``stability_cuts``, in score
    units on a HALF cohort: one list for every path, or one list per path (a length-3 path and a 200-gene set do not share a
    cut-off); with several cuts the columns carry the cut's index as a suffix.  It is required and has no default: a cut
    is a choice, and the labels must not make it -- a cut taken from this cohort's scores puts the selection back into
    every frequency here.  The numbers are selection frequencies under subsampling of this cohort: descriptive, no p-value
    and no family-wise statement, and ``HalfReplication`` is honest only if neither the paths nor the cuts were chosen on the
    full cohort's labels; otherwise it is optimistic.  The frame's ``attrs["PerHalfSelected"]`` holds, per cut, the mean
    number of paths half A selects in a draw (the q of ``stability_bound``).  ``stability=0`` returns exactly the frame
    without it.

    ``sequential`` = max_perms > 0: the SEQUENTIAL_COLUMNS of ``sequential_columns`` behind all of these
    (gcre_score_sets_sequential).  ``NominalPvalues`` cannot go below 1 / ``n_permutations``, and every path
    pays for all of them.  Here each path is permuted until its null score has reached its score ``sequential_hits`` times, or
    ``sequential`` permutations are used -- the permutations ``generate_permutations(seed, strata)`` would draw, made in
    batches and never kept, so the limit may be far above what a context holds.  ``SequentialPvalues`` = hits / permutations
    used, with a relative error of about 1 / sqrt(``sequential_hits``) wherever it is above ``sequential_hits`` /
    ``sequential``; ``SequentialPerms`` / ``SequentialHits`` are the two counts and ``SequentialStopped`` says whether the
    path reached its hits.  A nominal p-value, one path at a time: the paths stop at different permutations, so there is no
    family-wise version of it.  ``sequential=0`` returns exactly the frame without it.

    ``stratified``: the columns of ``stratified_columns`` behind all of these (gcre_score_sets_strata);
    needs ``strata``.  Stratified permutations keep every p-value above valid when case fraction and carrier frequency both
    differ between the strata, but ``Scores`` is still the POOLED score: a gene that is merely commoner in the case-rich
    stratum scores high under the observed labels and under every such permutation alike, and nothing is left to see.
    ``StratifiedScores`` scores every stratum on its own counts against the value table of its own cases and controls and
    sums the terms (the Cochran-Mantel-Haenszel idea); ``StratifiedPvalues`` is the nominal permutation p-value of that sum
    under the same masks, ``StratifiedFamilyPvalues`` single-step max-T over the given paths.  ``Score.<id>`` / ``Cases.<id>``
    / ``Controls.<id>`` show every stratum's term and carriers: descriptive, no test of heterogeneity is attached.
    ``stratified=False`` returns exactly the frame without it.

    ``case_odds``: one fitted odds of being a case per patient (``case_odds(covariates, ...)``); the masks then come from
    ``generate_weighted_permutations(seed, case_odds, strata)`` (gcre_generate_weighted_masks): every
    permutation p-value above is taken against labels redrawn with these odds, so a continuous covariate that shifts both
    the case fraction and the carrier frequency is in the null.  The adjustment is on the null, not on ``Scores``, and the
    p-values are only as good as the fitted model.  ``gwaspa_out`` must come from ``gwaspa`` with the same ``case_odds``
    (ValueError otherwise); ``sequential`` > 0 is refused with it (that stage makes its own, uniform masks) unless
    ``sequential_weighted`` is set.  None, the default: exactly the frame without it.

    ``sequential_weighted``: with ``case_odds`` and ``sequential`` > 0, the SEQUENTIAL_COLUMNS come from
    ``weighted_sequential_tests(odds=case_odds, strata=strata, seed=seed)`` (gcre_score_sets_sequential_weighted; DESIGN.md
    §3.24) on the call's own context: the permutations ``generate_weighted_permutations(seed, case_odds, strata)`` would
    draw, made in batches and never kept.  The switch is explicit because of what it costs: each weighted permutation takes
    about sqrt(2 pi V) attempts over the whole stratum (V the sum of p (1 - p) over its patients), where a uniform one
    costs one hash per patient -- a limit of 10^6 permutations that is cheap without ``case_odds`` may not be with it.
    Without ``case_odds``, or with ``sequential=0``, it is a ValueError.  False, the default: exactly the frame without it."""
    import pandas as pd
    if sequential_weighted and (case_odds is None or int(sequential) <= 0):
        raise ValueError("sequential_weighted=True needs case_odds and sequential > 0: it draws the sequential permutations with "
                         "these odds")
    if case_odds is not None and int(sequential) > 0 and not sequential_weighted:
        raise ValueError("case_odds: sequential p-values draw their own uniform masks; sequential_weighted=True draws them with "
                         "these odds instead (each permutation then costs about sqrt(2 pi V) attempts over the whole stratum)")
    if gwaspa_out is not None and gwaspa_out.get("case_odds_digest") != _odds_digest(case_odds):
        raise ValueError("gwaspa_out was drawn under different case_odds: its TestScores are not the null of these masks")
    if int(stability) < 0:
        raise ValueError("stability: the number of draws must not be negative")
    if int(sequential) < 0:
        raise ValueError("sequential: the limit of permutations must not be negative")
    if stratified and strata is None:
        raise ValueError("stratified=True needs strata: one id per patient")
    if int(stability) > 0 and stability_cuts is None:
        raise ValueError("stability > 0 needs stability_cuts: there is no default cut (a cut is a choice the labels must not make)")
    method = 2 if signed else 1
    genes, data = preprocess_table(genes, data, threshold, n_cases, n_ctrls)
    names, rows, signs = parse_sets(paths, genes)
    K = int(n_permutations)
    rec, fam, *more = _score_sets(rows, signs, data, n_cases, n_ctrls, method, K, strata, seed, device, family_inference, minp, case_odds)
    valid = rec["valid"] != 0
    score = rec["score"]
    lengths = np.array([len(n) for n in names], dtype=np.int64)
    nan = np.full(len(rec), np.nan)
    family = np.where(valid, _tail_pvalues(fam, score), np.nan) if K > 0 else nan.copy()
    pv = nan.copy()
    if gwaspa_out is not None:
        levels = gwaspa_out["levels"]
        for L in np.unique(lengths).tolist():
            lst = levels.get(f"lst{L}") if 1 <= L <= 5 else None
            sel = (lengths == L) & valid
            if lst is not None and sel.any():
                pv[sel] = _tail_pvalues(lst.null, score[sel])
    cols = {
        "SignedPaths": [" -> ".join(f"{g} {POS if s == 1 else NEG}" for g, s in zip(nm, sg)) for nm, sg in zip(names, signs)],
        "Paths": [" -> ".join(nm) for nm in names],
        "Lengths": lengths,
        "Scores": score,
        "Cases": np.where(valid, rec["cases"], np.nan),
        "Controls": np.where(valid, rec["ctrls"], np.nan),
        "NominalPvalues": rec["pvalue"],
        "FamilyPvalues": family,
        "Pvalues": pv,
    }
    names_out = list(SCORE_PATHS_COLUMNS)
    if family_inference:
        cols.update(family_columns(score, valid, more[0], more[1], K))
        names_out += FAMILY_COLUMNS
    if minp:
        cols.update(minp_columns(rec["n_ge"], valid, score, more[-1], K))
        names_out += MINP_COLUMNS
    if int(competitive) > 0:
        n_ge = _competitive_counts(rows, signs, genes, data, n_cases, n_ctrls, method, int(competitive), competitive_bins, fixed,
                                   seed, device)
        cols.update(competitive_columns(n_ge, valid & ~np.isnan(score), int(competitive)))
        names_out += COMPETITIVE_COLUMNS
    per_half = None
    if int(stability) > 0:
        counts = _stability_counts(rows, signs, data, n_cases, n_ctrls, method, int(stability), stability_cuts, seed, device)
        more_cols, per_half = stability_columns(counts, valid, int(stability))
        cols.update(more_cols)
        names_out += list(more_cols)
    if int(sequential) > 0:
        seq = _sequential_counts(rows, signs, data, n_cases, n_ctrls, method, int(sequential_hits), int(sequential), strata, seed, device,
                                 case_odds if sequential_weighted else None)
        cols.update(sequential_columns(seq, valid))
        names_out += SEQUENTIAL_COLUMNS
    if stratified:
        sr, sfam, terms, counts, ids = _stratified_scores(rows, signs, data, n_cases, n_ctrls, method, K, strata, seed, device, case_odds)
        more_cols = stratified_columns(sr, valid, sfam, terms, counts, ids, K)
        cols.update(more_cols)
        names_out += list(more_cols)
    df = pd.DataFrame(cols, columns=names_out)
    if per_half is not None:
        df.attrs["PerHalfSelected"] = per_half
    return df


def _stability_counts(rows, signs, data, n_cases, n_ctrls, method, draws, cuts, seed, device) -> Dict[str, np.ndarray]:
    """The counts of subsample_tests for ``score_paths``: the default halves and their tables, on the rows the sets use, on a
    context of its own without permutations."""
    from . import api
    used: Dict[int, int] = {}
    sets = [[-1 if r < 0 else used.setdefault(r, len(used)) for r in rs] for rs in rows]
    data = np.asarray(data)
    sub = data[list(used.keys())] if used else np.zeros((0, n_cases + n_ctrls), np.int32)
    ex = api.JoinExec(method, n_cases, n_ctrls, 0, device=device)
    try:
        ex.set_value_table(api.values_table(n_cases, n_ctrls))
        return ex.subsample_tests(sets, sub, signs, draws=draws, seed=seed, cuts=cuts)[1]
    finally:
        ex.close()


def _sequential_counts(rows, signs, data, n_cases, n_ctrls, method, hits, max_perms, strata, seed, device, odds=None) -> np.ndarray:
    """The SEQ_SCORE records of sequential_tests -- with ``odds`` of weighted_sequential_tests -- for ``score_paths``: on the
    rows the sets use, on a context of its own without permutations."""
    from . import api
    used: Dict[int, int] = {}
    sets = [[-1 if r < 0 else used.setdefault(r, len(used)) for r in rs] for rs in rows]
    data = np.asarray(data)
    sub = data[list(used.keys())] if used else np.zeros((0, n_cases + n_ctrls), np.int32)
    ex = api.JoinExec(method, n_cases, n_ctrls, 0, device=device)
    try:
        ex.set_value_table(api.values_table(n_cases, n_ctrls))
        if odds is not None:
            return ex.weighted_sequential_tests(sets, sub, signs, odds=odds, hits=hits, max_perms=max_perms, seed=seed, strata=strata)[1]
        return ex.sequential_tests(sets, sub, signs, hits=hits, max_perms=max_perms, seed=seed, strata=strata)[1]
    finally:
        ex.close()


def _competitive_counts(rows, signs, genes, data, n_cases, n_ctrls, method, draws, n_bins, fixed, seed, device) -> np.ndarray:
    """n_ge of competitive_tests for ``score_paths``: the whole table is the pool, the bins are ``carrier_bins``'; the sets
    that contain a ``fixed`` gene come from a second call in which those genes have bin -1."""
    from . import api
    data = np.asarray(data)
    bins = carrier_bins(data, n_bins)
    ex = api.JoinExec(method, n_cases, n_ctrls, 0, device=device)
    try:
        ex.set_value_table(api.values_table(n_cases, n_ctrls))
        n_ge = ex.competitive_tests(rows, data, signs, bins=bins, draws=draws, seed=seed)[1].copy()
        held = {i for i, g in enumerate(genes) if g in set(fixed)} if fixed else set()
        touched = np.array([any(r in held for r in rs) for rs in rows], bool)
        if touched.any():
            fb = bins.copy()
            fb[sorted(held)] = -1
            n_ge[touched] = ex.competitive_tests(rows, data, signs, bins=fb, draws=draws, seed=seed)[1][touched]
        return n_ge
    finally:
        ex.close()


FAMILY_KMAX = 10   # GCRE_FAMILY_KMAX: the largest null scores of a permutation gcre_score_sets_family keeps
FAMILY_KS = (2, 5, 10)
FAMILY_COLUMNS = ["FamilyPvaluesStepDown", "FamilyExpectedFalse", "FamilyFDR", "FamilyQvalues"] + [f"FamilykFWER.{k}" for k in FAMILY_KS]


def family_reference(obs, valid, null) -> Dict[str, np.ndarray]:
    """The numpy statement of gcre_score_sets_family, no device call: ``obs`` the observed scores, ``valid``
    which sets have no NA member, ``null`` the float32 null matrix [n_sets][K] (rows of invalid sets are not read).  Over the
    valid sets, every comparison as doubles: D_j = {i : obs_i > obs_j} (ties never exclude one another, a NaN score is in
    no D); ``n_ge_stepdown[j]`` = #{r : max over i not in D_j of null[i][r] >= obs_j}; ``exceed[j]`` = #{(i, r) :
    null[i][r] >= obs_j}; ``observed[j]`` = #{i : obs_i >= obs_j}; ``kmax[k][r]`` = the (k+1)-th largest of column r (0
    beyond the valid sets).  A NaN score gets 0 / 0 / 0, an invalid set -1 / 0 / -1.  Computed by one running maximum down
    the sets in ascending order and one sort of the pooled values."""
    obs = np.asarray(obs, np.float64).ravel()
    S = len(obs)
    valid = np.asarray(valid).ravel() != 0
    N = np.asarray(null, np.float32).reshape(S, -1)
    K = N.shape[1]
    sd = np.where(valid, 0, -1).astype(np.int64)
    ob = sd.copy()
    ex = np.zeros(S, np.uint64)
    kmax = np.zeros((FAMILY_KMAX, K), np.float32)
    idx = np.flatnonzero(valid)
    if len(idx) == 0:
        return {"n_ge_stepdown": sd, "exceed": ex, "observed": ob, "kmax": kmax}
    ov = obs[idx]
    isnan = np.isnan(ov)
    order = np.concatenate([np.flatnonzero(isnan), np.flatnonzero(~isnan)[np.argsort(ov[~isnan], kind="stable")]])
    Nv = N[idx][order].astype(np.float64)                 # ascending observed order, NaN scores first
    top = -np.sort(-N[idx], axis=0)[:FAMILY_KMAX]
    kmax[:len(top)] = top
    t = ov[order]
    n_nan = int(isnan.sum())
    ts = t[n_nan:]
    run = np.maximum.accumulate(Nv, axis=0)               # run[i] = the maximum over the sets up to sorted position i
    last = n_nan + np.searchsorted(ts, ts, side="right") - 1    # the end of each tie group: nothing up to it is in D
    first = n_nan + np.searchsorted(ts, ts, side="left")
    pooled = np.sort(Nv.ravel())
    dst = idx[order[n_nan:]]
    sd[dst] = (run[last] >= ts[:, None]).sum(axis=1)
    ex[dst] = (len(pooled) - np.searchsorted(pooled, ts, side="left")).astype(np.uint64)
    ob[dst] = len(idx) - first
    return {"n_ge_stepdown": sd, "exceed": ex, "observed": ob, "kmax": kmax}


def family_columns(scores, valid, family, kmax, perms: int) -> Dict[str, np.ndarray]:
    """FAMILY_COLUMNS of one family of given sets, from what ``JoinExec.family_tests(kmax=True)`` (or ``family_reference``)
    returns: ``family`` with n_ge_stepdown / exceed / observed per set, ``kmax`` float32 [FAMILY_KMAX][perms].
    ``FamilyPvaluesStepDown`` through ``stepdown_columns`` (the monotone step), ``FamilyExpectedFalse`` / ``FamilyFDR`` /
    ``FamilyQvalues`` through ``fdr_columns``, ``FamilykFWER.k`` = the share of permutations whose k-th largest null score
    reaches the set's score (the probability of k or more false positives at that threshold, single-step).  NaN for a set
    with an NA member or a NaN score, and everywhere when perms = 0."""
    s = np.asarray(scores, np.float64).ravel()
    ok = (np.asarray(valid).ravel() != 0) & ~np.isnan(s)
    B = int(perms)
    out = {c: np.full(len(s), np.nan) for c in FAMILY_COLUMNS}
    if B <= 0 or not ok.any():
        return out
    out["FamilyPvaluesStepDown"][ok] = stepdown_columns(s[ok], np.asarray(family["n_ge_stepdown"])[ok], B)["PvaluesStepDown"]
    fdr = fdr_columns(s[ok], np.asarray(family["exceed"])[ok], np.asarray(family["observed"])[ok], B)
    for c in FDR_COLUMNS:
        out["Family" + c][ok] = fdr[c]
    km = np.asarray(kmax, np.float32).reshape(FAMILY_KMAX, -1)
    for k in FAMILY_KS:
        out[f"FamilykFWER.{k}"][ok] = _tail_pvalues(km[k - 1], s[ok])
    return out


MINP_COLUMNS = ["FamilyPvaluesMinP", "FamilyPvaluesMinPStepDown"]


def minp_reference(obs, valid, null) -> Dict[str, np.ndarray]:
    """The numpy statement of gcre_score_sets_minp, no device call: ``obs`` the observed scores, ``valid``
    which sets have no NA member, ``null`` the float32 null matrix [n_sets][K] (rows of invalid sets are not read).  Over the
    valid sets: ``n_ge[i]`` = c_i = #{r : (double)null[i][r] >= obs_i} (0 for a NaN score); ``counts[i][r]`` = R[i][r] =
    #{r' : null[i][r'] >= null[i][r]}, compared as float32; ``min_count[r]`` = the minimum of R[.][r];  ``n_le_minp[j]`` =
    #{r : min_count[r] <= c_j}; D_j = {i : c_i < c_j} (ties never exclude one another, a NaN score is in no D);
    ``n_le_stepdown[j]`` = #{r : min over i not in D_j of R[i][r] <= c_j}.  A NaN score gets 0 / 0, an invalid set n_ge 0,
    -1 / -1 and a row of 0xFFFFFFFF; ``min_count`` is 0xFFFFFFFF without a valid set.  Computed by one sort per row and one
    running minimum down the sets in descending order of c."""
    obs = np.asarray(obs, np.float64).ravel()
    S = len(obs)
    valid = np.asarray(valid).ravel() != 0
    N = np.asarray(null, np.float32).reshape(S, -1)
    K = N.shape[1]
    c = np.zeros(S, np.int64)
    mp = np.where(valid, 0, -1).astype(np.int64)
    sd = mp.copy()
    counts = np.full((S, K), 0xFFFFFFFF, np.uint32)
    mc = np.full(K, 0xFFFFFFFF, np.uint32)
    idx = np.flatnonzero(valid)
    if len(idx) == 0 or K == 0:
        return {"n_ge": c, "n_le_minp": mp, "n_le_stepdown": sd, "min_count": mc, "counts": counts}
    Nv = N[idx]
    srt = np.sort(Nv, axis=1)
    for k, i in enumerate(idx):
        counts[i] = K - np.searchsorted(srt[k], Nv[k], side="left")
        if not np.isnan(obs[i]):
            c[i] = K - np.searchsorted(srt[k].astype(np.float64), obs[i], side="left")
    Rv = counts[idx]
    mc = Rv.min(axis=0)
    cv = c[idx]
    isnan = np.isnan(obs[idx])
    scored = np.flatnonzero(~isnan)
    order = np.concatenate([np.flatnonzero(isnan), scored[np.argsort(-cv[scored], kind="stable")]])
    run = np.minimum.accumulate(Rv[order], axis=0)        # run[i] = the minimum over the sets up to walk position i
    n_nan = int(isnan.sum())
    cs = cv[order[n_nan:]]                                # descending
    last = n_nan + np.searchsorted(-cs, -cs, side="right") - 1   # the end of each tie group: nothing up to it is in D
    dst = idx[order[n_nan:]]
    sd[dst] = (run[last] <= cs[:, None].astype(np.uint32)).sum(axis=1)
    mcs = np.sort(mc)
    mp[dst] = np.searchsorted(mcs, cs.astype(np.uint32), side="right")
    return {"n_ge": c, "n_le_minp": mp, "n_le_stepdown": sd, "min_count": mc, "counts": counts}


def minp_columns(n_ge, valid, scores, minp, perms: int) -> Dict[str, np.ndarray]:
    """MINP_COLUMNS of one family of given sets, from what ``JoinExec.minp_tests`` (or ``minp_reference``) returns: ``minp``
    with n_le_minp / n_le_stepdown per set, ``n_ge`` the sets' own counts c.  ``FamilyPvaluesMinP`` = n_le_minp / perms,
    the single-step min-P adjusted p-value; ``FamilyPvaluesMinPStepDown`` = n_le_stepdown / perms made monotone by a
    running maximum from the smallest c upwards (a less significant set never gets a smaller adjusted p-value; sets that tie
    in c are equal).  NaN for a set with an NA member or a NaN score, and everywhere when perms = 0."""
    s = np.asarray(scores, np.float64).ravel()
    ok = (np.asarray(valid).ravel() != 0) & ~np.isnan(s)
    B = int(perms)
    out = {col: np.full(len(s), np.nan) for col in MINP_COLUMNS}
    if B <= 0 or not ok.any():
        return out
    c = np.asarray(n_ge, np.int64).ravel()[ok]
    out["FamilyPvaluesMinP"][ok] = np.asarray(minp["n_le_minp"], np.int64).ravel()[ok] / B
    sd = np.asarray(minp["n_le_stepdown"], np.int64).ravel()[ok]
    order = np.argsort(c, kind="stable")
    mono = np.maximum.accumulate(sd[order])
    last = np.searchsorted(c[order], c[order], side="right") - 1     # tied sets take the value at the end of their group
    adj = np.empty(len(c))
    adj[order] = mono[last] / B
    out["FamilyPvaluesMinPStepDown"][ok] = adj
    return out


# competitive set tests: matched random sets on the observed labels

COMPETITIVE_COLUMNS = ["CompetitivePvalues"]
COMPETE_ATTEMPTS = 64      # attempts of a member before the fallback, and the stride of the member index in the random stream
_U64 = np.uint64


def _mix64(z):
    """gcre_mix64 (the splitmix64 finaliser) on numpy uint64, wrapping."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=_U64) + _U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


def _compete_base(seed: int, s: int, b) -> np.ndarray:
    """dp_perm_base(dp_split_key(seed, s), b) for every draw of ``b``."""
    with np.errstate(over="ignore"):
        key = _mix64(_U64(int(seed) & (2**64 - 1)) ^ (_U64(0xD1B54A32D192ED03) * _U64(int(s) + 1)))
        return _mix64(key ^ (_U64(0x51ED270B7F3C9A1D) * (np.asarray(b, dtype=_U64) + _U64(1))))


def _mulhi(u, n: int) -> np.ndarray:
    """floor(u * n / 2^64) for uint64 u and 0 < n < 2^32, by 32-bit halves: neither partial product leaves 64 bits."""
    u = np.asarray(u, dtype=_U64)
    n = _U64(n)
    hi, lo = u >> _U64(32), u & _U64(0xFFFFFFFF)
    return ((hi * n + ((lo * n) >> _U64(32))) >> _U64(32)).astype(np.int64)


def _compete_pools(bins, n_rows: int):
    """(bin of every row, {bin: its rows ascending}); ``bins`` None = one bin with every row."""
    bn = np.zeros(int(n_rows), np.int64) if bins is None else np.asarray(bins, dtype=np.int64).reshape(-1)
    if len(bn) != n_rows:
        raise ValueError(f"bins: {len(bn)} entries for {n_rows} rows")
    return bn, {int(v): np.flatnonzero(bn == v) for v in np.unique(bn[bn >= 0])}


def _compete_draws(members, bn, pools, s: int, b, seed: int, attempts: int) -> np.ndarray:
    """The draw rule for the draws ``b`` of set ``s`` at once: int64 [len(b)][members]."""
    members = np.asarray(members, dtype=np.int64).reshape(-1)
    b = np.asarray(b, dtype=np.int64).reshape(-1)
    if not 1 <= int(attempts) <= COMPETE_ATTEMPTS:
        raise ValueError(f"attempts must be 1..{COMPETE_ATTEMPTS}")
    base = _compete_base(seed, s, b)
    picks = np.full((len(b), len(members)), -1, np.int64)
    need: Dict[int, int] = {}
    for j, row in enumerate(members.tolist()):
        beta = int(bn[row]) if row >= 0 else -1
        if beta < 0:                     # a fixed member stays itself
            picks[:, j] = row
            continue
        pool = pools[beta]
        need[beta] = need.get(beta, 0) + 1
        if 2 * need[beta] > len(pool):
            raise ValueError(f"set {s} draws {need[beta]} members from bin {beta} of {len(pool)} rows: 2k <= N is required")
        pending = np.arange(len(b))
        with np.errstate(over="ignore"):
            at = base + _U64(COMPETE_ATTEMPTS * j)
        for t in range(int(attempts)):
            if len(pending) == 0:
                break
            with np.errstate(over="ignore"):
                u = _mix64(at[pending] + _U64(t))
            cand = pool[_mulhi(u, len(pool))]
            taken = (picks[pending, :j] == cand[:, None]).any(axis=1)
            picks[pending[~taken], j] = cand[~taken]
            pending = pending[taken]
        for i in pending.tolist():        # the fallback: the lowest pool entry not yet handed out
            picks[i, j] = pool[~np.isin(pool, picks[i, :j])][0]
    return picks


def competitive_picks(set_members, bins, n_rows: int, s: int, b: int, seed: int, attempts: int = COMPETE_ATTEMPTS) -> np.ndarray:
    """The draw rule of gcre_score_sets_compete (csrc/gcre_compete.h is the same rule in C++): the row every
    member of set ``s`` (``set_members``: rows of the pool, in list order) receives in draw ``b``.  ``bins`` [n_rows]: the bin
    of every row, -1 = never drawn (a member there is fixed); None = one bin.  The pool of a bin is its rows, ascending.
    Member j, in order, reads u = mix64(base + 64 j + t) for attempt t = 0, 1, ..., base = mix64(key ^ C2 (b + 1)), key =
    mix64(seed ^ C1 (s + 1)) (dp_perm_base / dp_split_key), proposes pool entry floor(u N / 2^64) and takes the first proposal
    no earlier member of the draw received; after ``attempts`` failures the lowest pool entry not handed out.  A pure
    function of (seed, s, b).  int64 [members]."""
    bn, pools = _compete_pools(bins, n_rows)
    return _compete_draws(set_members, bn, pools, s, [b], seed, attempts)[0]


def competitive_reference(sets, rows, signs, bins, draws: int, seed: int, n_cases: int, table, method: int,
                          attempts: int = COMPETE_ATTEMPTS) -> Dict[str, np.ndarray]:
    """The numpy statement of gcre_score_sets_compete, no device call.  ``rows``: the 0/1 carrier matrix
    [pool rows][patients], columns < n_cases the cases; ``sets`` / ``signs`` as ``JoinExec.score_sets`` takes them; ``table``
    the value table.  Per valid set and draw the picks of ``competitive_picks``, the unions of the drawn rows (method 1 the OR
    of all, method 2 P / N by sign), and table[|P & cases|][|P & ctrls|] (+ table[|N & ctrls|][|N & cases|], added in this
    order).  Returns ``n_ge`` int64 [sets] = #{b : null >= observed} as doubles (-1 for a set with an NA member), ``null``
    float64 [sets][draws] (NaN rows for those), ``picks`` int32 [draws][members of all sets] (-1 for those) and ``obs``."""
    d = np.asarray(rows) != 0
    n = d.shape[1]
    B = int(draws)
    VT = np.asarray(table, np.float64)
    case = np.arange(n) < n_cases
    bn, pools = _compete_pools(bins, len(d))
    S = len(sets)
    lens = [len(x) for x in sets]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n_ge = np.zeros(S, np.int64)
    obs = np.full(S, np.nan)
    null = np.full((S, B), np.nan)
    picks = np.full((B, int(off[-1])), -1, np.int32)

    def scores(r, sg):                       # r [draws][members] rows, sg [members]
        neg = (sg == -1) if method == 2 else np.zeros(len(sg), bool)
        P = np.zeros((len(r), n), bool)
        N = np.zeros((len(r), n), bool)
        for j in range(r.shape[1]):
            (N if neg[j] else P)[:] |= d[r[:, j]]
        v = _vt_cell(VT, n, (P & case).sum(axis=1), (P & ~case).sum(axis=1))
        if method == 2:
            with np.errstate(invalid="ignore"):                       # inf - inf
                v = v + _vt_cell(VT, n, (N & ~case).sum(axis=1), (N & case).sum(axis=1))
        return v

    for s in range(S):
        m = np.asarray(sets[s], dtype=np.int64).reshape(-1)
        if (m < 0).any():
            n_ge[s] = -1
            continue
        sg = np.ones(len(m), np.int64) if signs is None else np.asarray(signs[s], dtype=np.int64).reshape(-1)
        obs[s] = scores(m[None, :], sg)[0]
        if B == 0:
            continue
        pk = _compete_draws(m, bn, pools, s, np.arange(B), seed, attempts)
        picks[:, off[s]:off[s + 1]] = pk
        null[s] = scores(pk, sg)
        n_ge[s] = int((null[s] >= obs[s]).sum())
    return {"n_ge": n_ge, "null": null, "picks": picks, "obs": obs}


def carrier_bins(data, n_bins: int) -> np.ndarray:
    """Bins of equal count by carrier total for ``competitive_tests``: the rows of the 0/1 matrix ``data`` ordered by their
    carrier totals (stable: ties by row) and cut into ``n_bins`` runs whose sizes differ by at most one, the fewest
    carriers in bin 0.  int32 [rows]; fewer rows than bins leave the upper bins empty."""
    tot = (np.asarray(data) != 0).sum(axis=1)
    R = len(tot)
    nb = max(int(n_bins), 1)
    order = np.argsort(tot, kind="stable")
    out = np.zeros(R, np.int32)
    out[order] = (np.arange(R, dtype=np.int64) * nb // max(R, 1)).astype(np.int32)
    return out


def competitive_columns(n_ge, valid, draws: int) -> Dict[str, np.ndarray]:
    """COMPETITIVE_COLUMNS from what ``JoinExec.competitive_tests`` (or ``competitive_reference``) returns:
    ``CompetitivePvalues`` = n_ge / draws, the share of matched random sets that score at least as high on the observed
    labels -- the project's n / K convention, not (n + 1) / (K + 1).  NaN for a set with an NA member (``valid`` 0 or n_ge
    < 0), for a NaN score (``valid`` may carry ``~isnan(score)``) and with 0 draws."""
    c = np.asarray(n_ge, np.int64).ravel()
    ok = (np.asarray(valid).ravel() != 0) & (c >= 0)
    B = int(draws)
    out = np.full(len(c), np.nan)
    if B > 0:
        out[ok] = c[ok] / B
    return {"CompetitivePvalues": out}


# split-half stability: sets scored on random halves of the cohort and on their complements

STABILITY_COLUMNS = ["StabilityA", "StabilityB", "StabilityBoth", "HalfReplication"]
SUBSAMPLE_SEED_TAG = 0x73756273616D706C     # "subsampl": seed' = mix64(seed ^ tag)


def subsample_masks(n_cases: int, n_ctrls: int, m_cases: int, m_ctrls: int, draws, seed: int) -> np.ndarray:
    """The draw rule of gcre_score_sets_subsample (csrc/gcre_subsample.h is the same rule in C++): bool
    [draws][n_cases + n_ctrls], row b the patients of draw b -- exactly ``m_cases`` among the columns < n_cases and
    ``m_ctrls`` among the rest.  ``draws``: their number (draws 0 .. draws-1), or a sequence of draw indices.  Knuth's
    selection sampling with the label as the stratum: with seed' = mix64(seed ^ SUBSAMPLE_SEED_TAG) and base_b = mix64(seed'
    ^ C2 (b + 1)), patient c, in column order, reads u = mix64(base_b + c) and is taken when floor(u rem / 2^64) < need, rem
    the patients of its stratum not yet walked (c included) and need those still to be taken.  A pure function of (seed, b,
    c)."""
    n_cases, n_ctrls, m_cases, m_ctrls = int(n_cases), int(n_ctrls), int(m_cases), int(m_ctrls)
    if not (0 <= m_cases <= n_cases and 0 <= m_ctrls <= n_ctrls):
        raise ValueError(f"m = ({m_cases}, {m_ctrls}) outside 0 .. ({n_cases}, {n_ctrls})")
    b = np.arange(int(draws), dtype=np.int64) if np.ndim(draws) == 0 else np.asarray(draws, dtype=np.int64).reshape(-1)
    n = n_cases + n_ctrls
    with np.errstate(over="ignore"):
        seed1 = _mix64(_U64(int(seed) & (2**64 - 1)) ^ _U64(SUBSAMPLE_SEED_TAG))
        base = _mix64(seed1 ^ (_U64(0x51ED270B7F3C9A1D) * (b.astype(_U64) + _U64(1))))
    out = np.zeros((len(b), n), bool)
    need = np.zeros(len(b), np.int64)
    for c in range(n):
        if c == 0:
            rem, need[:] = n_cases, m_cases
        if c == n_cases:
            rem, need[:] = n_ctrls, m_ctrls
        with np.errstate(over="ignore"):
            u = _mix64(base + _U64(c))
        take = _mulhi(u, rem) < need
        out[:, c] = take
        need -= take
        rem -= 1
    return out


def subsample_reference(sets, rows, signs, n_cases: int, m_cases: int, m_ctrls: int, draws: int, seed: int, table_a, table_b,
                        cuts, method: int) -> Dict[str, np.ndarray]:
    """The numpy statement of gcre_score_sets_subsample, no device call.  ``rows``: the 0/1 carrier matrix
    [rows][patients], columns < n_cases the cases; ``sets`` / ``signs`` as ``JoinExec.score_sets`` takes them; ``table_a`` /
    ``table_b`` the value tables of the half cohorts (``table_b`` None or False: half B is not scored); ``cuts`` [sets][cuts],
    one list for every set, or None.  Per valid set and draw S_b of ``subsample_masks``: half A = table_a[|P & S_b &
    cases|][|P & S_b & ctrls|] (+ table_a[|N & S_b & ctrls|][|N & S_b & cases|], added in this order), half B the same on
    the complement of S_b from table_b; cells a table does not have read as -1.  Returns ``n_a`` / ``n_b`` / ``n_both`` int64
    [sets][cuts] (-1 for a set with an NA member; the B counts None without half B) and ``scores_a`` / ``scores_b`` float64
    [sets][draws] (NaN rows for those)."""
    d = np.asarray(rows) != 0
    n = d.shape[1]
    B = int(draws)
    S = len(sets)
    case = np.arange(n) < n_cases
    half_b = table_b is not None and table_b is not False
    TA = np.asarray(table_a, np.float64)
    TB = np.asarray(table_b, np.float64) if half_b else None
    ct = np.zeros((S, 0)) if cuts is None else np.asarray(cuts, np.float64)
    if ct.ndim == 1:
        ct = np.broadcast_to(ct, (S, len(ct)))
    mk = subsample_masks(n_cases, n - n_cases, m_cases, m_ctrls, B, seed)
    n_half = int(m_cases) + int(m_ctrls)

    def scores(P, N, keep, VT, nh):                 # P, N bool [n]; keep bool [draws][n]
        v = _vt_cell(VT, nh, (keep & (P & case)).sum(axis=1), (keep & (P & ~case)).sum(axis=1))
        if method == 2:
            with np.errstate(invalid="ignore"):      # inf - inf
                v = v + _vt_cell(VT, nh, (keep & (N & ~case)).sum(axis=1), (keep & (N & case)).sum(axis=1))
        return v

    res = {"n_a": np.zeros((S, ct.shape[1]), np.int64), "scores_a": np.full((S, B), np.nan),
           "n_b": np.zeros((S, ct.shape[1]), np.int64) if half_b else None,
           "n_both": np.zeros((S, ct.shape[1]), np.int64) if half_b else None,
           "scores_b": np.full((S, B), np.nan) if half_b else None}
    for s in range(S):
        m = np.asarray(sets[s], dtype=np.int64).reshape(-1)
        if (m < 0).any():
            for k in ("n_a", "n_b", "n_both"):
                if res[k] is not None:
                    res[k][s] = -1
            continue
        sg = np.ones(len(m), np.int64) if signs is None else np.asarray(signs[s], dtype=np.int64).reshape(-1)
        neg = (sg == -1) if method == 2 else np.zeros(len(m), bool)
        P = d[m[~neg]].any(axis=0) if (~neg).any() else np.zeros(n, bool)
        N = d[m[neg]].any(axis=0) if neg.any() else np.zeros(n, bool)
        A = scores(P, N, mk, TA, n_half)
        res["scores_a"][s] = A
        with np.errstate(invalid="ignore"):
            ga = A[None, :] >= ct[s][:, None]                            # [cuts][draws]; a NaN never counts
            res["n_a"][s] = ga.sum(axis=1)
            if half_b:
                Bs = scores(P, N, ~mk, TB, n - n_half)
                res["scores_b"][s] = Bs
                gb = Bs[None, :] >= ct[s][:, None]
                res["n_b"][s] = gb.sum(axis=1)
                res["n_both"][s] = (ga & gb).sum(axis=1)
    return res


def stability_columns(counts, valid, draws: int):
    """(columns, PerHalfSelected) from the ``counts`` of ``JoinExec.subsample_tests`` (or ``subsample_reference``):
    ``StabilityA`` = n_a / draws, ``StabilityB`` = n_b / draws and ``StabilityBoth`` = n_both / draws, the shares of the
    draws in which half A, the complementary half B and both reach the cut; ``HalfReplication`` = n_both / n_a, the share of
    half A's selections that half B confirms, NaN where half A never selects.  With several cuts every name carries the
    cut's index (``StabilityA.0``, ``StabilityA.1``, ...).  NaN for a set with an NA member (``valid`` 0 or a count < 0) and
    with 0 draws; the B columns are all NaN without half B.  ``PerHalfSelected``: per cut the mean number of valid sets half
    A selects in a draw, the sum of n_a over the valid sets / draws -- the q of ``stability_bound``.
    Selection frequencies under subsampling of this cohort: descriptive, not p-values, and ``HalfReplication`` is optimistic
    if the sets or the cuts were chosen on the full cohort's labels."""
    na = np.asarray(counts["n_a"], np.int64)
    na = na.reshape(len(na), -1)
    S, C = na.shape
    B = int(draws)
    ok = (np.asarray(valid).ravel()[:S] != 0)[:, None] & (na >= 0)
    get = lambda k: (np.asarray(counts[k], np.int64).reshape(S, C) if counts.get(k) is not None else None)
    nb, nab = get("n_b"), get("n_both")

    def share(num, den):
        out = np.full((S, C), np.nan)
        if num is not None:
            den = np.broadcast_to(np.asarray(den, np.float64), (S, C))
            sel = ok & (den > 0)
            out[sel] = num[sel] / den[sel]
        return out

    mats = {"StabilityA": share(na, B), "StabilityB": share(nb, B), "StabilityBoth": share(nab, B), "HalfReplication": share(nab, na)}
    cols = {(name if C == 1 else f"{name}.{j}"): mats[name][:, j] for j in range(C) for name in STABILITY_COLUMNS}
    per_half = (np.where(ok, na, 0).sum(axis=0) / B) if B > 0 else np.full(C, np.nan)
    return cols, per_half


def stability_bound(q: float, n_sets: int, tau: float) -> float:
    """Meinshausen & Buhlmann's (2010, Theorem 1) bound on the expected number of falsely selected sets among those whose
    selection frequency is at least ``tau`` > 1/2: q^2 / ((2 tau - 1) n_sets), q the mean number of sets a half selects
    (``PerHalfSelected``) and ``n_sets`` the size of the family.  The bound assumes that the selection of the null sets is
    exchangeable and no worse than random guessing.  Overlapping paths through one gene do not meet this -- they are
    selected together or not at all -- so the number is indicative, not a guarantee."""
    if not tau > 0.5:
        raise ValueError("stability_bound: tau must be above 1/2")
    if n_sets < 1:
        raise ValueError("stability_bound: n_sets must be at least 1")
    return float(q) * float(q) / ((2.0 * float(tau) - 1.0) * float(n_sets))


SEQUENTIAL_COLUMNS = ["SequentialPvalues", "SequentialPerms", "SequentialHits", "SequentialStopped"]


def permutation_masks(n_cases: int, n_ctrls: int, perms, seed: int, strata=None) -> np.ndarray:
    """The mask rule of ``JoinExec.generate_permutations(seed, strata)`` and of gcre_score_sets_sequential (k_generate_masks;
    csrc/gcre_sequential.h is the same rule in C++): bool [perms][n_cases + n_ctrls], row r the patients that permutation r
    labels as cases -- inside every stratum as many as it has cases among the columns < n_cases.  ``perms``: their number
    (permutations 0 .. perms-1), or a sequence of permutation indices (any non-negative integers below 2^64 - 1).
    ``strata``: one id >= 0 per patient, or None for one stratum.  Knuth's selection sampling per stratum: with base_r =
    mix64(seed ^ C2 (r + 1)), patient c, in column order, reads u = mix64(base_r + c) and becomes a case when
    floor(u rem / 2^64) < need, rem the patients of its stratum not yet walked (c included) and need its cases still to be
    placed.  A pure function of (seed, r, c)."""
    n_cases, n_ctrls = int(n_cases), int(n_ctrls)
    n = n_cases + n_ctrls
    r = np.arange(int(perms), dtype=_U64) if np.ndim(perms) == 0 else np.array([int(x) for x in np.asarray(perms, dtype=object).reshape(-1)], dtype=_U64)
    st = np.zeros(n, np.int64) if strata is None else np.asarray(strata, dtype=np.int64).reshape(-1)
    if len(st) != n or (st < 0).any():
        raise ValueError(f"strata: one id >= 0 per patient ({n}), not {len(st)} of which {(st < 0).sum()} are negative")
    ns = int(st.max()) + 1 if n else 1
    with np.errstate(over="ignore"):
        base = _mix64(_U64(int(seed) & (2**64 - 1)) ^ (_U64(0x51ED270B7F3C9A1D) * (r + _U64(1))))
    out = np.zeros((len(r), n), bool)
    need = np.zeros((ns, len(r)), np.int64)
    rem = np.zeros(ns, np.int64)
    for s in range(ns):
        need[s] = int((st[:n_cases] == s).sum())
        rem[s] = int((st == s).sum())
    for c in range(n):
        s = int(st[c])
        with np.errstate(over="ignore"):
            u = _mix64(base + _U64(c))
        take = _mulhi(u, int(rem[s])) < need[s]
        out[:, c] = take
        need[s] -= take
        rem[s] -= 1
    return out


WEIGHTED_TAG = 0x7765696768746564   # kWeightedTag (csrc/gcre_weighted.h): "weighted"
WEIGHTED_NONE = 0xFFFFFFFF          # kWeightedNone: no accepted attempt below the cap


def _draw_permutations(ex, seed, strata, case_odds) -> None:
    """The masks of a ``gwaspa`` / ``score_paths`` context: uniform, or with ``case_odds`` the covariate-adjusted ones."""
    if case_odds is None:
        ex.generate_permutations(seed, strata)
    else:
        ex.generate_weighted_permutations(seed, case_odds, strata)


def _odds_digest(case_odds):
    """What ``gwaspa`` records of the odds its masks were drawn with, and ``score_paths`` compares: None, or a digest."""
    if case_odds is None:
        return None
    import hashlib
    h = hashlib.sha256(np.ascontiguousarray(np.asarray(case_odds, dtype=np.float64).reshape(-1)).tobytes())
    return h.hexdigest()


def weighted_masks(thresholds, n_cases: int, n_ctrls: int, perms, seed: int, strata=None, max_attempts: int = 1 << 20):
    """The draw rule of ``JoinExec.generate_weighted_permutations`` (csrc/gcre_weighted.h) in numpy, on the
    library's own ``thresholds`` (``api.weighted_thresholds``: uint32 per patient): ``(masks, attempts)`` -- bool
    [perms][n], row r the patients permutation r labels as cases, and uint32 [perms][S], the accepted attempts.  ``strata``:
    one id per patient, any integers (mapped to 0 .. S-1 in ascending order), or None for one stratum.

    Exact rejection in integers: with seed' = mix64(seed ^ WEIGHTED_TAG), key_r = mix64(seed' ^ C2 (r + 1)), base_rs =
    mix64(key_r ^ C1 (s + 1)) and pair_rsj = mix64(base_rs + j), attempt a of (r, s) reads u = mix64(pair_rsj + c), j = a >> 1,
    for the patient in column c of stratum s and labels it a case when the high half of u (a even) or the low half (a odd)
    is below the patient's threshold.  The accepted attempt is the smallest a whose case count over the stratum equals its
    cases among the columns < n_cases; a pair without one below ``max_attempts`` gets WEIGHTED_NONE and no case."""
    n_cases, n_ctrls = int(n_cases), int(n_ctrls)
    n = n_cases + n_ctrls
    thr = np.asarray(thresholds, dtype=_U64).reshape(-1)
    if len(thr) != n:
        raise ValueError(f"thresholds: one per patient ({n}), not {len(thr)}")
    if strata is None:
        inv, S = np.zeros(n, np.int64), 1
    else:
        ids, inv = np.unique(np.asarray(strata).reshape(-1), return_inverse=True)
        S = len(ids)
        if len(inv) != n:
            raise ValueError(f"strata: one id per patient ({n}), not {len(inv)}")
    K = int(perms)
    cap = int(max_attempts)
    masks = np.zeros((K, n), bool)
    att = np.full((K, S), WEIGHTED_NONE, dtype=np.uint32)
    r = np.arange(K, dtype=_U64)
    with np.errstate(over="ignore"):
        seed1 = _mix64(_U64(int(seed) & (2**64 - 1)) ^ _U64(WEIGHTED_TAG))
        key = _mix64(seed1 ^ (_U64(0x51ED270B7F3C9A1D) * (r + _U64(1))))
    for s in range(S):
        cols = np.flatnonzero(inv == s)
        need = int((cols < n_cases).sum())
        with np.errstate(over="ignore"):
            base = _mix64(key ^ (_U64(0xD1B54A32D192ED03) * _U64(s + 1)))
        todo = np.arange(K)
        j = 0
        while len(todo) and 2 * j < cap:
            with np.errstate(over="ignore"):
                pair = _mix64(base[todo] + _U64(j))
                u = _mix64(pair[:, None] + cols.astype(_U64)[None, :])
            even = (u >> _U64(32)) < thr[cols][None, :]
            odd = (u & _U64(0xFFFFFFFF)) < thr[cols][None, :]
            hit_e = even.sum(axis=1) == need
            hit_o = (odd.sum(axis=1) == need) & ~hit_e & (2 * j + 1 < cap)
            for hit, bits, a in ((hit_e, even, 2 * j), (hit_o, odd, 2 * j + 1)):
                rows = todo[hit]
                masks[np.ix_(rows, cols)] = bits[hit]
                att[rows, s] = a
            todo = todo[~(hit_e | hit_o)]
            j += 1
    return masks, att


def conditional_bernoulli_reference(p, m: int, subsets: bool = False):
    """The target law of the weighted masks, exactly: independent Bernoulli(p_c) conditioned on exactly ``m`` successes
    (equivalently P(A) proportional to the product of the odds p_c / (1 - p_c) over A).  Returns the inclusion
    probabilities P(c in A), float64 [n], by the standard recursion on R(k, C) = the sum over k-subsets of C of the product
    of the odds: R(k, C) = R(k, C \\ c) + w_c R(k - 1, C \\ c), P(c in A) = w_c R(m - 1, C \\ c) / R(m, C).  With ``subsets``
    (tiny n) also ``(subset tuples in lexicographic order, their probabilities)``.  p_c = 1 is not accepted (an odds of
    +infinity)."""
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    n, m = len(p), int(m)
    if (p < 0).any() or (p >= 1).any() or not 0 <= m <= n:
        raise ValueError("p in [0, 1) and 0 <= m <= n are required")
    w = p / (1.0 - p)

    def R(ws):
        e = np.zeros(m + 1)
        e[0] = 1.0
        for x in ws:
            e[1:] = e[1:] + x * e[:-1]
        return e

    total = R(w)[m]
    if total <= 0:
        raise ValueError("fewer patients with positive odds than successes")
    incl = np.array([w[c] * R(np.delete(w, c))[m - 1] / total if m >= 1 else 0.0 for c in range(n)])
    if not subsets:
        return incl
    import itertools
    subs = list(itertools.combinations(range(n), m))
    pr = np.array([np.prod(w[list(a)]) / total for a in subs])
    return incl, subs, pr


def case_odds(covariates, n_cases: int, n_ctrls: int, ridge: float = 0.0, max_iter: int = 50, tol: float = 1e-10) -> np.ndarray:
    """Fitted odds of being a case, for ``generate_weighted_permutations`` / ``gwaspa(case_odds=)``: a logistic regression of
    the labels (the columns < n_cases are the cases) on ``covariates`` ([n] or [n][k]) with an intercept, by iteratively
    reweighted least squares in numpy; returns p / (1 - p), float64 [n].  ``ridge``: an L2 penalty on the slopes (not the
    intercept), 0 by default.  Raises ValueError on separation (a fitted probability within 1e-8 of 0 or 1, or a
    coefficient beyond 30 in absolute value on standardised covariates) and on non-convergence, instead of returning huge
    odds silently.  The permutation p-values that follow are only as good as this model."""
    n_cases, n_ctrls = int(n_cases), int(n_ctrls)
    n = n_cases + n_ctrls
    X = np.asarray(covariates, dtype=np.float64)
    X = X.reshape(-1, 1) if X.ndim <= 1 else X
    if X.shape[0] != n or not np.isfinite(X).all():
        raise ValueError(f"covariates: finite values, one row per patient ({n})")
    if n_cases == 0 or n_ctrls == 0:
        raise ValueError("case_odds: needs at least one case and one control")
    # standardise the columns that vary: the fitted probabilities do not depend on it, the conditioning does
    sd = X.std(axis=0)
    Z = (X[:, sd > 0] - X[:, sd > 0].mean(axis=0)) / sd[sd > 0]
    A = np.hstack([np.ones((n, 1)), Z])
    y = (np.arange(n) < n_cases).astype(np.float64)
    pen = np.diag([0.0] + [float(ridge)] * Z.shape[1])
    beta = np.zeros(A.shape[1])
    beta[0] = np.log(n_cases / n_ctrls)
    for _ in range(int(max_iter)):
        eta = A @ beta
        mu = 1.0 / (1.0 + np.exp(-eta))
        wgt = mu * (1.0 - mu)
        if (np.abs(beta) > 30).any() or (mu < 1e-8).any() or (mu > 1 - 1e-8).any():
            raise ValueError("case_odds: the covariates separate cases from controls (perfectly or nearly): no finite fit; "
                             "drop a covariate or set ridge > 0")
        H = A.T @ (A * wgt[:, None]) + pen
        step = np.linalg.solve(H, A.T @ (y - mu) - pen @ beta)
        beta = beta + step
        if np.abs(step).max() < tol:
            mu = 1.0 / (1.0 + np.exp(-(A @ beta)))
            if (np.abs(beta) > 30).any() or (mu < 1e-8).any() or (mu > 1 - 1e-8).any():
                raise ValueError("case_odds: the covariates separate cases from controls (perfectly or nearly): no finite fit; "
                                 "drop a covariate or set ridge > 0")
            return mu / (1.0 - mu)
    raise ValueError(f"case_odds: no convergence in {int(max_iter)} IRLS steps")


def sequential_reference(null, obs, valid, hits: int, max_perms: int) -> Dict[str, np.ndarray]:
    """The definition of gcre_score_sets_sequential taken literally on a null matrix.  ``null``
    [sets][>= max_perms]: the null score of every set under permutations 0, 1, ... in order (the f32 values of
    ``score_sets``); ``obs`` [sets] the observed scores; ``valid`` [sets].  With e[r] = (float64(null[r]) >= obs), r <
    max_perms (a NaN never counts): a set with at least ``hits`` ones stops at the 1-based position of the ``hits``-th --
    ``n_perm`` that position, ``n_hit`` = hits, ``stopped`` 1; otherwise ``n_perm`` = max_perms, ``n_hit`` their number,
    ``stopped`` 0.  An invalid set gets ``n_hit`` = ``n_perm`` = -1.  Returns int64 ``n_hit``, ``n_perm`` and int32
    ``stopped``, [sets] each."""
    h, P = int(hits), int(max_perms)
    if h < 1 or P < 0:
        raise ValueError(f"sequential_reference: hits = {hits} must be at least 1 and max_perms = {max_perms} not negative")
    obs = np.asarray(obs, np.float64).reshape(-1)
    S = len(obs)
    nul = np.asarray(null).reshape(S, -1) if S else np.zeros((0, P))
    if nul.shape[1] < P:
        raise ValueError(f"sequential_reference: {nul.shape[1]} null scores per set for max_perms = {P}")
    ok = np.asarray(valid).reshape(-1)[:S] != 0
    n_hit, n_perm, stopped = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, np.int32)
    for s in range(S):
        if not ok[s]:
            n_hit[s] = n_perm[s] = -1
            continue
        with np.errstate(invalid="ignore"):
            e = nul[s, :P].astype(np.float64) >= obs[s]
        at = np.flatnonzero(e)
        if len(at) >= h:
            n_hit[s], n_perm[s], stopped[s] = h, int(at[h - 1]) + 1, 1
        else:
            n_hit[s], n_perm[s] = len(at), P
    return {"n_hit": n_hit, "n_perm": n_perm, "stopped": stopped}


def weighted_sequential_reference(null, obs, valid, hits: int, max_perms: int, attempts) -> Dict[str, object]:
    """The definition of gcre_score_sets_sequential_weighted (csrc/gcre_seq_weighted.h) taken literally.
    ``null`` / ``obs`` / ``valid`` as ``sequential_reference`` takes them, the null scores under the masks of
    ``weighted_masks``; ``attempts`` [>= max_perms][S]: its accepted attempts under the call's ``max_attempts``.  R
    (``first_left_over``) is the first permutation below ``max_perms`` with a WEIGHTED_NONE entry, or None.
    ``sequential_reference`` is applied to permutations 0 .. min(max_perms, R) - 1.  Without R: its dict as it is.  With R
    and every valid set stopped (``n_perm`` <= R): the same, complete.  Otherwise ``refused`` is True -- a valid set had
    not stopped in front of R; one with a NaN score never does -- and the counts are what the truncated range gave
    (``n_active`` says how many sets were still active).  Returns the dict plus ``first_left_over``, ``refused`` and
    ``n_active``."""
    P = int(max_perms)
    att = np.asarray(attempts)
    att = att.reshape(len(att), -1)
    if len(att) < P:
        raise ValueError(f"weighted_sequential_reference: {len(att)} rows of attempts for max_perms = {P}")
    bad = np.flatnonzero((att[:P] == WEIGHTED_NONE).any(axis=1))
    R = int(bad[0]) if len(bad) else None
    out: Dict[str, object] = dict(sequential_reference(null, obs, valid, hits, P if R is None else R))
    active = (np.asarray(valid).reshape(-1)[:len(out["stopped"])] != 0) & (out["stopped"] == 0)
    out["first_left_over"] = R
    out["n_active"] = int(active.sum()) if R is not None else 0
    out["refused"] = R is not None and bool(active.any())
    return out


def sequential_columns(seq, valid) -> Dict[str, np.ndarray]:
    """The SEQUENTIAL_COLUMNS from the ``seq`` records of ``JoinExec.sequential_tests`` (or the dict of
    ``sequential_reference``): ``SequentialPvalues`` = n_hit / n_perm, the set's nominal p-value by the n / K convention of
    this module (0 where no permutation reached the score; with the counts beside it a caller forms (n_hit + 1) / (n_perm +
    1) for the sets that did not stop); ``SequentialPerms`` and ``SequentialHits`` the two counts; ``SequentialStopped`` 1
    where the set reached its hits before the limit, else 0.  NaN for a set with an NA member (``valid`` 0 or a count < 0);
    the p-value is NaN also where no permutation was used."""
    n_hit = np.asarray(seq["n_hit"], np.int64).reshape(-1)
    n_perm = np.asarray(seq["n_perm"], np.int64).reshape(-1)
    stopped = np.asarray(seq["stopped"], np.int64).reshape(-1)
    ok = (np.asarray(valid).reshape(-1)[:len(n_hit)] != 0) & (n_hit >= 0) & (n_perm >= 0)
    nan = np.full(len(n_hit), np.nan)
    p = nan.copy()
    sel = ok & (n_perm > 0)
    p[sel] = n_hit[sel] / n_perm[sel]
    return {"SequentialPvalues": p, "SequentialPerms": np.where(ok, n_perm, nan), "SequentialHits": np.where(ok, n_hit, nan),
            "SequentialStopped": np.where(ok, stopped, nan)}


# stratified set scores: every stratum scored against its own table, the terms summed

STRATIFIED_COLUMNS = ["StratifiedScores", "StratifiedPvalues", "StratifiedFamilyPvalues"]
STRATUM_COLUMNS = ["Score", "Cases", "Controls"]


def strata_reference(sets, rows, signs, n_cases: int, strata, tables, masks, method: int) -> Dict[str, np.ndarray]:
    """The numpy statement of gcre_score_sets_strata, no device call.  ``rows``: the 0/1 carrier matrix
    [rows][patients], columns < n_cases the cases; ``sets`` / ``signs`` as ``JoinExec.score_sets`` takes them; ``strata``: one
    id per patient, any integers, stratum s = the s-th id in ascending order; ``tables``: one value table per stratum in that
    order, cells a table lacks reading as -1; ``masks`` bool [K][patients] from ``permutation_masks`` (None: no permutation).
    With P, N a set's unions (method 1: one union alone), Z_s the patients of stratum s and m a label mask -- the observed
    labels or a row of ``masks`` -- term_s(m) = T_s[|P & Z_s & m|][|P & Z_s \\ m|] (+ T_s[|N & Z_s \\ m|][|N & Z_s & m|],
    added in this order) and score(m) = ((+0.0 + term_0) + term_1) + ..., in ascending s.  Returns ``score`` [sets] (NaN
    for a set with an NA member), ``n_ge`` int64 [sets] = #{r : score(mask_r) >= score} as doubles (-1 for those), ``terms``
    [sets][S], ``counts`` int32 [sets][S][4] (cases_pos, ctrls_pos, cases_neg, ctrls_neg), ``null_scores`` [sets][K] and
    ``family_max`` [K], the maximum over the valid sets with NaN and negatives as +0."""
    d = np.asarray(rows) != 0
    n = d.shape[1]
    NSETS = len(sets)
    ids, st = np.unique(np.asarray(strata).reshape(-1), return_inverse=True)
    if len(st) != n:
        raise ValueError(f"strata: one id per patient ({n}), not {len(st)}")
    NS = len(ids)
    T = [np.asarray(t, np.float64) for t in tables]
    if len(T) != NS:
        raise ValueError(f"tables: one per stratum ({NS}), not {len(T)}")
    obs = np.arange(n) < n_cases
    mk = np.zeros((0, n), bool) if masks is None else np.asarray(masks, bool).reshape(-1, n)
    K = len(mk)
    Z = [st == s for s in range(NS)]
    size = [int(z.sum()) for z in Z]

    def summed(P, N, m):                       # P, N bool [n]; m bool [labels][n] -> (sum [labels], terms [S][labels], counts)
        total = np.zeros(len(m))               # +0.0
        terms, counts = [], []
        for s in range(NS):                    # the stated order
            a, b = (m & (P & Z[s])).sum(axis=1), (~m & (P & Z[s])).sum(axis=1)
            term = _vt_cell(T[s], size[s], a, b)
            k = [a, b, np.zeros_like(a), np.zeros_like(a)]
            if method == 2:
                c, e = (~m & (N & Z[s])).sum(axis=1), (m & (N & Z[s])).sum(axis=1)
                with np.errstate(invalid="ignore"):      # inf - inf
                    term = term + _vt_cell(T[s], size[s], c, e)
                k[2], k[3] = c, e
            with np.errstate(invalid="ignore"):
                total = total + term
            terms.append(term)
            counts.append(k)
        return total, terms, counts

    res = {"score": np.full(NSETS, np.nan), "n_ge": np.zeros(NSETS, np.int64), "terms": np.full((NSETS, NS), np.nan),
           "counts": np.zeros((NSETS, NS, 4), np.int32), "null_scores": np.full((NSETS, K), np.nan), "family_max": np.zeros(K)}
    for i in range(NSETS):
        mem = np.asarray(sets[i], dtype=np.int64).reshape(-1)
        if (mem < 0).any():
            res["n_ge"][i] = -1
            continue
        sg = np.ones(len(mem), np.int64) if signs is None else np.asarray(signs[i], dtype=np.int64).reshape(-1)
        neg = (sg == -1) if method == 2 else np.zeros(len(mem), bool)
        P = d[mem[~neg]].any(axis=0) if (~neg).any() else np.zeros(n, bool)
        N = d[mem[neg]].any(axis=0) if neg.any() else np.zeros(n, bool)
        total, terms, counts = summed(P, N, obs[None, :])
        res["score"][i] = total[0]
        res["terms"][i] = [t[0] for t in terms]
        res["counts"][i] = [[int(x[0]) for x in k] for k in counts]
        if K:
            null = summed(P, N, mk)[0]
            res["null_scores"][i] = null
            with np.errstate(invalid="ignore"):
                res["n_ge"][i] = int((null >= total[0]).sum())          # a NaN on either side never counts
                res["family_max"] = np.maximum(res["family_max"], np.where(null > 0, null, 0.0))
    return res


def stratified_columns(strata_records, valid, family_max, terms, counts, ids, perms: int) -> Dict[str, np.ndarray]:
    """The columns of the stratified scores from what ``JoinExec.strata_tests(family=True, terms=True)`` returns (or the dict
    entries of ``strata_reference``): ``strata_records`` with ``score`` and ``n_ge``, ``family_max`` [perms], ``terms``
    [sets][S], ``counts`` [sets][S][4]; ``ids``: the S stratum ids as the caller gave them, ascending.
    ``StratifiedScores``: the sum over the strata of each stratum's score against its own value table.
    ``StratifiedPvalues`` = n_ge / perms: a nominal permutation p-value of that sum, one set at a time (0 where no
    permutation reached it).  ``StratifiedFamilyPvalues``: single-step max-T over the call's sets, the share of the
    permutations whose maximum over all of them reaches the set's sum.  Per stratum ``Score.<id>`` (its term), ``Cases.<id>``
    and ``Controls.<id>`` (the set's carriers among its cases and controls, as ``Cases`` / ``Controls`` count them): these
    are descriptive, and no test of heterogeneity between the strata is attached.  NaN for a set with an NA member
    (``valid`` 0 or n_ge < 0); the p-values are NaN without permutations."""
    score = np.asarray(strata_records["score"], np.float64).reshape(-1)
    n_ge = np.asarray(strata_records["n_ge"], np.int64).reshape(-1)
    S = len(score)
    ok = (np.asarray(valid).reshape(-1)[:S] != 0) & (n_ge >= 0)
    K = int(perms)
    nan = np.full(S, np.nan)
    p, fp = nan.copy(), nan.copy()
    if K > 0:
        p[ok] = n_ge[ok] / K
        fm = np.asarray(family_max, np.float64).reshape(-1)[:K]
        with np.errstate(invalid="ignore"):
            fp[ok] = (fm[None, :] >= score[ok][:, None]).sum(axis=1) / K
    cols = {"StratifiedScores": np.where(ok, score, np.nan), "StratifiedPvalues": p, "StratifiedFamilyPvalues": fp}
    ids = list(np.asarray(ids).reshape(-1).tolist())
    tm = np.asarray(terms, np.float64).reshape(S, len(ids))
    cn = np.asarray(counts, np.int64).reshape(S, len(ids), 4)
    for j, name in enumerate(ids):
        cols[f"Score.{name}"] = np.where(ok, tm[:, j], np.nan)
        cols[f"Cases.{name}"] = np.where(ok, cn[:, j, 0] + cn[:, j, 2], np.nan)
        cols[f"Controls.{name}"] = np.where(ok, cn[:, j, 1] + cn[:, j, 3], np.nan)
    return cols


def _stratified_scores(rows, signs, data, n_cases, n_ctrls, method, n_permutations, strata, seed, device, case_odds=None):
    """strata_tests for ``score_paths``: on the rows the sets use, on a context of its own whose masks keep ``strata``;
    (strata records, family maxima, terms, counts, the ids ascending)."""
    from . import api
    used: Dict[int, int] = {}
    sets = [[-1 if r < 0 else used.setdefault(r, len(used)) for r in rs] for rs in rows]
    data = np.asarray(data)
    sub = data[list(used.keys())] if used else np.zeros((0, n_cases + n_ctrls), np.int32)
    ids, inv = np.unique(np.asarray(strata).reshape(-1), return_inverse=True)
    ex = api.JoinExec(method, n_cases, n_ctrls, n_permutations, device=device)
    try:
        ex.set_value_table(api.values_table(n_cases, n_ctrls))
        if n_permutations > 0:
            _draw_permutations(ex, seed, inv, case_odds)
        rec, sr, fam, terms, counts = ex.strata_tests(sets, sub, signs, strata=inv, family=True, terms=True)
        return sr, fam, terms, counts, ids
    finally:
        ex.close()


VARIABLE_THRESHOLD_COLUMNS = ["Sets", "Genes", "Scores", "NominalPvalues", "BestGenes", "BestThreshold", "AdaptiveScores",
                              "AdaptivePvalues", "AdaptiveFamilyPvalues"]


def _cut_lists(lists, cuts, flat_input: bool):
    """``cuts`` as one list of 0/1 flags per set of ``lists`` (None: every member), from either form ``prefix_tests`` takes."""
    if cuts is None:
        return [[1] * len(m) for m in lists]
    if flat_input:
        flat = (np.asarray(cuts).reshape(-1) != 0).astype(int).tolist()
        if len(flat) != sum(len(m) for m in lists):
            raise ValueError("cuts: one flag per member of every set")
        pos = np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(int)
        return [flat[pos[s]:pos[s + 1]] for s in range(len(lists))]
    ct = [[int(bool(x)) for x in m] for m in cuts]
    if len(ct) != len(lists) or any(len(a) != len(b) for a, b in zip(ct, lists)):
        raise ValueError("cuts: one flag per member of every set")
    return ct


def prefix_sets(sets, signs, cuts):
    """The steps of ``JoinExec.prefix_tests`` as sets of their own: ``(step_sets, step_signs, step_set)``.
    Step k of set s is its members up to and including the k-th member with a non-zero ``cuts`` flag (None: every member;
    the last member of a set always ends a step), with their signs; the steps of set 0 come first, then those of set 1.
    ``step_signs`` is None without ``signs``; ``step_set`` int64 [steps] names the set of every step.  ``sets`` / ``signs`` /
    ``cuts`` in either form the set entries take.  ``score_sets`` and ``family_tests`` on ``step_sets`` give what
    ``prefix_reference`` turns back into the call's results."""
    flat_input = isinstance(sets, tuple) and len(sets) == 2 and isinstance(sets[0], np.ndarray)
    lists, sg = _set_lists(sets, signs)
    ct = _cut_lists(lists, cuts, flat_input)
    step_sets, step_signs, step_set = [], [], []
    for s, m in enumerate(lists):
        for i in range(len(m)):
            if ct[s][i] or i + 1 == len(m):
                step_sets.append(list(m[:i + 1]))
                step_signs.append(list(sg[s][:i + 1]) if sg is not None else None)
                step_set.append(s)
    return step_sets, (step_signs if sg is not None else None), np.asarray(step_set, np.int64)


def prefix_reference(step_obs, step_null, step_set, n_sets: int, valid) -> Dict[str, np.ndarray]:
    """gcre_score_sets_prefix by its definition, in numpy, no device call.  ``step_obs`` float64 [steps] the
    observed score of every step, ``step_null`` float32 [steps][K] its null scores (already folded: what
    ``family_tests(null=True)`` returns for ``prefix_sets``), ``step_set`` [steps] the set of every step, ``valid`` [n_sets].
    Per set: ``best_step`` the smallest step that attains the maximum of the observed scores, NaN steps skipped (-1 if all
    are NaN); ``score`` the observed score of that step (NaN); ``null_max`` float32 [n_sets][K] the maximum over the set's
    steps per permutation; ``n_ge`` the permutations with (double) null_max >= score (0 for a NaN score).  A set that is not
    valid gets NaN, -1, a NaN row and n_ge -1."""
    obs = np.asarray(step_obs, np.float64).reshape(-1)
    null = np.asarray(step_null, np.float32)
    null = null.reshape(len(obs), -1) if null.size else np.zeros((len(obs), 0), np.float32)
    owner = np.asarray(step_set, np.int64).reshape(-1)
    ok = np.asarray(valid).reshape(-1) != 0
    K = null.shape[1]
    out = {"score": np.full(n_sets, np.nan), "best_step": np.full(n_sets, -1, np.int64), "n_ge": np.zeros(n_sets, np.int64),
           "null_max": np.full((n_sets, K), np.nan, np.float32)}
    for s in range(int(n_sets)):
        if not ok[s]:
            out["n_ge"][s] = -1
            continue
        rows = np.flatnonzero(owner == s)
        best = -1
        for k, r in enumerate(rows.tolist()):
            if obs[r] == obs[r] and (best < 0 or obs[r] > obs[rows[best]]):
                best = k
        t = null[rows].max(axis=0) if len(rows) else np.zeros(K, np.float32)
        out["null_max"][s] = t
        if best >= 0:
            out["best_step"][s] = best
            out["score"][s] = obs[rows[best]]
            out["n_ge"][s] = int((t.astype(np.float64) >= obs[rows[best]]).sum())
    return out


def adaptive_sequential_reference(step_obs, step_null, step_set, n_sets: int, valid, hits: int, max_perms: int,
                                  attempts=None) -> Dict[str, object]:
    """gcre_score_sets_prefix_sequential and gcre_score_sets_dose_sequential by their definition, in numpy, no device call
    (DESIGN.md §3.25): ``prefix_reference``'s ``score`` and ``null_max`` fed to ``sequential_reference``.  ``step_obs`` /
    ``step_null`` / ``step_set`` / ``valid`` as ``prefix_reference`` takes them -- the steps of ``prefix_sets`` or the level
    sets of ``dose_sets`` -- with ``step_null`` [steps][>= max_perms] under permutations 0, 1, ... in order.  A NaN step is
    skipped for the pick but still takes part in the null maximum (folded: 0); a set whose steps are all NaN has a NaN
    score and never counts.  With ``attempts`` [>= max_perms][S] (the accepted attempts of ``weighted_masks``) the rule is
    ``weighted_sequential_reference``'s, and the dict also holds ``first_left_over``, ``refused`` and ``n_active``.  Returns
    ``n_hit`` / ``n_perm`` / ``stopped`` [n_sets] plus ``score`` and ``best_step`` of ``prefix_reference``.  It is a nominal
    p-value of the maximum, one set at a time."""
    ref = prefix_reference(step_obs, step_null, step_set, n_sets, valid)
    null_max = ref["null_max"]
    if null_max.shape[1] == 0:
        null_max = np.zeros((int(n_sets), 0), np.float32)
    if attempts is None:
        out: Dict[str, object] = dict(sequential_reference(null_max, ref["score"], valid, hits, max_perms))
    else:
        out = weighted_sequential_reference(null_max, ref["score"], valid, hits, max_perms, attempts)
    out["score"] = ref["score"]
    out["best_step"] = ref["best_step"]
    return out


def threshold_order(set_genes, data):
    """The order and the cuts of the variable-threshold test (Price et al. 2010) for one set: ``(order, cuts)``.  ``set_genes``
    are rows of the 0/1 matrix ``data`` (-1 = NA); ``order`` int64 are positions of ``set_genes`` by ascending carrier total
    of their rows, ties by row (then by position; NA last), so the set's members in prefix order are
    ``np.asarray(set_genes)[order]`` and its signs likewise; ``cuts`` uint8 flag the last gene of every run of equal carrier
    total, so that genes of one total enter together: every step is "all genes with at most t carriers".  The carrier totals
    do not look at the labels, which is what makes the permutation test of the best step valid."""
    rows = np.asarray(set_genes, np.int64).reshape(-1)
    d = np.asarray(data)
    tot = np.array([int((d[r] != 0).sum()) if r >= 0 else np.iinfo(np.int64).max for r in rows.tolist()], np.int64)
    key_row = np.where(rows >= 0, rows, np.iinfo(np.int64).max)
    order = np.lexsort((np.arange(len(rows)), key_row, tot)).astype(np.int64)
    st = tot[order]
    cuts = np.ones(len(rows), np.uint8)
    if len(rows) > 1:
        cuts[:-1] = (st[1:] != st[:-1]) | (rows[order][:-1] < 0)
    return order, cuts


def variable_threshold_test(sets, genes: Sequence[str], data: np.ndarray, n_cases: int, n_ctrls: int, signed: bool = False,
                            names=None, threshold: float = 0.05, n_permutations: int = 100,
                            strata: Optional[Sequence[int]] = None, seed: int = 0, device: int = 0):
    """``variable_threshold_sequential_test`` without the sequential columns: the frame this function always returned (its
    docstring describes the test and the VARIABLE_THRESHOLD_COLUMNS)."""
    return variable_threshold_sequential_test(sets, genes, data, n_cases, n_ctrls, signed=signed, names=names, threshold=threshold,
                                              n_permutations=n_permutations, strata=strata, seed=seed, device=device, sequential=0)


def variable_threshold_sequential_test(sets, genes: Sequence[str], data: np.ndarray, n_cases: int, n_ctrls: int,
                                       signed: bool = False, names=None, threshold: float = 0.05, n_permutations: int = 100,
                                       strata: Optional[Sequence[int]] = None, seed: int = 0, device: int = 0, sequential: int = 0,
                                       sequential_hits: int = 20):
    """Variable-threshold test of gene sets the caller names (``JoinExec.prefix_tests``).  Every other set
    statistic scores a set's full union, so which genes count is decided by one carrier-frequency threshold chosen before
    the analysis; here a set's genes are ordered by carrier total (``threshold_order``), every prefix "all genes with at
    most t carriers" is scored, the best one is the statistic, and the same maximum is taken under every permutation.
    ``sets`` as ``parse_sets`` reads them; genes are looked up after ``preprocess_table(threshold)`` (pass a generous
    threshold: the test chooses its own); ``names``: one per set.  The masks are ``generate_permutations(seed, strata)``'s.

    One row per set, VARIABLE_THRESHOLD_COLUMNS: ``Genes`` the set's size; ``Scores`` / ``NominalPvalues`` of the full set,
    as ``score_paths`` gives them; ``BestGenes`` the size of the best prefix and ``BestThreshold`` the carrier total of its
    last gene; ``AdaptiveScores`` its score; ``AdaptivePvalues`` = n_ge / permutations, a self-contained permutation p-value
    of the maximum over the set's nested prefixes, one set at a time; ``AdaptiveFamilyPvalues`` single-step max-T of that
    statistic over the call's sets.  NaN for a set with a gene not found, a NaN score and 0 permutations.

    ``sequential`` = max_perms > 0 appends the SEQUENTIAL_COLUMNS of ``sequential_columns`` for the adaptive statistic
    (``JoinExec.prefix_sequential_tests``): every set is permuted until the maximum over its prefixes has
    reached ``AdaptiveScores`` ``sequential_hits`` times, with the seed and strata of the resident masks, in batches that are
    never resident, so ``sequential`` may be far above ``n_permutations``.  It is a nominal p-value of the maximum, one set
    at a time.  0, the default, returns the frame as it always was.  Not built: ``case_odds`` here (the API call takes
    ``odds``), a family-wise value of the sequential p-value."""
    import pandas as pd
    from . import api
    genes, data = preprocess_table(genes, data, threshold, n_cases, n_ctrls)
    data = np.asarray(data)
    _, rows, signs = parse_sets(sets, genes)
    S = len(rows)
    if names is not None and len(names) != S:
        raise ValueError(f"variable_threshold_test: {len(names)} names for {S} sets")
    K = int(n_permutations)
    ordered, osigns, cuts = [], [], []
    for rs, sg in zip(rows, signs):
        order, ct = threshold_order(rs, data)
        ordered.append(np.asarray(rs, np.int64)[order].tolist())
        osigns.append(np.asarray(sg, np.int64)[order].tolist())
        cuts.append(ct.tolist())
    used: Dict[int, int] = {}
    idx = [[-1 if r < 0 else used.setdefault(r, len(used)) for r in rs] for rs in ordered]
    sub = data[list(used.keys())] if used else np.zeros((0, n_cases + n_ctrls), np.int32)
    ex = api.JoinExec(2 if signed else 1, n_cases, n_ctrls, K, device=device)
    try:
        ex.set_value_table(api.values_table(n_cases, n_ctrls))
        if K > 0:
            ex.generate_permutations(seed, strata)
        rec, px, fam = ex.prefix_tests(idx, sub, osigns, cuts=cuts, family=True)
        seq = None
        if int(sequential) > 0:
            seq = ex.prefix_sequential_tests(idx, sub, osigns, cuts=cuts, hits=sequential_hits, max_perms=int(sequential), seed=seed,
                                             strata=strata)[2]
    finally:
        ex.close()
    nan = np.full(S, np.nan)
    ok = (rec["valid"] != 0) & (px["best_step"] >= 0) & (K > 0)
    tot = (data != 0).sum(axis=1) if len(data) else np.zeros(0, np.int64)
    best_thr = nan.copy()
    for s in np.flatnonzero(ok).tolist():
        best_thr[s] = tot[ordered[s][px["best_members"][s] - 1]]
    adaptive_p, family_p = nan.copy(), nan.copy()
    if K > 0:
        adaptive_p[ok] = px["n_ge"][ok] / K
        family_p[ok] = _tail_pvalues(fam, px["score"][ok])
    cols = {
        "Sets": [str(x) for x in names] if names is not None else [f"Set{s}" for s in range(S)],
        "Genes": np.array([len(r) for r in rows], np.int64),
        "Scores": rec["score"],
        "NominalPvalues": rec["pvalue"],
        "BestGenes": np.where(ok, px["best_members"], np.nan),
        "BestThreshold": best_thr,
        "AdaptiveScores": np.where(ok, px["score"], np.nan),
        "AdaptivePvalues": adaptive_p,
        "AdaptiveFamilyPvalues": family_p,
    }
    if seq is not None:
        cols.update(sequential_columns(seq, rec["valid"]))
        return pd.DataFrame(cols, columns=VARIABLE_THRESHOLD_COLUMNS + SEQUENTIAL_COLUMNS)
    return pd.DataFrame(cols, columns=VARIABLE_THRESHOLD_COLUMNS)


MULTI_HIT_COLUMNS = ["Sets", "Genes", "Scores", "NominalPvalues", "BestLevel", "BestCases", "BestControls", "MultiHitScores",
                     "MultiHitPvalues", "MultiHitFamilyPvalues"]


def dose_sets(sets, rows, signs, levels, signed):
    """The level rows of ``JoinExec.dose_tests`` written out in numpy as synthetic "genes", and the sets that score them
    (DESIGN.md §3.20): ``(level_rows, level_sets, level_signs, owner)``.  Per set and per level m of ``levels``, in that
    order: without ``signed`` (method 1) one row, the patients who carry at least m of the set's listed members -- the signs
    are ignored and a member listed twice counts twice -- and the one-member set of that row; with ``signed`` (method 2) two
    rows, the same count over the (+) members and over the (-) members of ``signs`` (None: all (+)), and the two-member set
    of the (+) row with sign +1 and the (-) row with sign -1.  ``level_rows`` int8 [rows made][patients] over all the columns
    of ``rows``; ``owner`` int64 [level sets] names the set of every level set.  A set with an NA member (-1) has no rows:
    its level sets hold -1 and are scored by nobody.  ``sets`` / ``signs`` in either form the set entries take.
    ``score_sets`` and ``family_tests(null=True)`` on ``level_sets``, folded by ``prefix_reference``, are what the call returns."""
    lists, sg = _set_lists(sets, signs)
    d = np.asarray(rows) != 0
    if d.ndim != 2:
        raise ValueError("dose_sets: rows is a 0/1 matrix [rows][patients]")
    lv = [int(m) for m in levels]
    n = d.shape[1]
    made, level_sets, level_signs, owner = [], [], [], []
    for s, m in enumerate(lists):
        valid = all(r >= 0 for r in m)
        if valid:
            g = np.ones(len(m), bool) if not signed or sg is None else np.asarray(sg[s]) != -1
            mem = np.asarray(m, np.int64)
            pos = d[mem[g]].sum(axis=0, dtype=np.int64) if g.any() else np.zeros(n, np.int64)
            neg = d[mem[~g]].sum(axis=0, dtype=np.int64) if (~g).any() else np.zeros(n, np.int64)
        for level in lv:
            if not valid:
                level_sets.append([-1, -1] if signed else [-1])
            else:
                level_sets.append([len(made), len(made) + 1] if signed else [len(made)])
                made.append(pos >= level)
                if signed:
                    made.append(neg >= level)
            level_signs.append([1, -1] if signed else [1])
            owner.append(s)
    level_rows = np.array(made, np.int8).reshape(len(made), n)
    return level_rows, level_sets, level_signs, np.asarray(owner, np.int64)


def pair_sets(rows):
    """All unordered pairs of the gene rows ``rows`` as two-member sets, in the order (0,1), (0,2), .., (1,2), ..: digenic
    screening is ``dose_tests(pair_sets(g), data, levels=[2], family=True)`` -- the patients who carry both genes."""
    g = [int(r) for r in rows]
    return [[g[i], g[j]] for i in range(len(g)) for j in range(i + 1, len(g))]


def multi_hit_test(sets, genes: Sequence[str], data: np.ndarray, n_cases: int, n_ctrls: int, signed: bool = False,
                   names=None, levels=(1, 2, 3), threshold: float = 0.05, n_permutations: int = 100,
                   strata: Optional[Sequence[int]] = None, seed: int = 0, device: int = 0):
    """``multi_hit_sequential_test`` without the sequential columns: the frame this function always returned (its docstring
    describes the test and the MULTI_HIT_COLUMNS)."""
    return multi_hit_sequential_test(sets, genes, data, n_cases, n_ctrls, signed=signed, names=names, levels=levels, threshold=threshold,
                                     n_permutations=n_permutations, strata=strata, seed=seed, device=device, sequential=0)


def multi_hit_sequential_test(sets, genes: Sequence[str], data: np.ndarray, n_cases: int, n_ctrls: int, signed: bool = False,
                              names=None, levels=(1, 2, 3), threshold: float = 0.05, n_permutations: int = 100,
                              strata: Optional[Sequence[int]] = None, seed: int = 0, device: int = 0, sequential: int = 0,
                              sequential_hits: int = 20):
    """Multi-hit test of gene sets the caller names (``JoinExec.dose_tests``).  Every other set statistic
    scores a set's union, where a patient with a variant in one gene of a pathway and a patient with variants in four count
    the same; here, per level m of ``levels``, the patients who carry at least m of the set's genes are scored, the best
    level is the statistic, and the same maximum is taken under every permutation.  ``sets`` as ``parse_sets`` reads them;
    genes are looked up after ``preprocess_table(threshold)``; a gene named twice in a set is kept once (its first sign);
    ``names``: one per set.  With ``signed`` the (+) and the (-) genes are counted apart.  The masks are
    ``generate_permutations(seed, strata)``'s.  The levels must not be chosen from the labels.

    One row per set, MULTI_HIT_COLUMNS: ``Genes`` the set's distinct genes; ``Scores`` / ``NominalPvalues`` of the full
    union, as ``score_paths`` gives them; ``BestLevel`` the best level and ``BestCases`` / ``BestControls`` the cases and
    controls of its (+) row; ``MultiHitScores`` its score; ``MultiHitPvalues`` = n_ge / permutations, a self-contained
    permutation p-value of the maximum over the levels, one set at a time; ``MultiHitFamilyPvalues`` single-step max-T of
    that statistic over the call's sets.  NaN for a set with a gene not found, a NaN score and 0 permutations.

    ``sequential`` = max_perms > 0 appends the SEQUENTIAL_COLUMNS of ``sequential_columns`` for the multi-hit statistic
    (``JoinExec.dose_sequential_tests``): every set is permuted until the maximum over its levels has reached
    ``MultiHitScores`` ``sequential_hits`` times, with the seed and strata of the resident masks, in batches that are never
    resident.  It is a nominal p-value of the maximum, one set at a time.  0, the default, returns the frame as it always
    was.  Not built: ``case_odds`` here (the API call takes ``odds``), a family-wise value of the sequential p-value."""
    import pandas as pd
    from . import api
    genes, data = preprocess_table(genes, data, threshold, n_cases, n_ctrls)
    data = np.asarray(data)
    names_of, rows, signs = parse_sets(sets, genes)
    S = len(rows)
    if names is not None and len(names) != S:
        raise ValueError(f"multi_hit_test: {len(names)} names for {S} sets")
    K = int(n_permutations)
    lv = api._dose_levels(levels)
    once, osigns = [], []
    for nm, rs, sg in zip(names_of, rows, signs):
        first = [i for i, x in enumerate(nm) if x not in nm[:i]]
        once.append([rs[i] for i in first])
        osigns.append([sg[i] for i in first])
    used: Dict[int, int] = {}
    idx = [[-1 if r < 0 else used.setdefault(r, len(used)) for r in rs] for rs in once]
    sub = data[list(used.keys())] if used else np.zeros((0, n_cases + n_ctrls), np.int32)
    ex = api.JoinExec(2 if signed else 1, n_cases, n_ctrls, K, device=device)
    try:
        ex.set_value_table(api.values_table(n_cases, n_ctrls))
        if K > 0:
            ex.generate_permutations(seed, strata)
        rec, ds, fam = ex.dose_tests(idx, sub, osigns, levels=lv, family=True)
        seq = None
        if int(sequential) > 0:
            seq = ex.dose_sequential_tests(idx, sub, osigns, levels=lv, hits=sequential_hits, max_perms=int(sequential), seed=seed,
                                           strata=strata)[2]
    finally:
        ex.close()
    nan = np.full(S, np.nan)
    ok = (rec["valid"] != 0) & (ds["best_index"] >= 0) & (K > 0)
    own_p, family_p = nan.copy(), nan.copy()
    if K > 0:
        own_p[ok] = ds["n_ge"][ok] / K
        family_p[ok] = _tail_pvalues(fam, ds["score"][ok])
    cols = {
        "Sets": [str(x) for x in names] if names is not None else [f"Set{s}" for s in range(S)],
        "Genes": np.array([len(r) for r in once], np.int64),
        "Scores": rec["score"],
        "NominalPvalues": rec["pvalue"],
        "BestLevel": np.where(ok, ds["best_level"], np.nan),
        "BestCases": np.where(ok, ds["cases_pos"], np.nan),
        "BestControls": np.where(ok, ds["ctrls_pos"], np.nan),
        "MultiHitScores": np.where(ok, ds["score"], np.nan),
        "MultiHitPvalues": own_p,
        "MultiHitFamilyPvalues": family_p,
    }
    if seq is not None:
        cols.update(sequential_columns(seq, rec["valid"]))
        return pd.DataFrame(cols, columns=MULTI_HIT_COLUMNS + SEQUENTIAL_COLUMNS)
    return pd.DataFrame(cols, columns=MULTI_HIT_COLUMNS)


def check_best_paths(results_df, genes: Sequence[str], data: np.ndarray, n_cases: int, n_ctrls: int, signed: bool,
                     device: int = 0):
    """checkBestPaths (R/CheckResults.R:2-89) on the device scorer without permutations: the dataset preprocessed with
    threshold 1 (:12-13), every row's SignedPaths rescored from the raw data, compared with ``Scores`` by ``!=`` (:76).
    Returns (passed, the rows that fail with the recomputed score, counts and checkBestPaths' half counts).  A row with an
    NA gene fails."""
    genes, data = preprocess_table(genes, data, 1, n_cases, n_ctrls)
    _, rows, signs = parse_sets(list(results_df["SignedPaths"]), genes)
    rec, _ = _score_sets(rows, signs, data, n_cases, n_ctrls, 2 if signed else 1, 0, None, 0, device)
    bad = ~(rec["score"] == results_df["Scores"].to_numpy(dtype=np.float64))
    out = results_df[bad].copy()
    out["CheckScores"] = rec["score"][bad]
    out["CheckCases"] = rec["cases"][bad]
    out["CheckControls"] = rec["ctrls"][bad]
    for f, c in (("cases_pos", "cases_pos"), ("ctrls_pos", "controls_pos"), ("cases_neg", "cases_neg"),
                 ("ctrls_neg", "controls_neg")):
        out[c] = rec[f][bad]
    return not bool(bad.any()), out


# ---------------------------------------------------------------------------------------------------------------
# per-gene best paths

GENE_LEVELS = ["1b", "2", "3", "4", "5"]   # the join whose top-k is lst1 .. lst5
GENE_COLUMNS = ["Gene", "Lengths", "Scores", "Pvalues", "Cases", "Controls", "SignedPaths", "Paths"]


def gene_slots(name: str, n_genes: int, n_genes2: int) -> int:
    """Slots of a level's tally: ranks in Ents2 at level 1, in Ents above."""
    return int(n_genes2 if name == "1b" else n_genes)


def gene_tables(levels, n_genes: int, n_genes2: int) -> Dict[str, Tuple[Optional[np.ndarray], Optional[np.ndarray]]]:
    """Per level name ("1b", "2", .., "5") the slot tables of a GeneTally: (genes0, genes1).  genes0[r] / genes1[r]
    are the genes a joined path inherits from row r of the join's paths0 / paths1 (int32 [rows][w], None = none), read
    from exactly the columns ``get_paths`` decodes for that level: a joined path (src, trg) touches
    genes0[src] | genes1[trg], the genes ``get_paths`` prints for ids (src + 1, trg + 1).  Slots are ranks in Ents
    (levels 2..5, ``n_genes`` of them) or in Ents2 (level 1, ``n_genes2``): ``gene_slots``."""
    rs, rt = np.asarray(levels.uids["3"].src, np.int32), np.asarray(levels.uids["3"].trg, np.int32)   # rels: row = relation
    r3 = levels.rels3
    a, b, c = (np.asarray(r3[k], np.int32) for k in ("srcuid", "trguid", "trguid2"))
    n2 = len(levels.uids["1b"].count)
    triple = np.stack([a, b, c], axis=1) if len(a) else np.zeros((0, 3), np.int32)
    out = {
        # level 1: paths0 is empty, paths1 row j is the data row of Ents2 gene data_inds["1b"][j]
        "1b": (None, np.asarray(levels.data_inds["1b"], np.int32).reshape(n2, 1)),
        "2": (None, np.stack([rs, rt], axis=1)),            # paths0 = the source gene's row, named by rels too
        "3": (np.stack([rs, rt], axis=1), rt.reshape(-1, 1)),
        "4": (triple, rt.reshape(-1, 1)),
        "5": (triple, np.stack([b, c], axis=1) if len(a) else np.zeros((0, 2), np.int32)),
    }
    for name, pair in out.items():
        for t in pair:
            if t is not None and t.size and (t.min() < 0 or t.max() >= gene_slots(name, n_genes, n_genes2)):
                raise ValueError(f"level {name}: a gene rank lies outside the {gene_slots(name, n_genes, n_genes2)} genes given")
    return out


def gene_best_reference(all_scores, all_cases, all_ctrls, uids, genes0, genes1, n_slots: int,
                        shard: Optional[Tuple[int, int]] = None) -> Dict[str, np.ndarray]:
    """The definition of the per-gene tally in plain numpy -- what gcre_gene_tally must return, bit for bit.

    ``all_scores`` / ``all_cases`` / ``all_ctrls``: one entry per joined path in ordinal order (ordinal p = path_idx[i] + j
    for uid row i, j < count[i]; src = i, trg = location[i] + j).  A path touches the slots genes0[src] and genes1[trg]
    (-1 and a None table: none).  Per slot: the touching path with the largest score, ties to the smallest ordinal
    (lexsort on (-score, ordinal)); only scores above -inf count, and only ordinals inside ``shard`` when given.  A slot
    nothing touches has score -inf, ordinal / src / trg -1 and counts 0."""
    count = np.maximum(np.asarray(uids.count, dtype=np.int64), 0)
    P = int(count.sum())
    src = np.repeat(np.arange(len(count), dtype=np.int64), count)
    first = np.cumsum(count) - count
    trg = np.repeat(np.asarray(uids.location, dtype=np.int64), count) + (np.arange(P, dtype=np.int64) - np.repeat(first, count))
    score = np.asarray(all_scores, dtype=np.float64)
    assert len(score) == P
    ok = score > -np.inf                       # (NaN compares false: not a score)
    if shard is not None:
        ords = np.arange(P)
        ok &= (ords >= shard[0]) & (ords < shard[1])
    out = {"score": np.full(n_slots, -np.inf), "ordinal": np.full(n_slots, -1, np.int64), "src": np.full(n_slots, -1, np.int32),
           "trg": np.full(n_slots, -1, np.int32), "cases": np.zeros(n_slots, np.int32), "ctrls": np.zeros(n_slots, np.int32)}
    slot_list, ord_list = [], []
    for table, rows in ((genes0, src), (genes1, trg)):
        if table is None:
            continue
        t = np.asarray(table, dtype=np.int64)
        for col in range(t.shape[1]):
            s = t[rows, col] if P else np.zeros(0, np.int64)
            keep = ok & (s >= 0)
            slot_list.append(s[keep])
            ord_list.append(np.flatnonzero(keep))
    if not slot_list:
        return out
    slots, ords = np.concatenate(slot_list), np.concatenate(ord_list)
    order = np.lexsort((ords, -score[ords], slots))     # by slot, then score descending, then ordinal ascending
    slots, ords = slots[order], ords[order]
    head = np.ones(len(slots), bool)
    head[1:] = slots[1:] != slots[:-1]
    g, p = slots[head], ords[head]
    out["score"][g] = score[p]
    out["ordinal"][g] = p
    out["src"][g] = src[p]
    out["trg"][g] = trg[p]
    out["cases"][g] = np.asarray(all_cases)[p]
    out["ctrls"][g] = np.asarray(all_ctrls)[p]
    return out


def gene_results(best: Dict[int, object], level_results: Dict[str, object], frames: Dict[str, Dict[str, np.ndarray]],
                 ents: Tuple[Sequence[int], Sequence[str]], ents2: Tuple[Sequence[int], Sequence[str]]):
    """Gene.Results: one row per (gene, length) with a finite best score.  ``best``: length L -> the tally of that level
    (anything with score / src / trg / cases / ctrls per slot: api.GeneBest, or gene_best_reference's dict); the other
    arguments as ``results_table`` takes them.  ``Pvalues`` compare the f64 score with the length's f32-rounded null
    maxima, like a GWASPA.Results row: a gene's best score is at most the level's maximum, so it is the family-wise
    p-value over all paths of that length.  Paths are decoded from (src, trg) by ``get_paths``.  Ordered like
    GWASPA.Results: p ascending, score descending, stable (lengths ascending, genes in Ents order)."""
    import pandas as pd

    per_level = {1: ("rels_data2", "rels_data2"), 2: ("rels_data", "rels"), 3: ("rels", "rels"),
                 4: ("rels3", "rels"), 5: ("rels3", "rels3")}
    cols: Dict[str, list] = {c: [] for c in GENE_COLUMNS}
    for L in sorted(best):
        b = best[L]
        get = (lambda k: np.asarray(b[k])) if isinstance(b, dict) else (lambda k: np.asarray(getattr(b, k)))
        score = get("score")
        sel = np.flatnonzero(np.isfinite(score))
        who = ents2 if L == 1 else ents
        ids = np.stack([get("src")[sel].astype(np.int64) + 1, get("trg")[sel].astype(np.int64) + 1], axis=1)
        f1, f2 = per_level[L]
        paths, signpaths = get_paths(ids, L, frames[f1], frames[f2])
        cols["Gene"] += [who[1][g] for g in sel.tolist()]
        cols["Lengths"] += [L] * len(sel)
        cols["Scores"] += score[sel].tolist()
        cols["Pvalues"] += _tail_pvalues(level_results[f"lst{L}"].null, score[sel]).tolist()
        cols["Cases"] += get("cases")[sel].tolist()
        cols["Controls"] += get("ctrls")[sel].tolist()
        cols["SignedPaths"] += uid_to_symbol(who[0], who[1], signpaths, signed=True)
        cols["Paths"] += uid_to_symbol(who[0], who[1], paths)
    df = pd.DataFrame(cols, columns=GENE_COLUMNS)
    p = df["Pvalues"].to_numpy(dtype=np.float64)
    order = np.lexsort((-df["Scores"].to_numpy(dtype=np.float64), np.where(np.isnan(p), np.inf, p)))
    return df.iloc[order].reset_index(drop=True)


def gene_summary(df):
    """Per gene the one row of Gene.Results to look at first: the smallest p-value, then the highest score, then the
    shortest length.  Genes in order of that row (p ascending, score descending)."""
    p = df["Pvalues"].to_numpy(dtype=np.float64)
    order = np.lexsort((df["Lengths"].to_numpy(), -df["Scores"].to_numpy(dtype=np.float64), np.where(np.isnan(p), np.inf, p)))
    ranked = df.iloc[order]
    return ranked[~ranked["Gene"].duplicated()].reset_index(drop=True)


# ---------------------------------------------------------------------------------------------------------------
# hit lists: every joined path at or above a score

def hits_reference(all_scores, all_cases, all_ctrls, uids, cutoff: float,
                   shard: Optional[Tuple[int, int]] = None) -> Dict[str, object]:
    """The definition of a hit list in plain numpy -- what gcre_hits must return, bit for bit.

    ``all_scores`` / ``all_cases`` / ``all_ctrls``: one entry per joined path in ordinal order, as ``gene_best_reference``
    takes them (ordinal p = path_idx[i] + j for uid row i, j < count[i]; src = i, trg = location[i] + j).  A path is a
    hit when its score is >= ``cutoff`` as doubles (so a cut-off of either zero admits both zeros) and above -inf (NaN
    compares false: not a score); only ordinals inside ``shard`` when given.  Returns "found" and the six arrays "score",
    "ordinal", "src", "trg", "cases", "ctrls", best first: score descending (the two zeros tie), then ordinal ascending."""
    count = np.maximum(np.asarray(uids.count, dtype=np.int64), 0)
    P = int(count.sum())
    src = np.repeat(np.arange(len(count), dtype=np.int64), count)
    first = np.cumsum(count) - count
    trg = np.repeat(np.asarray(uids.location, dtype=np.int64), count) + (np.arange(P, dtype=np.int64) - np.repeat(first, count))
    score = np.asarray(all_scores, dtype=np.float64)
    assert len(score) == P
    if np.isnan(cutoff):
        raise ValueError("hits_reference: the cut-off is NaN")
    with np.errstate(invalid="ignore"):
        ok = (score >= float(cutoff)) & (score > -np.inf)
    if shard is not None:
        ords = np.arange(P)
        ok &= (ords >= shard[0]) & (ords < shard[1])
    p = np.flatnonzero(ok)
    p = p[np.lexsort((p, -score[p]))]
    return {"found": int(len(p)), "score": score[p], "ordinal": p.astype(np.int64), "src": src[p].astype(np.int32),
            "trg": trg[p].astype(np.int32), "cases": np.asarray(all_cases)[p].astype(np.int32),
            "ctrls": np.asarray(all_ctrls)[p].astype(np.int32)}


def significance_cutoff(null_max, alpha: float) -> float:
    """The smallest double c such that a score is >= c exactly when its ``Pvalues`` entry -- #(null_max >= score) /
    len(null_max), the f64 score against the f32 maxima (``JoinResult.pvalues``) -- would be <= ``alpha``.

    With K maxima, m = the largest n in 0..K with n / K <= alpha (the very division ``pvalues`` makes, not
    floor(alpha * K): 0.29 * 100 is 28.999...) and nm the maxima as doubles in descending order, a score has at most m
    maxima at or above it exactly when it lies above nm[m]: the cut-off is nextafter(nm[m], +inf), and -inf when m == K
    (every score passes).  Null maxima are finite (table values), so the cut-off is."""
    nm = np.sort(np.asarray(null_max, dtype=np.float32).astype(np.float64).ravel())[::-1]
    K = len(nm)
    if K == 0:
        raise ValueError("significance_cutoff: no null maxima (0 permutations): there are no p-values to cut at")
    if np.isnan(alpha):
        raise ValueError("significance_cutoff: alpha is NaN")
    n = np.arange(K + 1, dtype=np.int64)
    ok = np.flatnonzero(n / K <= alpha)
    if len(ok) == 0:           # alpha < 0: no p-value is that small
        return float("inf")
    m = int(ok[-1])
    return float(np.nextafter(nm[m], np.inf)) if m < K else float("-inf")


def hit_gene_counts(hits, genes0, genes1, n_slots: int) -> np.ndarray:
    """How many hits run through each gene slot: int64 [n_slots].  ``hits``: anything with src / trg per hit (api.Hits, or
    ``hits_reference``'s dict); ``genes0`` / ``genes1``: the level's tables from ``gene_tables`` (None = none): a hit
    (src, trg) touches genes0[src] | genes1[trg].  A slot a path lists twice counts once."""
    get = (lambda k: np.asarray(hits[k])) if isinstance(hits, dict) else (lambda k: np.asarray(getattr(hits, k)))
    cols = []
    for table, rows in ((genes0, get("src")), (genes1, get("trg"))):
        if table is not None:
            t = np.asarray(table, dtype=np.int64)
            cols.append(t[rows.astype(np.int64)].reshape(len(rows), t.shape[1]))
    out = np.zeros(int(n_slots), np.int64)
    if not cols or len(cols[0]) == 0:
        return out
    s = np.sort(np.concatenate(cols, axis=1), axis=1)
    s[:, 1:][s[:, 1:] == s[:, :-1]] = -1          # the second listing of a slot on one path
    s = s[s >= 0]
    if s.size and s.max() >= int(n_slots):
        raise ValueError(f"hit_gene_counts: slot {int(s.max())} lies outside the {int(n_slots)} slots given")
    return np.bincount(s, minlength=int(n_slots)).astype(np.int64)


def hit_sets(found, tables, n_genes: int, n_genes2: int, nulls=None) -> Tuple[np.ndarray, np.ndarray]:
    """The member lists of every hit of every length, as ``api.JoinExec.clump_sets`` takes sets: ``(off, members)``, set s
    = members[off[s]:off[s + 1]], rows of ``vstack(data1, data2)``.  ``found``: length -> api.Hits (a list that overflowed
    has no records and contributes no sets); ``tables``: ``gene_tables``.  A hit (src, trg) of a level has the members
    genes0[src] | genes1[trg] with -1 dropped and a slot listed twice kept once, ascending; the slots of levels 2..5 are
    ranks in Ents (``n_genes`` rows of data1), those of level 1 ranks in Ents2, offset by ``n_genes`` into the stacked
    matrix.  The sets are in the row order in which ``results_table`` lays out the same lists (``Hits.as_join_result``):
    p-value ascending, then score descending, stable over the lengths one after the other, each from its worst hit to its
    best; ``nulls``: length -> the level's null maxima, which the p-values compare with as ``JoinResult.pvalues`` does
    (None: no p-values, as with no permutations).  Whole-array numpy: no strings, no loop over hits."""
    lengths = sorted(int(L) for L in found)
    blocks, scores, pvals = [], [], []
    for L in lengths:
        h = found[L]
        name = GENE_LEVELS[L - 1]
        src = np.asarray(h.src, np.int64)[::-1]
        trg = np.asarray(h.trg, np.int64)[::-1]
        sc = np.asarray(h.score, np.float64)[::-1]
        cols = []
        for table, idx in zip(tables[name], (src, trg)):
            if table is not None:
                t = np.asarray(table, np.int64)
                cols.append(t[idx].reshape(len(idx), t.shape[1]))
        m = np.concatenate(cols, axis=1) if cols else np.zeros((len(sc), 0), np.int64)
        slots = gene_slots(name, n_genes, n_genes2)
        if m.size and m.max() >= slots:
            raise ValueError(f"hit_sets: length {L}: slot {int(m.max())} lies outside the {slots} slots given")
        if name == "1b":
            m = np.where(m >= 0, m + int(n_genes), -1)
        blocks.append(m)
        scores.append(sc)
        t = None if nulls is None else np.sort(np.asarray(nulls[L], np.float32).astype(np.float64))
        pvals.append(np.full(len(sc), np.nan) if t is None or len(t) == 0 else
                     (len(t) - np.searchsorted(t, sc, side="left")) / len(t))
    n = sum(len(b) for b in blocks)
    if n == 0:
        return np.zeros(1, np.int64), np.zeros(0, np.int32)
    w = max(b.shape[1] for b in blocks)
    m = np.full((n, w), -1, np.int64)
    at = 0
    for b in blocks:
        m[at:at + len(b), :b.shape[1]] = b
        at += len(b)
    sc, p = np.concatenate(scores), np.concatenate(pvals)
    m = m[np.lexsort((-sc, np.where(np.isnan(p), np.inf, p)))]     # results_table's order
    m = np.sort(m, axis=1)
    m[:, 1:][m[:, 1:] == m[:, :-1]] = -1                            # the second listing of a slot on one path
    keep = m >= 0
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(keep.sum(axis=1))
    return off, np.ascontiguousarray(m[keep], dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------
# null exceedance counts, permutation FDR

FDR_COLUMNS = ["ExpectedFalse", "FDR", "Qvalues"]


def _vt_cell(VT, n, a, b):
    """VT[a][b] as the device reads its copy of the value table: -1 outside the caller's table and beyond n patients."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if VT.size == 0:                                       # a table without a cell: everything is outside
        return np.full(np.broadcast(a, b).shape, -1.0)
    ok = (a >= 0) & (b >= 0) & (a <= n) & (b <= n) & (a < VT.shape[0]) & (b < VT.shape[1])
    return np.where(ok, VT[np.clip(a, 0, VT.shape[0] - 1), np.clip(b, 0, VT.shape[1] - 1)], -1.0)


def _vt_max(VT, n, a, b):
    """compute_value_table_max (methods.h:110-118): max(VT[a][b], VT[b][a]) with std::max semantics."""
    x, y = _vt_cell(VT, n, a, b), _vt_cell(VT, n, b, a)
    return np.where(x < y, y, x)


def _fold_f32(x):
    """The f32 value a join's null kernels fold into their maxima: rounded to f32, NaN and negatives as +0."""
    f = np.asarray(x, np.float64).astype(np.float32)
    return np.where(f > 0, f, np.float32(0)).astype(np.float32)


def _unpack_rows(rows, halves: int, n: int) -> np.ndarray:
    """Packed path rows uint64 [rows][halves * W] (W >= ceil(n / 64) words per half) -> bool [halves][rows][n]."""
    r = np.ascontiguousarray(rows, dtype="<u8")
    r = r.reshape(len(r), halves, -1)
    bits = np.unpackbits(r.view(np.uint8).reshape(len(r), halves, -1), axis=2, bitorder="little")[:, :, :n]
    return np.ascontiguousarray(np.moveaxis(bits, 1, 0)).astype(bool)


def _n_masks(masks, n: int, window=None) -> int:
    """The permutations ``_join_null_blocks`` walks for these masks and this window."""
    mk = np.asarray(masks)
    K = (mk.size // n if mk.dtype == bool else len(mk.reshape(len(mk), -1))) if mk.size else 0
    return len(range(K)[window[0]:window[1]]) if window is not None else K


def _join_null_blocks(method, n_cases: int, n_ctrls: int, uids, rows0, rows1, value_table, masks,
                      shard: Optional[Tuple[int, int]] = None, window: Optional[Tuple[int, int]] = None):
    """The null matrix of a join in blocks of joined paths, as ``exceed_reference`` states it: yields
    (lo, src, trg, scores, null) per block -- the block's first scored path, its (uid row, paths1 row) pairs, the observed
    scores (f64) and null[p][r] (f32 [paths][K], the value the null kernels fold into their maxima).  An empty join yields
    nothing."""
    M = 1 if method in (1, "method1") else 2
    n = int(n_cases) + int(n_ctrls)
    VT = np.asarray(value_table, np.float64)
    mk = np.asarray(masks)
    if mk.dtype != bool:
        mk = _unpack_rows(mk, 1, n)[0] if mk.size else np.zeros((0, n), bool)
    mk = mk.reshape(-1, n)
    if window is not None:
        mk = mk[window[0]:window[1]]
    K = len(mk)
    mf = mk.astype(np.float32)
    count = np.maximum(np.asarray(uids.count, dtype=np.int64), 0)
    P = int(count.sum())
    src = np.repeat(np.arange(len(count), dtype=np.int64), count)
    first = np.cumsum(count) - count
    trg = np.repeat(np.asarray(uids.location, dtype=np.int64), count) + (np.arange(P, dtype=np.int64) - np.repeat(first, count))
    b0, b1 = (0, P) if shard is None else (max(0, min(int(shard[0]), P)), max(0, min(int(shard[1]), P)))
    b1 = max(b0, b1)
    src, trg = src[b0:b1], trg[b0:b1]
    r0, r1 = _unpack_rows(rows0, M, n), _unpack_rows(rows1, M, n)
    keep = np.ones(len(src), bool)
    if M == 2:
        signs, L = np.asarray(uids.signs, np.int64), int(uids.path_length)
        sg = signs[src] if L > 3 else signs[trg] if L < 3 else np.where(signs[src] + signs[trg] == 0, -1, 1)
        keep = sg == 1
    case = np.arange(n) < int(n_cases)
    step = max(1, int(4e6 // max(K, 1)), 1)
    step = min(step, 1 << 16)
    for lo in range(0, len(src), step):
        s_, t_ = src[lo:lo + step], trg[lo:lo + step]
        if M == 1:
            bp = r0[0][s_] | r1[0][t_]
            tot = bp.sum(axis=1)
            scores = _vt_cell(VT, n, (bp & case).sum(axis=1), (bp & ~case).sum(axis=1))
            a = (bp.astype(np.float32) @ mf.T).astype(np.int64)            # exact: counts < 2^24
            null = _fold_f32(_vt_cell(VT, n, a, tot[:, None] - a))
        else:
            k_ = keep[lo:lo + step, None]
            bp = r0[0][s_] | np.where(k_, r1[0][t_], r1[1][t_])
            bn = r0[1][s_] | np.where(k_, r1[1][t_], r1[0][t_])
            tp, tn = bp.sum(axis=1), bn.sum(axis=1)
            scores = (_vt_cell(VT, n, (bp & case).sum(axis=1), (bp & ~case).sum(axis=1)) +
                      _vt_cell(VT, n, (bn & ~case).sum(axis=1), (bn & case).sum(axis=1)))
            a = (bp.astype(np.float32) @ mf.T).astype(np.int64)
            b = (bn.astype(np.float32) @ mf.T).astype(np.int64)
            null = _fold_f32(_vt_max(VT, n, a, tp[:, None] - a) + _vt_max(VT, n, tn[:, None] - b, b))
        yield lo, s_, t_, scores, null.reshape(len(s_), K)


def exceed_reference(method, n_cases: int, n_ctrls: int, uids, rows0, rows1, value_table, masks, thresholds,
                     shard: Optional[Tuple[int, int]] = None, window: Optional[Tuple[int, int]] = None,
                     per_permutation: bool = False) -> Dict[str, object]:
    """The definition of a join's exceedance counts in plain numpy -- what gcre_exceed must return, bit for bit.

    ``uids``: the join index (count / location / signs / path_length); ``rows0`` / ``rows1``: the packed rows of paths0 and
    paths1 (uint64 [rows][method * W]: the (+) half, then for the signed method the (-) half); ``masks``: the permutations'
    case masks, packed uint64 [K][W] or bool [K][n]; ``thresholds``: any order.  Joined path p = (uid row i, paths1 row
    location[i] + j) is paths0[i] | paths1[..], the added row's halves swapped when the signed method's relation is not
    positive (UidRelSet::need_flip).  Per permutation r its null value is the f32 the null kernels fold into their maxima
    -- method 1: VT[c][tot - c] for c carriers among the mask's cases; method 2: vtmax[a][P - a] + vtmax[N - b][b] added in
    f64 --, rounded to f32, NaN and negatives as 0.  exceed[j] counts the (p, r) with (double)null >= thresholds[j] over the
    scored paths (``shard``) and the permutations of ``window``; observed[j] the scored paths whose observed score (above
    -inf) is >= thresholds[j].  Returns {"exceed", "observed" (uint64), "perms", "paths", "scores" (f64 per scored path)}.

    ``per_permutation``: the result also has "perm_counts", uint64 [m][K] over the window's K permutations (column r is
    permutation window[0] + r), in the order of the thresholds given: perm_counts[j][r] counts the scored paths p with
    (double)null[p][r] >= thresholds[j], from the same null matrix -- what gcre_exceed_read_perm_counts must return for those
    permutations, exactly.  Every row sums to exceed[j]."""
    thr = np.asarray(thresholds, np.float64).ravel()
    if np.isnan(thr).any():
        raise ValueError("a threshold is NaN")
    K = _n_masks(masks, int(n_cases) + int(n_ctrls), window)
    order = np.argsort(thr, kind="stable")
    ts = thr[order]
    exceed_sorted = np.zeros(len(thr), np.uint64)
    perm_sorted = np.zeros((len(thr), K), np.uint64) if per_permutation else None
    parts = []
    for _lo, _s, _t, sc_, null in _join_null_blocks(method, n_cases, n_ctrls, uids, rows0, rows1, value_table, masks,
                                                     shard, window):
        parts.append(sc_)
        v = np.sort(null.astype(np.float64).ravel())
        exceed_sorted += (len(v) - np.searchsorted(v, ts, side="left")).astype(np.uint64)
        if per_permutation and null.size:
            reached = np.searchsorted(ts, null.astype(np.float64), side="right")   # thresholds <= the value: 0 .. m
            h = np.bincount((reached * K + np.arange(K)[None, :]).ravel(), minlength=(len(ts) + 1) * K).reshape(-1, K)
            perm_sorted += np.cumsum(h[::-1], axis=0)[::-1][1:].astype(np.uint64)   # row j: values reaching more than j
    scores = np.concatenate(parts).astype(np.float64) if parts else np.zeros(0, np.float64)
    sc = np.sort(scores[scores > -np.inf])                               # (NaN compares false: not a score)
    observed_sorted = (len(sc) - np.searchsorted(sc, ts, side="left")).astype(np.uint64)
    exceed, observed = np.zeros(len(thr), np.uint64), np.zeros(len(thr), np.uint64)
    exceed[order], observed[order] = exceed_sorted, observed_sorted
    out = {"exceed": exceed, "observed": observed, "perms": K, "paths": len(scores), "scores": scores}
    if per_permutation:
        out["perm_counts"] = np.zeros((len(thr), K), np.uint64)
        out["perm_counts"][order] = perm_sorted
    return out


def fdr_columns(thresholds, exceed, observed, perms: int) -> Dict[str, np.ndarray]:
    """Per threshold, in the order given: the per-family error rate PFER = exceed / B (the number of paths a permutation
    pushes to the threshold or beyond, on average over all B permutations drawn -- no identity permutation is added), the
    permutation FDR = min(1, PFER / observed) with pi0 = 1 (Storey-Tibshirani / SAM), and the q-value = the smallest FDR
    among the thresholds that are not larger (the monotone step: a q-value never falls as the threshold does).  NaN where
    nothing is observed at the threshold or B = 0; NaN entries do not take part in a q-value.  Equal thresholds get equal
    rows.  Returns {"ExpectedFalse", "FDR", "Qvalues"}."""
    t = np.asarray(thresholds, np.float64).ravel()
    e, o = np.asarray(exceed, np.float64).ravel(), np.asarray(observed, np.float64).ravel()
    B = int(perms)
    with np.errstate(divide="ignore", invalid="ignore"):
        pfer = e / B if B > 0 else np.full(len(t), np.nan)
        fdr = np.where(o > 0, np.minimum(1.0, pfer / o), np.nan)
    # thresholds ascending (ties kept together: equal thresholds have equal counts), running minimum ignoring NaN
    order = np.argsort(t, kind="stable")
    run = np.minimum.accumulate(np.where(np.isnan(fdr[order]), np.inf, fdr[order]))
    # a tie's first member has not seen its later members: equal thresholds carry equal FDRs, so nothing changes
    q = np.empty(len(t))
    q[order] = np.where(np.isnan(fdr[order]), np.nan, run)
    return {"ExpectedFalse": pfer, "FDR": fdr, "Qvalues": q}


EXCEED_PERM_CELLS = 1 << 26   # api.EXCEED_PERM_CELLS: thresholds x permutations of one object's per-permutation counts


def false_count_names(ks=(2, 5, 10)) -> List[str]:
    """The columns of ``false_count_columns``, in order."""
    return ["MedianFalse", "FDRmedian", "FalseBound", "FDPbound"] + [f"kFWER.{int(k)}" for k in ks]


def false_count_columns(thresholds, perm_counts, observed, perms: int, ks=(2, 5, 10), alpha: float = 0.05
                        ) -> Dict[str, np.ndarray]:
    """Per threshold, in the order given, from V = ``perm_counts`` (uint64 [m][B]: V[j][r] = paths permutation r pushes to
    threshold j or beyond; ``Exceedances.perm_counts``) and ``observed`` (paths whose observed score reaches it), B = ``perms``
    = the number of permutations V's columns stand for:

      MedianFalse   the ceil(B / 2)-th smallest of V[j][.]: the median number of false positives of a permutation
      FDRmedian     min(1, MedianFalse / observed): SAM's FDR estimate
      FalseBound    the ceil((1 - alpha) B)-th smallest (the rank is taken exactly, on alpha's shortest decimal form, and
                    is at least 1): the count a permutation does not exceed with frequency >= 1 - alpha
      FDPbound      min(1, FalseBound / observed): the same as a proportion of the rows at or above the threshold
      kFWER.<k>     #{r : V[j][r] >= k} / B for every k of ``ks``: how often at least k paths reach the threshold

    Everything is integer order statistics and one division: deterministic.  What they are: single-threshold permutation
    quantiles under the complete null (every path null, pi0 = 1) -- the distribution over permutations whose mean is
    ``fdr_columns``' ExpectedFalse.  What they are NOT: simultaneous over thresholds (reading the bound at the threshold
    that looks best is a selection the bound does not cover), nor a confidence statement about this data set's false
    discovery proportion when some paths are truly associated.  kFWER.1 is the ``Pvalues`` column (the family-wise p-value
    from the null maxima, no identity permutation added).  NaN where ``fdr_columns`` gives NaN: B = 0 for every column,
    observed = 0 for the two ratios.  Equal thresholds get equal rows."""
    t = np.asarray(thresholds, np.float64).ravel()
    m, B = len(t), int(perms)
    o = np.asarray(observed, np.float64).ravel()
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"alpha must be in [0, 1], not {alpha}")
    names = false_count_names(ks)
    if B <= 0:
        return {c: np.full(m, np.nan) for c in names}
    V = np.asarray(perm_counts, np.uint64).reshape(m, -1)
    if V.shape[1] != B:
        raise ValueError(f"perm_counts has {V.shape[1]} permutations per threshold, perms says {B}")
    Vs = np.sort(V, axis=1)
    r_med = (B + 1) // 2                                                 # ceil(B / 2) >= 1
    # ceil((1 - alpha) B) in exact arithmetic on the decimal alpha given, clamped into 1 .. B
    f = (1 - Fraction(str(float(alpha)))) * B
    r_bnd = min(B, max(1, -((-f.numerator) // f.denominator)))
    med, bnd = Vs[:, r_med - 1].astype(np.float64), Vs[:, r_bnd - 1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"MedianFalse": med, "FDRmedian": np.where(o > 0, np.minimum(1.0, med / o), np.nan),
               "FalseBound": bnd, "FDPbound": np.where(o > 0, np.minimum(1.0, bnd / o), np.nan)}
    for k in ks:
        out[f"kFWER.{int(k)}"] = (V >= np.uint64(max(int(k), 0))).sum(axis=1).astype(np.float64) / B
    return out


# ---------------------------------------------------------------------------------------------------------------
# step-down max-T p-values of a level's top rows

STEPDOWN_COLUMNS = ["PvaluesStepDown"]


def stepdown_reference(method, n_cases: int, n_ctrls: int, uids, rows0, rows1, value_table, masks, top) -> Dict[str, object]:
    """The definition of a join's step-down max-T counts (Westfall & Young 1993, Alg. 4.1) in plain numpy -- what
    gcre_exceed_stepdown must return, exactly.  The join is given as for ``exceed_reference``; ``top`` = (src, trg, scores)
    of its top rows: joined path (uid row src, paths1 row trg) and its observed score tau, all finite, sentinel rows left
    out, every pair a different joined path of the join.

    With null[p][r] as ``exceed_reference`` states it and D_j = {i : tau_i > tau_j} (f64: rows with equal scores do not
    exclude one another), u_j[r] = the maximum of null[p][r] over the joined paths p that are not rows of D_j, and
    n_ge[j] = #{r : (double)u_j[r] >= tau_j}.  It is computed from the successive maxima themselves: the null matrix in
    blocks of paths, a running maximum over the paths that are not top rows, the top rows' own null rows, and per row the
    maximum of the rest with the rows that are not better -- not through the counts V - E the device uses.

    Returns {"n_ge" (int64 [m], in the order of ``top``), "single" (int64 [m]: #{r : null_max[r] >= tau_j}, the single-step
    count), "null_max" (f32 [K]), "top_null" (f32 [m][K]: the rows' own null values), "scores" (f64 [m]: the rows' observed
    scores as the join computes them), "perms"}."""
    src_t = np.asarray(top[0], np.int64).ravel()
    trg_t = np.asarray(top[1], np.int64).ravel()
    tau = np.asarray(top[2], np.float64).ravel()
    m = len(tau)
    if not (len(src_t) == len(trg_t) == m):
        raise ValueError("top: one src, trg and score per row")
    if not np.isfinite(tau).all():
        raise ValueError("top: every score must be finite (leave the sentinel rows out)")
    where = {}
    for j, key in enumerate(zip(src_t.tolist(), trg_t.tolist())):
        if key in where:
            raise ValueError(f"top: rows {where[key]} and {j} are the same joined path {key}")
        where[key] = j
    K = _n_masks(masks, int(n_cases) + int(n_ctrls))
    rest = np.zeros(K, np.float32)                      # null values are >= 0
    top_null = np.zeros((m, K), np.float32)
    top_score = np.full(m, np.nan)
    found = np.zeros(m, bool)
    for _lo, s_, t_, sc_, null in _join_null_blocks(method, n_cases, n_ctrls, uids, rows0, rows1, value_table, masks):
        is_top = np.zeros(len(s_), bool)
        for i, key in enumerate(zip(s_.tolist(), t_.tolist())):
            j = where.get(key)
            if j is not None:
                is_top[i], found[j] = True, True
                top_null[j], top_score[j] = null[i], sc_[i]
        if (~is_top).any() and K:
            rest = np.maximum(rest, null[~is_top].max(axis=0))
    if not found.all():
        raise ValueError(f"top: row {int(np.flatnonzero(~found)[0])} is not a joined path of the join")
    null_max = np.maximum(rest, top_null.max(axis=0)) if m and K else rest.copy()
    n_ge = np.zeros(m, np.int64)
    for j in range(m):
        inside = tau <= tau[j]                          # the rows that stay in the family: not strictly better than row j
        u = np.maximum(rest, top_null[inside].max(axis=0)) if K else rest
        n_ge[j] = int((u.astype(np.float64) >= tau[j]).sum())
    single = (null_max.astype(np.float64)[None, :] >= tau[:, None]).sum(axis=1).astype(np.int64)
    return {"n_ge": n_ge, "single": single, "null_max": null_max, "top_null": top_null, "scores": top_score, "perms": K}


def stepdown_columns(thresholds, n_ge, perms: int) -> Dict[str, np.ndarray]:
    """Per threshold, in the order given: ``PvaluesStepDown`` = the largest raw step-down value n_ge[i] / B among the rows i
    whose threshold is at least this one (the monotone step of Westfall & Young's algorithm: a p-value never falls as the
    score does; equal thresholds get equal values).  B = ``perms``; NaN when B = 0.  No identity permutation is added, as in
    ``Pvalues``.  Returns {"PvaluesStepDown"}."""
    t = np.asarray(thresholds, np.float64).ravel()
    g = np.asarray(n_ge, np.float64).ravel()
    if len(g) != len(t):
        raise ValueError(f"{len(g)} counts for {len(t)} thresholds")
    B = int(perms)
    if B <= 0:
        return {"PvaluesStepDown": np.full(len(t), np.nan)}
    order = np.argsort(-t, kind="stable")               # descending; a tie group takes the value at its last member
    run = np.maximum.accumulate(g[order] / B)
    ts = t[order]
    last = np.searchsorted(-ts, -ts, side="right") - 1
    out = np.empty(len(t))
    out[order] = run[last]
    return {"PvaluesStepDown": out}


# ---------------------------------------------------------------------------------------------------------------
# carrier overlaps, clumping, conditional scores

CLUMP_COLUMNS = ["Clump", "ClumpLead", "ClumpSize", "LeadOverlap", "SharedCases", "SharedControls"]
RESIDUAL_COLUMNS = ["ResidualScores", "ResidualCases", "ResidualControls", "ResidualPvalues"]


def carrier_rows(sets, rows, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """(C, valid): C bool [S][n], row s = the OR of ALL members of set s (row indices of the 0/1 matrix ``rows``, whatever
    their signs: a patient who carries a variant in any gene of the path); valid[s] False, and the row all False, for a
    set with an NA member (-1)."""
    d = np.asarray(rows)[:, :n] != 0 if len(rows) else np.zeros((0, n), bool)
    C = np.zeros((len(sets), n), bool)
    valid = np.ones(len(sets), bool)
    for s, members in enumerate(sets):
        m = [int(x) for x in members]
        if any(x < 0 for x in m):
            valid[s] = False
            continue
        for x in m:
            C[s] |= d[x]
    return C, valid


def overlap_reference(sets, rows, n_cases: int, n_ctrls: int, a=None, b=None) -> Tuple[np.ndarray, np.ndarray]:
    """gcre_set_overlap by its definition, in numpy: size int32 [S][2] = carriers of every set among the cases (columns
    < n_cases) and the controls, (-1, -1) with an NA member; both int32 [na][nb][2] = the patients sets a[i] and b[j]
    share, zeros where either has an NA member.  ``a`` / ``b``: set indices, None = every set."""
    n = n_cases + n_ctrls
    C, valid = carrier_rows(sets, rows, n)
    S = len(sets)
    size = np.stack([C[:, :n_cases].sum(axis=1), C[:, n_cases:].sum(axis=1)], axis=1).astype(np.int32).reshape(S, 2)
    size[~valid] = -1
    ia = np.arange(S) if a is None else np.asarray(a, np.int64).reshape(-1)
    ib = np.arange(S) if b is None else np.asarray(b, np.int64).reshape(-1)
    A, B = C[ia].astype(np.float32), C[ib].astype(np.float32)   # counts <= 65,536 patients: exact in f32
    both = np.stack([A[:, :n_cases] @ B[:, :n_cases].T, A[:, n_cases:] @ B[:, n_cases:].T], axis=2).astype(np.int32)
    return size, both.reshape(len(ia), len(ib), 2)


def clump_rows(order, size, both_of, r: float, measure: str = "jaccard", patients: str = "all", block: int = 256):
    """Greedy clumping of rows by shared carriers, separable from the device.  ``order``: the rows to clump, best first;
    ``size`` [S][2] their carriers (cases, controls); ``both_of(leads, others)`` -> [len(leads)][len(others)][2] shared
    carriers.  Walk ``order``: a row not yet assigned becomes the lead of a new clump (numbered 0, 1, .. in that order) and
    every later unassigned row whose overlap with it is >= r joins.  ``patients``: "all" counts cases + controls, "cases"
    the cases only.  ``measure``: "jaccard" = both / (|A| + |B| - both), "containment" = both / min(|A|, |B|), in float64,
    0.0 where the denominator is 0 (so a lead without carriers stays alone).  Counts are asked for in blocks of ``block``
    candidate leads against all rows after them; the result does not depend on it.

    Returns (clump, lead, value, shared): per row of ``size`` the clump id (-1 outside ``order``), the lead's row (-1
    outside ``order``; a lead names itself), the measure against the lead (NaN on leads and outside ``order``) and the
    shared (cases, controls) against the lead (-1 on leads and outside ``order``)."""
    if not 0 < r <= 1:
        raise ValueError("r must be > 0 and <= 1")
    if measure not in ("jaccard", "containment"):
        raise ValueError("measure must be 'jaccard' or 'containment'")
    if patients not in ("all", "cases"):
        raise ValueError("patients must be 'all' or 'cases'")
    if block < 1:
        raise ValueError("block must be >= 1")
    size = np.asarray(size, np.int64).reshape(-1, 2)
    S = len(size)
    order = np.asarray(order, np.int64).reshape(-1)
    tot = size[:, 0] + (size[:, 1] if patients == "all" else 0)
    clump = np.full(S, -1, np.int64)
    lead = np.full(S, -1, np.int64)
    value = np.full(S, np.nan)
    shared = np.full((S, 2), -1, np.int64)
    free = np.ones(len(order), bool)   # by position in `order`
    k = 0
    pos = 0
    while pos < len(order):
        cand = pos + np.flatnonzero(free[pos:])[:block]          # positions of the next candidate leads
        if len(cand) == 0:
            break
        rest = cand[0] + 1 + np.flatnonzero(free[cand[0] + 1:])  # every unassigned position after the first of them
        counts = np.asarray(both_of(order[cand], order[rest]), np.int64).reshape(len(cand), len(rest), 2)
        for ci, cp in enumerate(cand.tolist()):
            if not free[cp]:
                continue   # absorbed by an earlier lead of this block: its counts are discarded
            row = order[cp]
            free[cp] = False
            clump[row], lead[row] = k, row
            sel = (rest > cp) & free[rest]
            others = order[rest[sel]]
            sh = counts[ci, sel]
            bo = sh[:, 0] + (sh[:, 1] if patients == "all" else 0)
            A, B = tot[row], tot[others]
            den = (A + B - bo) if measure == "jaccard" else np.minimum(A, B)
            v = np.zeros(len(others))
            np.divide(bo.astype(np.float64), den.astype(np.float64), out=v, where=den > 0)
            join = v >= r
            rows_in = others[join]
            clump[rows_in], lead[rows_in] = k, row
            value[rows_in] = v[join]
            shared[rows_in] = sh[join]
            free[rest[sel][join]] = False
            k += 1
        pos = int(cand[-1]) + 1
    return clump, lead, value, shared


def _set_clump_columns(out, clump, lead, value, shared) -> None:
    """``CLUMP_COLUMNS`` of a results table from the per-row arrays of ``clump_rows`` / ``clump_sets``."""
    S = len(out)
    is_member = (clump >= 0) & (lead != np.arange(S))
    paths = [str(p) for p in out["Paths"]]
    out["Clump"] = clump
    out["ClumpLead"] = [paths[l] if l >= 0 else None for l in lead.tolist()]
    out["ClumpSize"] = np.where(clump >= 0, np.bincount(clump[clump >= 0], minlength=1)[np.maximum(clump, 0)], 0)
    out["LeadOverlap"] = np.where(is_member, value, np.nan)
    out["SharedCases"] = np.where(is_member, shared[:, 0], np.nan)
    out["SharedControls"] = np.where(is_member, shared[:, 1], np.nan)


def residual_rows(sets, rows, signs, which, given, n: int, method: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """gcre_score_sets_given's union rows by their definition, in numpy: (pos, neg, valid), bool [entries][n]
    twice and bool [entries].  Entry i is set ``which[i]`` (None: every set in order) without the carriers of set
    ``given[i]`` (-1, or ``given`` None: nothing set aside): pos = the OR of its (+) members, neg of its (-) members (method
    1, or ``signs`` None: every member into pos), both ``& ~C_given`` with C the OR of ALL members of the given set
    (``carrier_rows``) -- the given set's own full row, whatever it is given itself.  An entry whose set has an NA member
    (-1) is not valid and its rows are all False; a given set with an NA member raises ValueError."""
    d = np.asarray(rows)[:, :n] != 0 if len(rows) else np.zeros((0, n), bool)
    S = len(sets)
    C, cvalid = carrier_rows(sets, rows, n)
    iw = np.arange(S) if which is None else np.asarray(which, np.int64).reshape(-1)
    ig = np.full(len(iw), -1, np.int64) if given is None else np.asarray(given, np.int64).reshape(-1)
    if len(ig) != len(iw):
        raise ValueError(f"given: {len(ig)} entries for {len(iw)} scored sets")
    pos = np.zeros((len(iw), n), bool)
    neg = np.zeros((len(iw), n), bool)
    valid = np.ones(len(iw), bool)
    for i, (s, g) in enumerate(zip(iw.tolist(), ig.tolist())):
        if not 0 <= s < S or not -1 <= g < S:
            raise ValueError(f"entry {i}: set {s} given {g} out of range ({S} sets)")
        if g >= 0 and not cvalid[g]:
            raise ValueError(f"entry {i}: the given set {g} has an NA member")
        members = [int(x) for x in sets[s]]
        if any(x < 0 for x in members):
            valid[i] = False
            continue
        sg = [1] * len(members) if signs is None else [int(x) for x in signs[s]]
        for m, x in zip(members, sg):
            if method == 2 and x == -1:
                neg[i] |= d[m]
            else:
                pos[i] |= d[m]
        if g >= 0:
            pos[i] &= ~C[g]
            neg[i] &= ~C[g]
    return pos, neg, valid


def _set_lists(sets, signs):
    """``sets`` as a list of member lists and ``signs`` as a list of sign lists (or None), from either form the set entries
    of ``api.JoinExec`` take: sequences per set, or ``(off, members)`` with one flat signs array."""
    if isinstance(sets, tuple) and len(sets) == 2 and isinstance(sets[0], np.ndarray):
        off = np.asarray(sets[0], np.int64)
        members = np.asarray(sets[1], np.int64)
        flat = None if signs is None else np.asarray(signs, np.int64).reshape(-1)
        if flat is not None and len(flat) != len(members):
            raise ValueError("signs: one sign per member of every set")
        return ([members[off[s]:off[s + 1]].tolist() for s in range(len(off) - 1)],
                None if flat is None else [flat[off[s]:off[s + 1]].tolist() for s in range(len(off) - 1)])
    lists = [[int(x) for x in m] for m in sets]
    if signs is None:
        return lists, None
    sg = [[int(x) for x in m] for m in signs]
    if len(sg) != len(lists) or any(len(a) != len(b) for a, b in zip(sg, lists)):
        raise ValueError("signs: one sign per member of every set")
    return lists, sg


def patient_counts_reference(sets, rows, signs, which, group, n_groups, n: int, by_sign) -> Tuple[np.ndarray, np.ndarray, int]:
    """gcre_set_patient_counts by its definition, in numpy: ``(counts, group_sets, skipped)``.  Entry i is
    set ``which[i]`` (None: every set once; a set listed twice is counted twice) in group ``group[i]`` (-1: not counted;
    None: group 0).  counts int32 [n_groups][H][n], H = 1 + by_sign: the carrier rows of the entries of a group, added up
    per patient -- plane 0 the OR of ALL members (``carrier_rows``) without ``by_sign``; with it plane 0 the OR of the +1
    members and plane 1 of the -1 members of ``signs`` (None: all +1), no conflict removal.  An entry with a group whose
    set has an NA member (-1) is counted nowhere but in ``skipped``; group_sets int64 [n_groups] = the entries counted.
    Columns of ``rows`` beyond ``n`` are not patients.  ``n_groups`` None: 1 without ``group``, max(group) + 1 with it."""
    lists, sg = _set_lists(sets, signs)
    d = np.asarray(rows)[:, :n] != 0 if len(rows) else np.zeros((0, n), bool)
    S = len(lists)
    iw = np.arange(S) if which is None else np.asarray(which, np.int64).reshape(-1)
    ig = np.zeros(len(iw), np.int64) if group is None else np.asarray(group, np.int64).reshape(-1)
    if len(ig) != len(iw):
        raise ValueError(f"group: {len(ig)} entries for {len(iw)} counted sets")
    G = (max(int(ig.max()) + 1, 1) if len(ig) else 1) if n_groups is None else int(n_groups)
    if G < 1 or (group is None and G != 1):
        raise ValueError(f"n_groups = {G}: at least 1, and 1 without group")
    H = 2 if by_sign else 1
    counts = np.zeros((G, H, n), np.int64)
    group_sets = np.zeros(G, np.int64)
    skipped = 0
    for i, (s, g) in enumerate(zip(iw.tolist(), ig.tolist())):
        if not 0 <= s < S or not -1 <= g < G:
            raise ValueError(f"entry {i}: set {s} in group {g} out of range ({S} sets, {G} groups)")
        if g < 0:
            continue
        if any(x < 0 for x in lists[s]):
            skipped += 1
            continue
        group_sets[g] += 1
        planes = np.zeros((H, n), bool)
        for k, x in enumerate(lists[s]):
            planes[1 if by_sign and sg is not None and sg[s][k] == -1 else 0] |= d[x]
        counts[g] += planes
    return counts.astype(np.int32), group_sets, skipped


PATIENT_COLUMNS = ["Patient", "Label", "Hits", "HitShare"]   # the group columns stand between Label and Hits


def patient_table(counts, n_cases: int, names=None, columns=None, group_sets=None, summed=None):
    """One row per patient, in patient order, from the counts of ``JoinExec.patient_counts`` / ``patient_counts_reference``
    (int [n_groups][1][n], or [n_groups][n]; the two planes of ``by_sign`` are not one tally and raise ValueError):
    "Patient" (the index, or ``names[q]``), "Label" ("case" for the first ``n_cases`` patients, "control" after them), one
    count column per group (``columns``; default "Group0", "Group1", ..), "Hits" -- the sum of the first ``summed`` group
    columns (None: all of them) -- and "HitShare" = Hits over the number of sets counted into those groups
    (``group_sets``; NaN without it or where that number is 0).  Descriptive: no p-value is attached, and the carriers of
    sets that were selected on the labels are enriched in cases by construction."""
    import pandas as pd

    c = np.asarray(counts)
    if c.ndim == 3:
        if c.shape[1] != 1:
            raise ValueError(f"patient_table: {c.shape[1]} planes (by_sign) are not one tally: pass one plane")
        c = c[:, 0, :]
    if c.ndim != 2:
        raise ValueError("patient_table: counts [n_groups][n] or [n_groups][1][n]")
    G, n = c.shape
    cols = [f"Group{g}" for g in range(G)] if columns is None else [str(x) for x in columns]
    if len(cols) != G or len(set(cols)) != G or set(cols) & set(PATIENT_COLUMNS):
        raise ValueError(f"patient_table: {G} distinct column names, none of {PATIENT_COLUMNS}")
    if not 0 <= int(n_cases) <= n:
        raise ValueError(f"patient_table: n_cases = {n_cases} of {n} patients")
    if names is not None and len(names) != n:
        raise ValueError(f"patient_table: {len(names)} names for {n} patients")
    k = G if summed is None else int(summed)
    if not 0 <= k <= G:
        raise ValueError(f"patient_table: summed = {summed} of {G} groups")
    out = {"Patient": list(names) if names is not None else np.arange(n, dtype=np.int64),
           "Label": np.where(np.arange(n) < int(n_cases), "case", "control")}
    for g, name in enumerate(cols):
        out[name] = c[g].astype(np.int64)
    hits = c[:k].astype(np.int64).sum(axis=0)
    total = 0 if group_sets is None else int(np.asarray(group_sets, np.int64).reshape(-1)[:k].sum())
    out["Hits"] = hits
    out["HitShare"] = hits / total if total > 0 else np.full(n, np.nan)
    return pd.DataFrame(out, columns=["Patient", "Label"] + cols + ["Hits", "HitShare"])


_patient_table = patient_table   # (gwaspa has a keyword of the same name)


def unpack_masks(masks, n: int) -> np.ndarray:
    """Packed permutation masks -- the uint64 words ``JoinExec.perm_mask`` returns, one row per permutation -- as a 0/1
    int64 matrix [permutations][n]: bit q of a row is patient q."""
    W = (int(n) + 63) // 64
    m = np.asarray(masks, dtype=np.uint64).reshape(-1, W)
    bits = (m[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return bits.reshape(len(m), W * 64)[:, :n].astype(np.int64)


def burden_reference(weights, masks, n_cases: int) -> Dict[str, np.ndarray]:
    """gcre_patient_burden by its definition, in numpy and int64.  ``weights``: non-negative integers
    [rows][n] (or [G][H][n], flattened), columns < ``n_cases`` the cases; ``masks``: the packed words ``JoinExec.perm_mask``
    returns, one row per permutation (bits beyond n are not patients).  For every row g: ``total`` = sum_q w[g][q],
    ``observed`` = the sum over q < n_cases, ``null`` [rows][permutations] = the sum over the q with bit q of the mask set,
    ``n_ge`` / ``n_le`` = the permutations with null >= / <= observed (a tie counts in both), ``planes`` = the bit length of
    the row's largest weight, ``p_upper`` / ``p_lower`` = n_ge / n_le over the permutations (NaN without any)."""
    w = np.asarray(weights)
    if w.ndim < 2:
        raise ValueError("weights: [rows][n]")
    n = w.shape[-1]
    w = w.reshape(-1, n).astype(np.int64)
    if (w < 0).any() or (w > 2**31 - 1).any():
        raise ValueError("weights: every weight must lie in 0 .. 2^31 - 1")
    if not 0 <= int(n_cases) <= n:
        raise ValueError(f"n_cases = {n_cases} of {n} patients")
    m = unpack_masks(masks, n) if np.size(masks) else np.zeros((0, n), np.int64)
    K = len(m)
    total = w.sum(axis=1)
    observed = w[:, :int(n_cases)].sum(axis=1)
    null = w @ m.T                                  # int64, exact
    n_ge = (null >= observed[:, None]).sum(axis=1).astype(np.int64)
    n_le = (null <= observed[:, None]).sum(axis=1).astype(np.int64)
    top = w.max(axis=1) if n else np.zeros(len(w), np.int64)
    planes = np.array([int(x).bit_length() for x in top], dtype=np.int32)
    nan = np.full(len(w), np.nan)
    return {"total": total, "observed": observed, "n_ge": n_ge, "n_le": n_le, "planes": planes,
            "p_upper": n_ge / K if K else nan, "p_lower": n_le / K if K else nan.copy(), "null": null}


BURDEN_COLUMNS = ["Group", "Sets", "Load", "CaseLoad", "ControlLoad", "CaseMean", "ControlMean", "PvalueUpper", "PvalueLower"]
BURDEN_NULL_COLUMNS = ["NullMean", "NullSD", "Z"]


def burden_table(res, n_cases: int, n_ctrls: int, names=None, group_sets=None):
    """One row per weight row of ``JoinExec.patient_burden`` / ``burden_reference`` (``res``, the dict either returns):
    "Group" (the row's index, or ``names[g]``), "Sets" (``group_sets[g]``, the sets tallied into the row; NaN without it),
    "Load" = total, "CaseLoad" = observed, "ControlLoad" = total - observed, "CaseMean" = CaseLoad / n_cases,
    "ControlMean" = ControlLoad / n_ctrls, "PvalueUpper" = n_ge / permutations (cases carry MORE than a random split),
    "PvalueLower" = n_le / permutations.  Where ``res`` holds the null sums: "NullMean" = null.mean(axis=1), "NullSD" =
    null.std(axis=1) (both float64 on the exact int64 matrix) and "Z" = (CaseLoad - NullMean) / NullSD, NaN where NullSD
    is 0 or there is no permutation.  The p-values mean something only where the weights were not selected on these
    labels: a second cohort, or sets chosen without the labels."""
    import pandas as pd

    total = np.asarray(res["total"], np.int64).reshape(-1)
    observed = np.asarray(res["observed"], np.int64).reshape(-1)
    R = len(total)
    if names is not None and len(names) != R:
        raise ValueError(f"burden_table: {len(names)} names for {R} rows")
    sets = np.full(R, np.nan) if group_sets is None else np.asarray(group_sets, np.int64).reshape(-1)
    if len(sets) != R:
        raise ValueError(f"burden_table: {len(sets)} set counts for {R} rows")
    if int(n_cases) < 0 or int(n_ctrls) < 0:
        raise ValueError("burden_table: n_cases and n_ctrls must not be negative")
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"Group": list(names) if names is not None else np.arange(R, dtype=np.int64), "Sets": sets, "Load": total,
               "CaseLoad": observed, "ControlLoad": total - observed,
               "CaseMean": observed / np.float64(n_cases), "ControlMean": (total - observed) / np.float64(n_ctrls),
               "PvalueUpper": np.asarray(res["p_upper"], np.float64).reshape(-1),
               "PvalueLower": np.asarray(res["p_lower"], np.float64).reshape(-1)}
        cols = list(BURDEN_COLUMNS)
        if res.get("null") is not None:
            null = np.asarray(res["null"], np.int64).reshape(R, -1)
            if null.shape[1]:
                mean, sd = null.mean(axis=1), null.std(axis=1)
            else:
                mean, sd = np.full(R, np.nan), np.full(R, np.nan)
            out["NullMean"], out["NullSD"] = mean, sd
            out["Z"] = np.where(sd > 0, (observed - mean) / np.where(sd > 0, sd, 1.0), np.nan)
            cols += BURDEN_NULL_COLUMNS
    return pd.DataFrame(out, columns=cols)


def burden_test(sets, genes: Sequence[str], data: np.ndarray, n_cases: int, n_ctrls: int, signed: bool = False, group=None,
                names=None, threshold: float = 0.05, n_permutations: int = 100, strata: Optional[Sequence[int]] = None,
                seed: int = 0, device: int = 0):
    """Burden test of sets the caller names: per patient, how many sets of a group the patient carries
    (``JoinExec.patient_counts``), and whether the cases carry more -- or fewer -- of them than the cases of
    ``n_permutations`` random relabellings (``JoinExec.patient_burden``), all on one context of its own with
    the masks of ``generate_permutations(seed, strata)``.  ``sets`` as ``parse_sets`` reads them; genes are looked up after
    ``preprocess_table(threshold)`` (a set with a symbol not found is counted nowhere).  ``group``: per set 0 .. G - 1, or
    -1 = not counted (None: one group); ``names``: one per group.  ``signed``: ``by_sign`` tallies, a (+) and a (-) row per
    group.  Returns the ``burden_table`` (with the null columns); ``.attrs["skipped"]`` is the number of sets skipped.

    A gene-set burden test -- per patient the number of genes of a pathway with a variant -- is this call with one-gene
    sets and ``group`` the pathway's index::

        pathways = {"KEGG_A": ["TP53", "ATM"], "KEGG_B": ["BRCA2", "ATM", "CHEK2"]}
        sets = [[g] for p in pathways.values() for g in p]
        group = [i for i, p in enumerate(pathways.values()) for _ in p]
        burden_test(sets, genes, data, n_cases, n_ctrls, group=group, names=list(pathways), n_permutations=10000)

    The p-values are valid where the sets were chosen without looking at these labels -- a pathway list, or the findings
    of ANOTHER cohort (``replicate``).  A burden p-value on sets selected on the same labels -- a run's own significant
    paths -- is meaningless: their carriers are enriched in cases by construction."""
    from . import api
    genes, data = preprocess_table(genes, data, threshold, n_cases, n_ctrls)
    _, rows, signs = parse_sets(sets, genes)
    used: Dict[int, int] = {}
    idx = [[-1 if r < 0 else used.setdefault(r, len(used)) for r in rs] for rs in rows]
    sub = np.asarray(data)[list(used.keys())] if used else np.zeros((0, n_cases + n_ctrls), np.int32)
    ex = api.JoinExec(2 if signed else 1, n_cases, n_ctrls, int(n_permutations), device=device)
    try:
        if n_permutations > 0:
            ex.generate_permutations(seed, strata)
        counts, group_sets, skipped = ex.patient_counts(idx, sub, group=group, by_sign=bool(signed), signs=signs if signed else None)
        res = ex.patient_burden(counts, null=True)
    finally:
        ex.close()
    G, H = counts.shape[:2]
    if names is not None and len(names) != G:
        raise ValueError(f"burden_test: {len(names)} names for {G} groups")
    base = [str(x) for x in names] if names is not None else [f"Group{g}" for g in range(G)]
    labels = [f"{b} {s}" for b in base for s in (POS, NEG)] if H == 2 else base
    out = burden_table(res, n_cases, n_ctrls, names=labels, group_sets=np.repeat(group_sets, H))
    out.attrs["skipped"] = int(skipped)
    return out


REPLICATE_GROUPS = ["L1", "L2", "L3", "L4", "L5", "All"]


def replicate(results_df, genes: Sequence[str], data: np.ndarray, n_cases: int, n_ctrls: int, signed: bool = False,
              threshold: float = 0.05, n_permutations: int = 100, strata: Optional[Sequence[int]] = None, seed: int = 0,
              device: int = 0, leads_only: bool = False) -> Dict[str, object]:
    """Do the findings of a DISCOVERY run replicate in a second cohort?  ``results_df``: a GWASPA.Results or
    Significant.Results table of the discovery run (its ``SignedPaths`` column with ``signed``, else ``Paths``);
    ``genes`` / ``data`` / ``n_cases`` / ``n_ctrls``: the matrix of the SECOND cohort, which the paths were not selected on.

      "Replication.Paths"   ``score_paths`` of every row in the second cohort: one permutation p-value per path
      "Replication.Burden"  the ``burden_table`` of the carrier tallies (``JoinExec.patient_counts``: a patient carries a
                            path with a variant in any of its genes), one row per path length "L1" .. "L5" and "All",
                            with a "Skipped" column: do the second cohort's cases carry more of the findings than the
                            cases of a random relabelling do (``JoinExec.patient_burden``)
      "skipped"             paths with a gene that is absent from the second cohort (after ``preprocess_table``): NA in
                            "Replication.Paths", counted in no tally, reported per group in "Skipped"

    ``leads_only``: only the rows that are their own ``ClumpLead`` (``clump_paths`` / ``gwaspa(clump=..)``) go into the
    tallies -- one vote per finding.  Both use the masks of ``generate_permutations(seed, strata)``.

    This is valid because the second cohort's labels had no part in choosing the paths.  A burden p-value on sets
    selected on the same labels -- the discovery cohort's own matrix here -- is meaningless: the carriers of selected paths
    are enriched in cases by construction (which is why ``gwaspa(patient_table=True)`` attaches none)."""
    from . import api
    col = "SignedPaths" if signed and "SignedPaths" in results_df else "Paths"
    paths = [str(p) for p in results_df[col]]
    keep = np.ones(len(paths), bool)
    if leads_only:
        if "ClumpLead" not in results_df:
            raise ValueError("leads_only: the table has no ClumpLead column (clump_paths, or gwaspa(clump=..))")
        keep = (results_df["ClumpLead"].astype(object) == results_df["Paths"].astype(object)).to_numpy(dtype=bool)
    out: Dict[str, object] = {"Replication.Paths": score_paths(paths, genes, data, n_cases, n_ctrls, signed, threshold,
                                                                n_permutations, strata, seed, device)}
    pgenes, pdata = preprocess_table(genes, data, threshold, n_cases, n_ctrls)
    names, rows, _ = parse_sets(paths, pgenes)
    used: Dict[int, int] = {}
    idx = [[-1 if r < 0 else used.setdefault(r, len(used)) for r in rs] for rs in rows]
    sub = np.asarray(pdata)[list(used.keys())] if used else np.zeros((0, n_cases + n_ctrls), np.int32)
    G = len(REPLICATE_GROUPS)
    sel = np.flatnonzero(keep)
    lengths = np.array([len(nm) for nm in names], np.int64)[sel]
    # every kept path once into its length's group (lengths outside 1 .. 5: none) and once into "All"
    which = np.concatenate([sel, sel])
    grp = np.concatenate([np.where((lengths >= 1) & (lengths <= 5), lengths - 1, -1), np.full(len(sel), G - 1, np.int64)])
    na = np.array([any(r < 0 for r in rows[s]) for s in sel.tolist()], bool)
    skipped_of = np.bincount(grp[np.concatenate([na, na]) & (grp >= 0)], minlength=G).astype(np.int64)
    ex = api.JoinExec(2 if signed else 1, n_cases, n_ctrls, int(n_permutations), device=device)
    try:
        if n_permutations > 0:
            ex.generate_permutations(seed, strata)
        counts, group_sets, _ = ex.patient_counts(idx, sub, which=which, group=grp, n_groups=G)
        res = ex.patient_burden(counts, null=True)
    finally:
        ex.close()
    table = burden_table(res, n_cases, n_ctrls, names=REPLICATE_GROUPS, group_sets=group_sets)
    table["Skipped"] = skipped_of
    out["Replication.Burden"] = table
    out["skipped"] = int(na.sum())
    return out


def _set_residual_columns(out, ex, sets, rows, signs, clump, lead) -> None:
    """``RESIDUAL_COLUMNS`` of a clumped table: every member row rescored without its lead's carriers, all of them in ONE
    ``JoinExec.score_sets(which=members, given=their leads)`` call on ``ex``.  NaN on leads and -1 rows."""
    S = len(out)
    res = {c: np.full(S, np.nan) for c in RESIDUAL_COLUMNS}
    js = np.flatnonzero((clump >= 0) & (lead != np.arange(S)))
    if len(js):
        rec = ex.score_sets(sets, rows, signs, which=js, given=lead[js])
        res["ResidualScores"][js] = rec["score"]
        res["ResidualCases"][js] = rec["cases"]
        res["ResidualControls"][js] = rec["ctrls"]
        res["ResidualPvalues"][js] = rec["pvalue"]
    for cname in RESIDUAL_COLUMNS:
        out[cname] = res[cname]


def clump_paths(results_df, genes: Sequence[str], data: np.ndarray, n_cases: int, n_ctrls: int, signed: bool = False,
                r: float = 0.5, measure: str = "jaccard", patients: str = "all", by_length: bool = False,
                conditional: bool = False, threshold: float = 0.05, n_permutations: int = 100,
                strata: Optional[Sequence[int]] = None, seed: int = 0, device: int = 0, on_device: bool = False, *,
                exec_=None, table: Optional[np.ndarray] = None):
    """Which rows of a GWASPA.Results table are the same finding: rows clumped by the patients that carry them, and with
    ``conditional`` each row rescored without its lead's carriers.  A row's carriers are the patients
    with a variant in any gene of its ``SignedPaths`` (``carrier_rows``); the pairwise shared-carrier counts come from the
    device (gcre_set_overlap), the rule is ``clump_rows``.  Genes are looked up after ``preprocess_table(threshold)``, as
    ``score_paths`` does.  Rows with a finite score and no NA gene are walked by ``Scores`` descending (ties: table
    position); with ``by_length`` every ``Lengths`` group, ascending, is clumped on its own and the clump ids keep
    counting.  Returns a copy of the table with

      ``Clump``  the clump id (-1: a row that was not clumped), ``ClumpLead``  the lead row's ``Paths`` (None for -1),
      ``ClumpSize``  rows in the clump (0 for -1), ``LeadOverlap``  the measure against the lead, ``SharedCases`` /
      ``SharedControls``  the carriers shared with the lead (the last three NaN on lead rows and on -1 rows).

    ``conditional``: every non-lead row is scored as if every patient column its lead carries were zeroed in the whole
    carrier matrix (method 1: U & ~C_lead; method 2: both halves & ~C_lead; n_cases / n_ctrls unchanged: the removed
    patients count as non-carriers) -- all of them in ONE ``JoinExec.score_sets(which=rows, given=their leads)`` call, the
    residual rows built on the device, on one context with ``api.values_table`` and the masks of
    ``generate_permutations(seed, strata)``: ``ResidualScores``, ``ResidualCases``, ``ResidualControls`` and
    ``ResidualPvalues``.  ``ResidualPvalues`` is that set's NOMINAL permutation p-value n_ge / n_permutations -- the
    residual score against its own null, not a family-wise number like ``Pvalues``.  NaN on lead rows and on -1 rows.

    ``on_device``: the rule runs on the device too -- one ``api.JoinExec.clump_sets`` call per group instead of the
    ``clump_rows`` / ``set_overlap`` loop, no pair count comes back.  Every column is what it is without
    it.

    ``exec_`` / ``table``: a JoinExec of this method and these patients to run everything on -- with ``conditional`` it must
    already hold the value table and the masks, and its iterations must be ``n_permutations`` -- or, without one, the value
    table itself, so that neither is built twice (``seed`` / ``strata`` are then the caller's business)."""
    from . import api
    method = 2 if signed else 1
    genes, data = preprocess_table(genes, data, threshold, n_cases, n_ctrls)
    _, rows, signs = parse_sets([str(p) for p in results_df["SignedPaths"]], genes)
    used: Dict[int, int] = {}
    sets = [[-1 if x < 0 else used.setdefault(x, len(used)) for x in rs] for rs in rows]
    sub = np.asarray(data)[list(used.keys())] if used else np.zeros((0, n_cases + n_ctrls), np.int32)
    S = len(sets)
    scores = results_df["Scores"].to_numpy(dtype=np.float64)
    lengths = results_df["Lengths"].to_numpy()
    ok = np.isfinite(scores) & np.array([all(x >= 0 for x in rs) for rs in rows], dtype=bool).reshape(S)
    K = int(n_permutations) if conditional else 0
    out = results_df.copy()
    clump = np.full(S, -1, np.int64)
    lead = np.full(S, -1, np.int64)
    value = np.full(S, np.nan)
    shared = np.full((S, 2), -1, np.int64)
    if exec_ is not None and conditional and exec_.iters != K:
        raise ValueError(f"exec_: a context of {exec_.iters} permutations, n_permutations = {K}")
    ex = exec_ if exec_ is not None else api.JoinExec(method, n_cases, n_ctrls, K, device=device)
    try:
        size, _ = ex.set_overlap(sets, sub, a=[], b=[]) if S and not on_device else (np.zeros((0, 2), np.int32), None)
        groups = [np.flatnonzero(ok & (lengths == L)) for L in np.unique(lengths[ok]).tolist()] if by_length \
            else [np.flatnonzero(ok)]
        base = 0
        for idx in groups:
            order = idx[np.argsort(-scores[idx], kind="stable")]
            if on_device:
                c, l, v, sh, _ = ex.clump_sets(sets, sub, order, r, measure, patients)
            else:
                c, l, v, sh = clump_rows(order, size, lambda la, lb: ex.set_overlap(sets, sub, a=la, b=lb)[1], r, measure,
                                         patients)
            clump[order], lead[order], value[order], shared[order] = c[order] + base, l[order], v[order], sh[order]
            base += int(c[order].max()) + 1 if len(order) else 0
        _set_clump_columns(out, clump, lead, value, shared)
        if conditional:
            if exec_ is None:
                ex.set_value_table(api.values_table(n_cases, n_ctrls) if table is None else table)
                if K > 0:
                    ex.generate_permutations(seed, strata)
            _set_residual_columns(out, ex, sets, sub, signs, clump, lead)
    finally:
        if exec_ is None:
            ex.close()
    return out


# ---------------------------------------------------------------------------------------------------------------
# inputs


def check_input(n_cases, n_ctrls, method, threshold, top_k, path_length, iterations):
    """check_input (R/Utils.R:203-241); same conditions, ValueError instead of stop()."""
    def integer(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    if not integer(n_cases) or n_cases < 2:
        raise ValueError("nCases must be an integer >= 2!")
    if not integer(n_ctrls) or n_ctrls < 2:
        raise ValueError("nControls must be an integer >= 2!")
    if not integer(top_k) or top_k < 1 or top_k > 10000:
        raise ValueError("K must be an integer >= 1 and <= 10000!")
    if not (isinstance(method, str) and method[:7] in ("method1", "method2")):
        raise ValueError("method must be one of: 'method1', 'method2'!")
    if not isinstance(threshold, (int, float)) or threshold > 1 or threshold <= 0:
        raise ValueError("threshold_percent must be a real number > 0 and <= 1!")
    if not integer(path_length) or path_length > 5 or path_length < 1:
        raise ValueError("pathLength must be an integer >= 1 and <= 5!")
    if not integer(iterations) or iterations < 0:
        raise ValueError("iterations must be an integer greater than or equal to 0!")
    if n_cases + n_ctrls > 65536:
        raise ValueError("Package cannot process data set with more than 65536 columns!")


def read_dataset(path: str) -> Tuple[List[str], List[str], np.ndarray]:
    """The whitespace table PreprocessTable reads (Utils.R:164-168): header ``symbols p1 p2 ...``, one gene per row."""
    with open(path) as fh:
        header = fh.readline().split()
        if not header or header[0].strip('"') != "symbols":
            raise ValueError("First column must be named symbols and must contain the gene symbols!")
        symbols, rows = [], []
        for line in fh:
            parts = line.split()
            if not parts:
                continue
            symbols.append(parts[0].strip('"'))
            rows.append(np.array(parts[1:], dtype=np.int32))
    return symbols, [h.strip('"') for h in header[1:]], np.vstack(rows) if rows else np.zeros((0, len(header) - 1), np.int32)


def preprocess_table(symbols: Sequence[str], data: np.ndarray, threshold: float, n_cases: int, n_ctrls: int
                     ) -> Tuple[List[str], np.ndarray]:
    """PreprocessTable (R/Utils.R:162-199): drop NA / duplicated symbols, 2 -> 1, check the shape and the 0/1
    alphabet, keep genes with at most ``threshold * ncol(df)`` variant carriers (ncol counts the symbols column)."""
    data = np.array(data, dtype=np.int32)
    keep, seen = [], set()
    for i, s in enumerate(symbols):
        if s is None or s == "NA" or s in seen:
            continue
        seen.add(s)
        keep.append(i)
    data = data[keep]
    genes = [symbols[i] for i in keep]
    data[data == 2] = 1
    if data.shape[1] != n_cases + n_ctrls:
        raise ValueError("The number of patients in the dataset must be equal to nCases + nControls!")
    if ((data != 0) & (data != 1)).any():
        raise ValueError("The patient columns must consist of only 0,1 or 2 entries!")
    freqs = data.sum(axis=1)
    sel = np.flatnonzero(freqs <= threshold * (data.shape[1] + 1))
    return [genes[i] for i in sel], data[sel]


@dataclass
class Prepared:
    """The frames GWASPA holds after filtering the network against the dataset (ProcessPaths.R:131-176, 206-212)."""

    ents_uid: np.ndarray          # genes with data that occur in a kept relation, ascending uid
    ents_symbol: List[str]
    ents2_uid: np.ndarray         # genes with data that are the source of any relation (targets may lack data)
    ents2_symbol: List[str]
    src: np.ndarray               # kept relations sorted by (src, trg) -- ranks into ents_uid
    trg: np.ndarray
    sign: np.ndarray
    data1: np.ndarray             # rows follow ents_uid
    data2: np.ndarray             # rows follow ents2_uid


def prepare_inputs(genes: Sequence[str], data: np.ndarray, ents_uid: Sequence[int], ents_symbol: Sequence[str],
                   rel_src: Sequence[int], rel_trg: Sequence[int], rel_sign: Sequence[int]) -> Prepared:
    """ProcessPaths.R:131-176: intersect the knowledge base with the dataset.

    Ents: symbol != "-1", first occurrence of each symbol, present in the dataset, ordered by uid.  Relations:
    unique (src, trg, sign) rows whose source is in Ents (these define Ents2); those whose target is too and that
    are not self loops define the joined network and shrink Ents to the genes they touch.
    """
    ents_uid = np.asarray(ents_uid, dtype=np.int64)
    row_of = {}
    for i, g in enumerate(genes):
        row_of.setdefault(g, i)
    keep, seen = [], set()
    for i, s in enumerate(ents_symbol):
        if s == "-1" or s in seen:
            continue
        seen.add(s)
        if s in row_of:
            keep.append(i)
    keep = sorted(keep, key=lambda i: int(ents_uid[i]))
    e_uid = ents_uid[keep]
    e_sym = [ents_symbol[i] for i in keep]
    present = set(e_uid.tolist())

    rels = np.unique(np.stack([np.asarray(rel_src, np.int64), np.asarray(rel_trg, np.int64),
                               np.asarray(rel_sign, np.int64)], axis=1), axis=0) if len(rel_src) else np.zeros((0, 3), np.int64)
    src_ok = np.array([s in present for s in rels[:, 0].tolist()], dtype=bool)
    rels2 = rels[src_ok]
    trg_ok = np.array([t in present for t in rels2[:, 1].tolist()], dtype=bool)
    rels1 = rels2[trg_ok & (rels2[:, 0] != rels2[:, 1])]
    rels1 = rels1[np.lexsort((rels1[:, 1], rels1[:, 0]))]
    if len(rels1) > 1 and (np.diff(rels1[:, 0]) == 0)[np.diff(rels1[:, 1]) == 0].any():
        raise ValueError("the network lists a relation (src, trg) with two different signs")

    sym_of = dict(zip(e_uid.tolist(), e_sym))
    left2 = np.unique(rels2[:, 0])
    e2_uid = np.array([u for u in e_uid.tolist() if u in set(left2.tolist())], dtype=np.int64)
    e2_sym = [sym_of[u] for u in e2_uid.tolist()]
    left = set(np.unique(np.concatenate([rels1[:, 0], rels1[:, 1]])).tolist())
    e1_uid = np.array([u for u in e_uid.tolist() if u in left], dtype=np.int64)
    e1_sym = [sym_of[u] for u in e1_uid.tolist()]

    rank = {u: i for i, u in enumerate(e1_uid.tolist())}
    src = np.array([rank[u] for u in rels1[:, 0].tolist()], dtype=np.int32)
    trg = np.array([rank[u] for u in rels1[:, 1].tolist()], dtype=np.int32)
    data = np.asarray(data, dtype=np.int32)
    d1 = data[[row_of[s] for s in e1_sym]] if len(e1_sym) else np.zeros((0, data.shape[1]), np.int32)
    d2 = data[[row_of[s] for s in e2_sym]] if len(e2_sym) else np.zeros((0, data.shape[1]), np.int32)
    return Prepared(e1_uid, e1_sym, e2_uid, e2_sym, src, trg, rels1[:, 2].astype(np.int32), d1, d2)


def frames_of(prep: Prepared, levels) -> Dict[str, Dict[str, np.ndarray]]:
    """The uid-valued frames getPaths indexes (ProcessPaths.R:206-212, 240): ranks -> uids."""
    u = prep.ents_uid
    r3 = levels.rels3
    return {
        "rels_data": {"srcuid": u},
        "rels_data2": {"srcuid": prep.ents2_uid},
        "rels": {"srcuid": u[prep.src], "trguid": u[prep.trg], "sign": prep.sign},
        "rels3": {"srcuid": u[r3["srcuid"]], "trguid": u[r3["trguid"]], "sign": r3["sign"],
                  "trguid2": u[r3["trguid2"]], "sign2": r3["sign2"]},
    }


def gwaspa(genes: Sequence[str], data: np.ndarray, n_cases: int, n_ctrls: int, network, signed: bool = False,
           threshold: float = 0.05, top_k: int = 10, path_length: int = 5, n_permutations: int = 100,
           strata: Optional[Sequence[int]] = None, seed: int = 0, device: int = 0, case_odds=None,
           decorated_pvalues: bool = False, gene_table: bool = False, fdr: bool = False,
           clump: Optional[float] = None, clump_conditional: bool = False, false_counts: bool = False,
           false_count_ks: Sequence[int] = (2, 5, 10), false_count_alpha: float = 0.05,
           stepdown: bool = False, significant: Optional[float] = None,
           significant_cap: int = 1_000_000, clump_significant: bool = False,
           patient_table: bool = False) -> Dict[str, object]:
    """GWASPA (R/ProcessPaths.R:87-344) without R: dataset -> GWASPA.Results, scored on the MI355X.

    ``network`` = (ents_uid, ents_symbol, rel_src, rel_trg, rel_sign): the knowledge base getStringKB() would load
    (the packaged STRING tables are data, not code -- callers bring their own).  ``strata`` gives one stratum id
    per patient column (what the strata file resolves to, ProcessPaths.R:180-191).  The scoring table, the level
    tables and the permutation masks are built by the native builders; permutations are
    drawn on the device from ``seed``, so two runs with the same seed return identical tables.

    ``decorated_pvalues``: also return "Decorated.Pvalues.Results", the split-path table of ``decorated_table``
    (R/DecoratedPvalue.R), drawn from a seed derived from ``seed`` (DECORATED_SEED_TAG).  R's GWASPA defaults to
    ``Decorated.Pvalues = TRUE``; here the default is False.  With ``path_length == 1`` it warns as R does and adds nothing.

    ``gene_table``: also return "Gene.Results" (``gene_results``): for every gene and length the best path through the
    gene, tallied on the device while the joins run (one GeneTally per level), and "gene_best" (length ->
    api.GeneBest, the raw tallies).  ``gene_summary`` reduces it to one row per gene.  Default False: the joins launch
    exactly what they launch without it.

    ``fdr``: after the usual pass every level is joined once more, on the same context, with an ``api.ExceedCounts`` whose
    thresholds are that level's finite top-K scores: GWASPA.Results gains "ExpectedFalse" (the per-family
    error rate: paths of the row's length a permutation pushes to the row's score or beyond, on average), "FDR" and
    "Qvalues" (``fdr_columns``: within a length, pi0 = 1), and the raw counts come back as "exceed" (length ->
    api.Exceedances).  Sentinel rows get NaN.  The row order and the other seven columns are what ``fdr=False`` returns.
    Default False.

    ``false_counts``: the same counting pass is made (whether or not ``fdr`` is set) with counters that keep the counts per
    permutation (``api.ExceedCounts(perm_counts=True)``), and GWASPA.Results gains the columns of
    ``false_count_columns(ks=false_count_ks, alpha=false_count_alpha)``: "MedianFalse", "FDRmedian", "FalseBound",
    "FDPbound" and "kFWER.<k>" -- single-threshold permutation quantiles under the complete null, not simultaneous over
    rows.  The raw arrays come back in "exceed" (``Exceedances.perm_counts``); ``fdr``'s own three columns appear only with
    ``fdr=True``.  ``top_k * n_permutations`` above 2^26 raises ValueError before anything runs; ``n_permutations == 0`` adds
    NaN columns.  Sentinel rows get NaN.  Default False: nothing new is called.

    ``stepdown``: the counting pass of ``false_counts`` is made (one pass and one set of counters when both are set), each
    level's finite top rows are turned into sets from the table's ``SignedPaths`` (``parse_sets``, signs for the signed
    method) and ``api.ExceedCounts.stepdown`` gives their step-down max-T counts (Westfall & Young 1993):
    GWASPA.Results gains "PvaluesStepDown" (``stepdown_columns``, within a length) -- the family-wise p-value of the row with
    the better rows of its length taken out of the family: never above ``Pvalues``, equal to it on each length's best row,
    the same FWER under the same assumption -- and the raw counts come back as "stepdown" (length -> int64 array, in the
    order of the level's finite scores).  ``top_k * n_permutations`` above 2^26 raises ValueError before anything runs;
    ``n_permutations == 0`` adds a NaN column.  Sentinel rows get NaN.  Default False: nothing new is called.

    ``clump``: with a value r, GWASPA.Results goes through ``clump_paths(r=clump, conditional=clump_conditional)`` with the
    run's own seed, strata, threshold and permutation count: it gains ``CLUMP_COLUMNS`` -- which rows are
    carried by the same patients as a better row -- and with ``clump_conditional`` ``RESIDUAL_COLUMNS``, each row rescored
    without its lead's carriers (``ResidualPvalues`` is a nominal per-set p-value, not a family-wise one).  The row order
    and the other columns are unchanged.  None, the default: nothing new is called.

    ``significant``: with a level alpha in (0, 1), after the usual pass each length's cut-off is taken from its own null
    maxima (``significance_cutoff``) and every level is joined once more with an ``api.HitList`` of ``significant_cap``
    records armed -- the same second pass that carries the counters of ``fdr`` / ``false_counts`` /
    ``stepdown`` when they are set: one extra pass in all.  "Significant.Results" has ``COLUMNS`` and holds EVERY path with
    ``Pvalues <= significant``, not only those among the ``top_k`` best of their length (built by ``results_table`` from the
    lists: same naming, same order); "significant" is length -> api.Hits, "significant_cutoffs" length -> float.  A length
    whose list overflowed contributes no rows and a warning naming how many were found.  Outside (0, 1), or with
    ``n_permutations == 0``, ValueError before anything runs.  GWASPA.Results and everything else are what
    ``significant=None`` returns.  None, the default: nothing new is called.

    ``clump_significant``: needs both ``clump`` and ``significant`` (ValueError before anything runs otherwise).
    "Significant.Results" gains ``CLUMP_COLUMNS``: its rows of all lengths are walked together by ``Scores`` descending
    (ties: table position), as ``clump_paths`` walks a table, with r = ``clump``, Jaccard over all patients.  The sets come
    from the hit lists themselves (``hit_sets``: no string is parsed) and the rule runs on the device, in one
    ``api.JoinExec.clump_sets`` call on the run's own context.  A length whose list overflowed contributes
    no rows, as without it.  With ``clump_conditional`` as well it gains ``RESIDUAL_COLUMNS`` too: every member row rescored
    without its lead's carriers in one ``score_sets(which=, given=)`` call on the run's own context -- its seed, strata and
    permutation count -- over the hit sets (unsigned) or the sets parsed from ``SignedPaths`` with their
    signs (signed).  False, the default: nothing new is called.

    ``patient_table``: needs ``significant`` (ValueError before anything runs otherwise).  "Patient.Results"
    (``patient_table``) says who carries the findings: one row per patient with "Hits.L1" .. "Hits.L<path_length>" -- how
    many rows of Significant.Results of that length the patient carries (a variant in any gene of the path, both methods)
    -- their sum "Hits" and "HitShare", from ONE ``api.JoinExec.patient_counts`` call on the run's own context over the hit
    sets.  With ``clump_significant`` the clump leads are listed a second time into one more group:
    "Leads", the distinct findings the patient carries.  The raw arrays come back as "patient_counts" = (counts,
    group_sets, skipped).  The table is descriptive: exact counts, no test statistic -- the paths were selected on these
    very labels, so their carriers are enriched in cases by construction; look for a handful of patients on every hit (a
    batch artefact), not for significance.  False, the default: the output and every launch are what they were.

    ``case_odds``: one fitted odds of being a case per patient (``case_odds(covariates, ...)``); the run's masks then come
    from ``generate_weighted_permutations(seed, case_odds, strata)`` (Epstein et al. 2012) and every
    ``Pvalues`` is taken against labels redrawn with these odds.  The adjustment is on the null, not on the scores, and the
    p-values are only as good as the fitted model.  ``decorated_pvalues`` and ``clump_conditional`` draw nulls of their own
    and are refused with it (ValueError before anything runs).  The output records "case_odds_digest", which
    ``score_paths(gwaspa_out=)`` compares.  None, the default: the output and every launch are what they were.
    """
    from . import api
    from .synth import Problem
    from .uids import UidRelSet

    method = "method2" if signed else "method1"
    check_input(n_cases, n_ctrls, method, threshold, top_k, path_length, n_permutations)
    if case_odds is not None and (decorated_pvalues or clump_conditional):
        raise ValueError("case_odds: decorated_pvalues and clump_conditional draw uniform nulls of their own; weighted draws are "
                         "not built there")
    if clump_significant and (clump is None or significant is None):
        raise ValueError("clump_significant: needs both clump (the overlap r) and significant (the family-wise level)")
    if clump_significant and not 0 < clump <= 1:
        raise ValueError("r must be > 0 and <= 1")
    if patient_table and significant is None:
        raise ValueError("patient_table: needs significant (the family-wise level): the tally runs over the hit lists")
    if significant is not None:
        if not 0.0 < float(significant) < 1.0:      # (NaN fails both comparisons)
            raise ValueError(f"significant: the family-wise level must lie inside (0, 1), not {significant!r}")
        if int(n_permutations) == 0:
            raise ValueError("significant: there are no p-values to cut at without permutations (n_permutations == 0)")
        if not 1 <= int(significant_cap) <= api.HITS_CAP_MAX:
            raise ValueError(f"significant_cap must be 1..{api.HITS_CAP_MAX} (2^26), not {significant_cap!r}")
    if (false_counts or stepdown) and int(top_k) * int(n_permutations) > EXCEED_PERM_CELLS:
        raise ValueError(f"{'false_counts' if false_counts else 'stepdown'}: top_k x n_permutations = {int(top_k) * int(n_permutations)} exceeds the limit of "
                         f"2^26 = {EXCEED_PERM_CELLS} per-permutation cells of a level")
    genes, data = preprocess_table(genes, data, threshold, n_cases, n_ctrls)
    prep = prepare_inputs(genes, data, *network)
    g = len(prep.ents_uid)
    if g == 0:
        raise ValueError("no gene of the dataset takes part in a relation of the network")
    levels = api.build_levels(g, prep.src, prep.trg, prep.sign)
    # level 1 runs over Ents2, which may hold genes whose relations all point outside the dataset (ProcessPaths.R:150-160)
    n2 = len(prep.ents2_uid)
    ids2 = np.arange(n2, dtype=np.int32)
    levels.uids["1b"] = UidRelSet(1, ids2, ids2, np.ones(n2, np.int32), np.arange(n2, dtype=np.int64), np.ones(n2, np.int32))
    levels.data_inds["1b"] = ids2.copy()
    levels.n_paths["1b"] = n2

    table = api.values_table(n_cases, n_ctrls)
    problem = Problem(method, n_cases, n_ctrls, path_length, top_k, n_permutations, levels, prep.data1, prep.data2,
                      table, np.zeros((0, 0), np.int32), seed)
    ex = api.JoinExec(method, n_cases, n_ctrls, n_permutations, device=device)
    ex.top_k = top_k
    ex.set_value_table(table)
    if n_permutations > 0:
        _draw_permutations(ex, seed, strata, case_odds)
    tallies = {}
    if gene_table:
        tables = gene_tables(levels, g, n2)
        for name in GENE_LEVELS[:path_length]:
            tallies[name] = api.GeneTally(ex, gene_slots(name, g, n2), *tables[name])
    lsts = api.process_paths(problem, device=device, exec_=ex, tallies=tallies or None)
    frames = frames_of(prep, levels)
    out = {"GWASPA.Results": results_table(lsts, path_length, frames,
                                           (prep.ents_uid, prep.ents_symbol), (prep.ents2_uid, prep.ents2_symbol)),
           "levels": lsts, "prepared": prep}
    if case_odds is not None:
        out["case_odds_digest"] = _odds_digest(case_odds)
    hit_lists, cutoffs = {}, {}
    if significant is not None:
        for L, name in enumerate(GENE_LEVELS[:path_length], start=1):
            cutoffs[L] = significance_cutoff(lsts[f"lst{L}"].null, float(significant))
            hit_lists[name] = api.HitList(ex, cutoffs[L], cap=int(significant_cap))
    hits_collected = False
    if fdr or false_counts or stepdown:
        keep = bool(false_counts or stepdown) and n_permutations > 0
        fc_names = false_count_names(false_count_ks) if false_counts else []
        new_cols = (FDR_COLUMNS if fdr else []) + fc_names + (STEPDOWN_COLUMNS if stepdown else [])
        counters = {}
        for L, name in enumerate(GENE_LEVELS[:path_length], start=1):
            s = np.asarray(lsts[f"lst{L}"].scores, np.float64)
            if np.isfinite(s).any():
                counters[name] = api.ExceedCounts(ex, s[np.isfinite(s)], perm_counts=True) if keep else \
                    api.ExceedCounts(ex, s[np.isfinite(s)])
        if counters:
            api.process_paths(problem, device=device, exec_=ex, exceeds=counters, hits=hit_lists or None)
            hits_collected = True
        df = out["GWASPA.Results"]
        lookup, counted = {}, {}
        if fdr or false_counts:
            out["exceed"] = counted
        if stepdown:
            out["stepdown"] = {}
        for L, name in enumerate(GENE_LEVELS[:path_length], start=1):
            if name not in counters:
                continue
            got = counters[name].read()
            counted[L] = got
            cols = fdr_columns(counters[name].thresholds, got.exceed, got.observed, got.perms) if fdr else {}
            if false_counts:
                cols.update(false_count_columns(counters[name].thresholds, got.perm_counts, got.observed, got.perms,
                                                ks=false_count_ks, alpha=false_count_alpha))
            if stepdown:
                thr = counters[name].thresholds
                if keep:
                    # set j = a table row of this length whose score is threshold j (tied rows: any of them, once each)
                    # (matched on the bits: the library compares a set's score with its threshold bit for bit)
                    sc_all = df["Scores"].to_numpy(np.float64)
                    at: Dict[bytes, List[int]] = {}
                    for i in np.flatnonzero((df["Lengths"].to_numpy() == L) & np.isfinite(sc_all)).tolist():
                        at.setdefault(sc_all[i].tobytes(), []).append(i)
                    picked = []
                    for t in thr:
                        left = at.get(t.tobytes())
                        if not left:
                            raise ValueError(f"stepdown: length {L}: no table row left for the top score {float(t)!r}")
                        picked.append(left.pop(0))
                    _, rows, signs = parse_sets([str(df["SignedPaths"].iat[i]) for i in picked], genes)
                    for i, rs in zip(picked, rows):
                        if any(r < 0 for r in rs):
                            raise ValueError(f"stepdown: length {L}, table row {i} ({df['SignedPaths'].iat[i]}): a gene is not "
                                             "in the dataset, so the row's carriers cannot be rebuilt")
                    used: Dict[int, int] = {}
                    sets = [[used.setdefault(r, len(used)) for r in rs] for rs in rows]
                    sub = np.asarray(data)[list(used.keys())] if used else np.zeros((0, n_cases + n_ctrls), np.int32)
                    try:
                        n_ge = counters[name].stepdown(sets, sub, signs if signed else None)
                    except api.GcreError as e:
                        # e.g. duplicate gene symbols: parse_sets takes the first row of a symbol, the join may have scored another
                        raise ValueError(f"stepdown: length {L}: the carriers rebuilt from SignedPaths are not the rows the join "
                                         f"scored ({e}); the other columns do not depend on this: run with stepdown=False") from e
                else:
                    n_ge = np.zeros(len(thr), np.int64)
                out["stepdown"][L] = n_ge
                cols.update(stepdown_columns(thr, n_ge, got.perms))
            for i, t in enumerate(counters[name].thresholds.tolist()):
                lookup[(L, t)] = tuple(cols[c][i] for c in new_cols)
            counters[name].free()
        rows = [lookup.get((int(L), float(sc)), (np.nan,) * len(new_cols)) for L, sc in zip(df["Lengths"], df["Scores"])]
        for k, c in enumerate(new_cols):
            df[c] = np.array([r[k] for r in rows], np.float64)
    if hit_lists:
        import warnings
        if not hits_collected:
            api.process_paths(problem, device=device, exec_=ex, hits=hit_lists)
        found, as_levels = {}, {}
        for L, name in enumerate(GENE_LEVELS[:path_length], start=1):
            h = found[L] = hit_lists[name].read()
            hit_lists[name].free()
            if not h.complete:
                warnings.warn(f"significant: length {L}: {h.found} paths reach the cut-off, more than significant_cap = "
                              f"{int(significant_cap)}: the length contributes no rows to Significant.Results")
            as_levels[f"lst{L}"] = h.as_join_result(lsts[f"lst{L}"].null)
        out["Significant.Results"] = results_table(as_levels, path_length, frames, (prep.ents_uid, prep.ents_symbol),
                                                   (prep.ents2_uid, prep.ents2_symbol))
        out["significant"] = found
        out["significant_cutoffs"] = cutoffs
        if clump_significant or patient_table:
            sig = out["Significant.Results"]
            hsets = hit_sets(found, gene_tables(levels, g, n2), g, n2,
                             nulls={L: lsts[f"lst{L}"].null for L in found})
            if len(hsets[0]) - 1 != len(sig):
                raise ValueError(f"{'clump_significant' if clump_significant else 'patient_table'}: {len(hsets[0]) - 1} hit sets for "
                                 f"{len(sig)} rows of Significant.Results")
        lead_rows = None
        if clump_significant:
            sc = sig["Scores"].to_numpy(dtype=np.float64)
            idx = np.flatnonzero(np.isfinite(sc))
            order = idx[np.argsort(-sc[idx], kind="stable")]
            c, l, v, sh, _ = ex.clump_sets(hsets, np.vstack([prep.data1, prep.data2]), order, r=clump)
            _set_clump_columns(sig, c, l, v, sh)
            lead_rows = np.flatnonzero((c >= 0) & (l == np.arange(len(sig))))
            if clump_conditional:
                if signed:   # the signs are in the table, not in the hit lists
                    _, prows, psigns = parse_sets([str(p) for p in sig["SignedPaths"]], genes)
                    used: Dict[int, int] = {}
                    rsets = [[-1 if x < 0 else used.setdefault(x, len(used)) for x in rs] for rs in prows]
                    rsub = np.asarray(data)[list(used.keys())] if used else np.zeros((0, n_cases + n_ctrls), np.int32)
                    _set_residual_columns(sig, ex, rsets, rsub, psigns, c, l)
                else:
                    _set_residual_columns(sig, ex, hsets, np.vstack([prep.data1, prep.data2]), None, c, l)
    if patient_table:
        # group = length - 1; the clump leads once more, into a group of their own (a set listed twice is counted twice)
        which = np.arange(len(sig), dtype=np.int64)
        grp = sig["Lengths"].to_numpy(dtype=np.int64) - 1
        names = [f"Hits.L{L}" for L in range(1, path_length + 1)]
        if lead_rows is not None:
            which = np.concatenate([which, lead_rows])
            grp = np.concatenate([grp, np.full(len(lead_rows), path_length, np.int64)])
            names.append("Leads")
        got = ex.patient_counts(hsets, np.vstack([prep.data1, prep.data2]), which=which, group=grp, n_groups=len(names))
        out["patient_counts"] = got
        out["Patient.Results"] = _patient_table(got[0], n_cases, columns=names, group_sets=got[1], summed=path_length)
    if gene_table:
        best = {L + 1: tallies[name].read() for L, name in enumerate(GENE_LEVELS[:path_length])}
        out["gene_best"] = best
        out["Gene.Results"] = gene_results(best, lsts, frames, (prep.ents_uid, prep.ents_symbol),
                                           (prep.ents2_uid, prep.ents2_symbol))
    if decorated_pvalues:
        dseed = int(api.load_library().gcre_mix64((int(seed) ^ DECORATED_SEED_TAG) & (2**64 - 1)))
        dec = decorated_table(out["GWASPA.Results"], genes, data, n_cases, n_ctrls, signed, n_permutations, strata,
                              dseed, device, path_length=path_length, exec_=ex, table=table)
        if dec is not None:
            out["Decorated.Pvalues.Results"] = dec
    if clump is not None:
        try:
            out["GWASPA.Results"] = clump_paths(out["GWASPA.Results"], genes, data, n_cases, n_ctrls, signed, r=clump,
                                                conditional=clump_conditional, threshold=threshold,
                                                n_permutations=n_permutations, strata=strata, seed=seed, device=device,
                                                exec_=ex, table=table)
        finally:
            ex.close()
    else:
        ex.close()
    return out
