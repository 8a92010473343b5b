"""The oracle against the reference's own scoring code on seeded random problems (CPU).  Same draw as
tests/test_gpu_fuzz.py; compared per level: every score (bit pattern), the ids in the reference's heap order, the counts, every f32 null
maximum and the hash of the kept path rows, as `ref_driver --bin` prints them.  The first FUZZ_GOLDEN_CASES cases compare
against those outputs committed under tests/golden/ref_cases/ (tests/golden/make_ref_goldens.py); later ones
(GCRE_FUZZ_CASES=300 for a long run) need oracle/_ref/ref_driver, the partial reference build."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
from geneticscre_amd.harness_io import problem_digest, write_problem_bin
from helpers import FUZZ_GOLDEN_CASES, fnv_rows, fuzz_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_cases")
N_CASES = min(int(os.environ.get("GCRE_FUZZ_CASES", "4")), 2000)


def reference_outputs(case, cfg, p, tmp_path):
    """What the reference's scoring code printed for this case: the committed golden when it was cut from this very draw
    (GCRE_FUZZ_LIGHT changes some draws), else a run of the partial reference build."""
    path = os.path.join(GOLDEN, f"fuzz{case}.json")
    if case < FUZZ_GOLDEN_CASES:
        ref = json.load(open(path))
        if ref["_case"]["draw"] == cfg:
            assert problem_digest(p) == ref["_case"]["input_sha256"], f"fuzz{case}: the generator no longer reproduces the golden's inputs"
            return ref
    if not os.path.exists(BINARY):
        pytest.skip("no committed golden for this draw and no partial reference build (oracle/_ref/ref_driver)")
    dump = str(tmp_path / "case.gcrebin")
    write_problem_bin(dump, p, nthreads=0)
    r = subprocess.run([BINARY, "--bin", dump], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-400:]
    return json.loads(r.stdout)


@pytest.mark.parametrize("case", range(N_CASES))
def test_oracle_matches_reference_code_on_random_problems(case, tmp_path):
    cfg, p = fuzz_problem(case)
    ref = reference_outputs(case, cfg, p, tmp_path)
    got = oracle.process_paths(p, order="reference", nthreads=0)
    for lvl in range(1, cfg["length"] + 1):
        e, g = ref[f"lst{lvl}"], got[f"lst{lvl}"]
        assert [f"{int(b):016x}" for b in g.scores.view(np.uint64)] == e["scores"], (case, lvl, cfg)
        assert g.src.tolist() == e["src"] and g.trg.tolist() == e["trg"], (case, lvl, cfg)
        assert g.cases.tolist() == e["cases"] and g.ctrls.tolist() == e["ctrls"], (case, lvl, cfg)
        assert [f"{int(b):08x}" for b in g.null.view(np.uint32)] == e["null"], (case, lvl, cfg)
    for lvl, key in ((1, "lst1a"), (2, "lst2"), (3, "lst3")):
        if lvl < cfg["length"]:
            assert fnv_rows(got[f"paths{lvl}"]) == ref[key]["kept_hash"], (case, key, cfg)
