"""The dense-matrix inputs as an R caller hands them over (pytest -m gpu, real MI355X): gcre_pathset_from_dense and
gcre_set_perm_cases through ctypes with col_major 0 and 1 on the same logical matrix, genotypes other than 0/1 (2, -1,
NA_integer_), labels other than 0/1, the threaded host packing past its 4e6-cell switch, and -- in one child process with
GCRE_DEVICE_PACK=1 -- the two device packing kernels.  The reference is numpy (np.packbits) in tests/input_roads.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import input_roads as ir
from geneticscre_amd import api

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", ir.DENSE_N)
@pytest.mark.parametrize("method", [1, 2])
def test_dense_rows_in_both_layouts_equal_numpy(method, n):
    """PathSet::load (gcre_paths.h:56-70) through pack_bits_host, row-major and column-major: every word, the zero (-) half,
    select with repeats, and the column-count assertion."""
    assert ir.check_dense_rows(method, n) == 2 * len(ir.DENSE_ROWS)


@pytest.mark.parametrize("n", ir.LABEL_N)
@pytest.mark.parametrize("K", ir.LABEL_K)
def test_permutation_labels_in_both_layouts_equal_numpy(K, n):
    """setPermutedCases (join_base.cpp:85-125) through pack_bits_host and k_masks_from_words: too few rows reused cyclically,
    surplus rows dropped (column-major: the `used < nrow` branch, whose columns keep the stride of the full matrix)."""
    assert ir.check_labels(K, n) == 2 * len(ir.label_rows(K))


# ---- the threaded form of pack_bits_host: taken at >= 4e6 cells, threads own word columns (column-major) or row blocks ----
BIG_ROWS, BIG_CASES, BIG_CTRLS = 2100, 1000, 1049      # 2,100 x 2,049 = 4.3e6 cells, 33 word columns


@pytest.fixture(scope="module")
def big():
    n = BIG_CASES + BIG_CTRLS
    assert BIG_ROWS * n >= 4e6 and (n + 63) // 64 == 33
    data = ir.draw(ir.GENOTYPES, (BIG_ROWS, n), 71)
    labels = ir.draw(ir.LABELS, (BIG_ROWS, n), 72)
    ex = api.JoinExec(1, BIG_CASES, BIG_CTRLS, BIG_ROWS)
    yield ex, data, labels, ir.expected_rows(data, 33, 1), ir.expected_masks(labels, BIG_CASES, BIG_ROWS, 33)
    ex.close()


@pytest.mark.parametrize("threads", [1, 5, 16])
@pytest.mark.parametrize("col_major", [0, 1])
def test_threaded_host_packing_gives_the_same_bits(big, col_major, threads, monkeypatch):
    """GCRE_PACK_THREADS is read on every call.  5 does not divide the 33 word columns (nor the 2,100 rows evenly into
    words); 1 is the serial form at the same size."""
    ex, data, labels, want_rows, want_masks = big
    monkeypatch.setenv("GCRE_PACK_THREADS", str(threads))
    ps = api.PathSet(ex, ir.from_dense(ex, data, col_major))
    np.testing.assert_array_equal(ps.to_numpy(), want_rows)
    ps.free()
    ex.set_permuted_masks(np.zeros((1, 33), np.uint64))
    ir.set_labels(ex, labels, col_major)
    np.testing.assert_array_equal(ir.all_masks(ex), want_masks)


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_join_behind_column_major_inputs_equals_the_oracle(method):
    ir.check_join_behind_column_major_inputs(method)


def test_device_packing_kernels_in_a_child_process():
    """GCRE_DEVICE_PACK=1 (read once per process, hence the child): all dense-row and label cases above and one join per
    method run again with k_pack_dense (both layouts) and k_masks_from_ints packing on the device.  The host calls
    k_masks_from_ints with col_major = 0 only -- it gathers the rows of a column-major matrix on the host first -- so the
    kernel's own col_major branch has no caller and is not run here either."""
    env = dict(os.environ, GCRE_DEVICE_PACK="1", GCRE_HOST_TIMING="1", GCRE_QUIET="1")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_pack_child.py")
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    done = json.loads(r.stdout.strip().splitlines()[-1])
    assert done == {"dense_sets": 2 * len(ir.DENSE_N) * len(ir.DENSE_ROWS) * 2,
                    "label_sets": sum(len(ir.label_rows(K)) for K in ir.LABEL_K) * len(ir.LABEL_N) * 2, "joins": 2}
    # the host-side timers report every host step they wrap: the packing steps are not among them in this process
    assert "[host] new_pathset" in r.stderr
    assert "pack genotypes (host)" not in r.stderr and "pack permutations (host)" not in r.stderr
