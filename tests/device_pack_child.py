"""Run by tests/test_gpu_inputs.py in ONE fresh process with GCRE_DEVICE_PACK=1 (the library reads that knob once per
process): every dense-row and label case of tests/input_roads.py and one join per method, now with k_pack_dense and
k_masks_from_ints packing the bits on the device.  Checks against numpy itself; prints one JSON line and exits 0, or
fails with the assertion."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for d in (HERE, os.path.dirname(HERE)):
    if d not in sys.path:
        sys.path.insert(0, d)


def main() -> int:
    assert os.environ.get("GCRE_DEVICE_PACK") == "1", "start this with GCRE_DEVICE_PACK=1"
    os.environ.setdefault("GCRE_QUIET", "1")
    import input_roads as ir
    dense = sum(ir.check_dense_rows(method, n) for method in (1, 2) for n in ir.DENSE_N)
    labels = sum(ir.check_labels(K, n) for K in ir.LABEL_K for n in ir.LABEL_N)
    for method in ("method1", "method2"):
        ir.check_join_behind_column_major_inputs(method)
    print(json.dumps({"dense_sets": dense, "label_sets": labels, "joins": 2}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
