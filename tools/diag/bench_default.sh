#!/bin/bash
# the full bench line (--full) with its wall time, and the figures beside the headline; OUT: output directory (default build/bench)
cd "$(dirname "$0")/../.."
OUT=${OUT:-build/bench}
mkdir -p "$OUT"
s=$(date +%s)
python bench.py --full > "$OUT"/bench_full.json 2> "$OUT"/bench_full.err
echo "rc=$? wall=$(( $(date +%s) - s )) s"
python - "$OUT"/bench_full.json <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["roofline"]["frac"], d["cpu_baseline"]["value"])
for k,v in d["other_configs"].items():
    if isinstance(v, dict): print(k, v.get("value"), v.get("ms_per_step"))
print({k: v.get("value") for k,v in d["sensitivity"].items() if isinstance(v, dict)})
print(d["end_to_end"].get("ms"), d["steady_state"].get("ms_per_step"))
PY
