#!/bin/bash
# The four bench lines of the round (C2 default, C3-C5 by --workload), each with its CPU baseline (--full), one JSON line each as
# <dir>/bench_<tag>*.json:   bash tools/bench_all.sh <tag> <dir>
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"; TAG=${1:-x}; OUT=${2:?usage: tools/bench_all.sh <tag> <dir>}; mkdir -p "$OUT"
timeout 300 python bench.py --full > "$OUT/bench_${TAG}.json" 2> "$OUT/bench_${TAG}.err"
for wl in smallpt dragon tr15_like; do
  timeout 400 python bench.py --full --workload $wl --steps 2 --warmup 1 > "$OUT/bench_${TAG}_$wl.json" 2> "$OUT/bench_${TAG}_$wl.err"
done
python - <<PY
import json, glob
for p in sorted(glob.glob("$OUT/bench_${TAG}*.json")):
    try:
        d = json.loads(open(p).read().strip().splitlines()[-1])
        print(p.split("/")[-1], d["value"], d["unit"], "frac", d["roofline"]["frac"], "cpu", d.get("cpu_baseline", {}).get("value"), "ms/step", d["ms_per_step"])
    except Exception as e:
        print(p, "unreadable", e)
PY
