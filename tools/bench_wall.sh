#!/bin/bash
# Wall time of a plain bench run and of a --full one (default arguments otherwise), and what the plain run spends outside its steps:
# wall - (steps + warmup) x ms_per_step.   tools/bench_wall.sh [out dir]   (default out/) -> bench_plain.json, bench_full.json
OUT=${1:-out}; mkdir -p $OUT
for MODE in plain full; do
  F=""; [ $MODE = full ] && F=--full
  s=$(date +%s.%N); python bench.py $F > $OUT/bench_$MODE.json 2> $OUT/bench_$MODE.err; rc=$?; e=$(date +%s.%N)
  echo "$MODE: rc $rc  wall $(python -c "print('%.1f' % ($e - $s))") s"
  python - $OUT/bench_$MODE.json $s $e <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[1]).read().splitlines() if l.startswith("{")][-1])
wall = float(sys.argv[3]) - float(sys.argv[2])
print("  value %.4g %s  ms_per_step %.4f  outside the steps %.1f s" % (d["value"], d["unit"], d["ms_per_step"],
                                                                     wall - (d["steps"] + d["warmup"]) * d["ms_per_step"] * 1e-3))
if "roofline" in d:
    print("  roofline frac %.3f  latency p50 %s us  cpu_baseline %s" % (d["roofline"]["frac"], d["latency_us"]["p50"], (d.get("cpu_baseline") or {}).get("value")))
PY
done
