#!/bin/bash
# BASELINE configs that are not the default bench line: C3 (synthetic 10k-node lattice, HBM-roofline run) and C5 (high-res
# lattice, single-tick latency with the follow-mode profile on every tick).   tools/extra_configs.sh [out dir]   (default out/)
# -> c3_bench.json, c5_latency.json, c5_latency_100m.json
OUT=${1:-out}; mkdir -p $OUT
python bench.py --full --workload c3 --batch 8192 --steps 50 --warmup 5 --latency-ticks 500 > $OUT/c3_bench.json 2> $OUT/c3_bench.err
tail -c 400 $OUT/c3_bench.err
python tools/c5_latency.py 300 > $OUT/c5_latency.json 2> $OUT/c5_latency.err
tail -c 400 $OUT/c5_latency.err
python tools/c5_latency.py 100 > $OUT/c5_latency_100m.json 2> $OUT/c5_latency_100m.err
cut -c1-300 $OUT/c3_bench.json; cat $OUT/c5_latency.json $OUT/c5_latency_100m.json
