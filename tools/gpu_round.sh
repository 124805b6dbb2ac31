#!/bin/bash
# One GPU-box session of a build round: parity tests, the full bench line, kernel stats, HBM traffic and lane utilisation counters.
# Test log, bench line and counter summaries land under $OUT/<tag>_* (default out/); tools/profile_round.sh and tools/pmc_pass.sh keep
# their own output folders, and tools/profile_summarise.py copies the summaries to profiles/.
#   tools/gpu_round.sh <tag> [skip-tests]
set -u
TAG=${1:-r02a}
OUT=${OUT:-out}
export TMPDIR=/tmp
mkdir -p $OUT
if [ "${2:-}" != "skip-tests" ]; then
  timeout 900 python -m pytest tests -m gpu -x -q > $OUT/${TAG}_gputest.log 2>&1
  echo "gpu tests rc=$?"; tail -5 $OUT/${TAG}_gputest.log
fi
timeout 600 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
echo "bench rc=$?"; cat $OUT/${TAG}_bench.json | head -c 6000; tail -3 $OUT/${TAG}_bench.err
tools/profile_round.sh ${TAG}
tools/pmc_pass.sh ${TAG}_lanes "SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU SQ_INSTS_SALU" > $OUT/${TAG}_lanes.txt 2>&1
tools/pmc_pass.sh ${TAG}_occ "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_LDS" > $OUT/${TAG}_occ.txt 2>&1
cat $OUT/${TAG}_lanes.txt $OUT/${TAG}_occ.txt | head -80
