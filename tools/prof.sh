#!/bin/bash
# rocprofv3 kernel-trace + stats of the whole bench (--full: every leg); counters are collected
# in runs of their own (tools/pmc.sh).  Output under $OUT (default prof_out/).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
OUT=${OUT:-prof_out}
mkdir -p $OUT/prof
make -C rag-snvbert_amd -j16 > $OUT/make.log 2>&1 || exit 3
TAG=${TAG:-r1}
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof/$TAG -o bench \
  -- python3 bench.py --full --steps ${BSTEPS:-5} --warmup 2 --cpu-baseline 0 > $OUT/prof_bench_$TAG.log 2>&1
rc=$?
echo "rocprof rc=$rc"; tail -3 $OUT/prof_bench_$TAG.log
find $OUT/prof -name "*stats*" | head
exit $rc
