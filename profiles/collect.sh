#!/bin/bash
# Run on the GPU box from the repo root:  bash profiles/collect.sh r01
# Three separate rocprofv3 passes of the same bench command (kernel trace + stats, FETCH_SIZE, WRITE_SIZE), written under
# build/prof/ (ignored by git); profiles/extract_rocprof.py then turns the three databases into the summaries committed in profiles/.
# The bench runs with --full: the summaries price the two serialized passes that close the roofline leg.
TAG=${1:-r01}
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$R/build/prof
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_stats $OUT/prof_fetch $OUT/prof_write
mkdir -p $OUT
rocprofv3 --kernel-trace --stats -d $OUT/prof_stats -o $TAG -- python $R/bench.py --steps 3 --warmup 1 --full --no-cpu-baseline --no-other-configs --no-end-to-end > $OUT/${TAG}_bench_under_rocprof.log 2>&1
rocprofv3 --pmc FETCH_SIZE -d $OUT/prof_fetch -o $TAG -- python $R/bench.py --steps 2 --warmup 1 --full --no-cpu-baseline --no-other-configs --no-end-to-end > $OUT/${TAG}_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE -d $OUT/prof_write -o $TAG -- python $R/bench.py --steps 2 --warmup 1 --full --no-cpu-baseline --no-other-configs --no-end-to-end > $OUT/${TAG}_write.log 2>&1
cd $R && python3 profiles/extract_rocprof.py $OUT/prof_stats/${TAG}_results.db $OUT/prof_fetch/${TAG}_results.db $OUT/prof_write/${TAG}_results.db $TAG
mkdir -p $OUT/profiles && cp profiles/${TAG}_* $OUT/profiles/ && grep '^{"metric"' $OUT/${TAG}_bench_under_rocprof.log > $OUT/profiles/${TAG}_bench_under_rocprof.log
ls -la $OUT/profiles
