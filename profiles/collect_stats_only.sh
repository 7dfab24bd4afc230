#!/bin/bash
# Run on the GPU box from the repo root:  bash profiles/collect_stats_only.sh r02_final
# The kernel-trace + stats pass of profiles/collect.sh alone (the two PMC passes are unchanged by host-side work);
# writes <tag>_kernel_stats.md straight from the rocpd database, under build/prof/ (ignored by git).
TAG=${1:-r02_final}
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$R/build/prof
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_stats
mkdir -p $OUT
rocprofv3 --kernel-trace --stats -d $OUT/prof_stats -o $TAG -- python $R/bench.py --steps 3 --warmup 1 --full --no-cpu-baseline --no-other-configs --no-end-to-end > $OUT/${TAG}_bench_under_rocprof.log 2>&1
cd $R && python3 - "$TAG" "$OUT" <<'PY'
import sqlite3, sys, glob
tag, out = sys.argv[1], sys.argv[2]
db = glob.glob(f"{out}/prof_stats/**/{tag}_results.db", recursive=True)[0]
c = sqlite3.connect(db)
rows = list(c.execute("select name, total_calls, total_duration, average, percentage from top_kernels"))
lines = [f"# rocprofv3 --kernel-trace --stats — bench.py --steps 3 --warmup 1 (configs[1], 10k docs, 1 MI355X), tag {tag}", "",
         "| kernel | calls | total ms | avg ms | % |", "|---|---:|---:|---:|---:|"]
for name, calls, tot, avg, pct in rows:
    lines.append(f"| {name} | {calls} | {tot / 1e3:.3f} | {avg / 1e3:.4f} | {pct:.2f} |")
open(f"{out}/{tag}_kernel_stats.md", "w").write("\n".join(lines) + "\n")
print("\n".join(lines[:12]))
PY
grep '^{"metric"' $OUT/${TAG}_bench_under_rocprof.log > $OUT/${TAG}_bench_line.json
rm -rf $OUT/prof_stats
