#!/bin/bash
# Round evidence: the --full bench line + rocprofv3 kernel summary of the same command.
#   OUT=<dir> tools/refresh_profiles.sh r02 v1   ->  <dir>/<round>_bench_<tag>.json,
#   <dir>/<round>_bench_kernel_stats_<tag>.csv  (copy both into profiles/; default <dir>: the working directory)
set -e
round=${1:-r02}
tag=${2:-vX}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${OUT:-.}" && cd "${OUT:-.}" && pwd)
cd /tmp && export TMPDIR=/tmp
python $R/bench.py --full > $OUT/bench_$tag.log 2>&1
grep "^{" $OUT/bench_$tag.log | tail -1 > $OUT/${round}_bench_$tag.json
rm -rf $OUT/prof_$tag
rocprofv3 --kernel-trace --stats -d $OUT/prof_$tag -- python $R/bench.py --full --steps 5 --warmup 2 --no-e2e --no-cpu-baseline > $OUT/prof_$tag.log 2>&1
# (one database per traced process: bench.py's drop-in leg runs a host program of its own -- all of them are summed)
db=$(find $OUT/prof_$tag -name "*.db" | tr '\n' ' ')
if [ -n "$db" ]; then
  python $R/tools/rocpd_stats.py $db > $OUT/${round}_bench_kernel_stats_$tag.csv
else
  f=$(find $OUT/prof_$tag -name "*kernel_stats.csv" | head -1)
  cp $f $OUT/${round}_bench_kernel_stats_$tag.csv
fi
rm -rf $OUT/prof_$tag        # the trace itself is large; the summary is what is kept
# Second summary: a plain run, ONLY the headline launches (no BA, no RANSAC passes, no end-to-end job, no CPU
# baseline, no drop-in / realistic-operand legs), so that the AverageNs of match_tile_kernel<8, false, true, true>
# IS roofline.avg_launch_ms of the line printed by the same command.
rocprofv3 --kernel-trace --stats -d $OUT/prof_h_$tag -- python $R/bench.py --steps 10 --warmup 2 > $OUT/prof_h_$tag.log 2>&1
grep "^{" $OUT/prof_h_$tag.log | tail -1 > $OUT/${round}_bench_headline_only_$tag.json
db=$(find $OUT/prof_h_$tag -name "*.db" | tr '\n' ' ')
if [ -n "$db" ]; then
  python $R/tools/rocpd_stats.py $db > $OUT/${round}_bench_headline_only_kernel_stats_$tag.csv
else
  f=$(find $OUT/prof_h_$tag -name "*kernel_stats.csv" | head -1)
  cp $f $OUT/${round}_bench_headline_only_kernel_stats_$tag.csv
fi
rm -rf $OUT/prof_h_$tag
head -6 $OUT/${round}_bench_headline_only_kernel_stats_$tag.csv
head -8 $OUT/${round}_bench_kernel_stats_$tag.csv
python - <<PY
import json
d = json.load(open("$OUT/${round}_bench_$tag.json"))
print(d["value"], d["ms_per_step"], d["roofline"]["avg_launch_ms"], d["roofline"]["frac"])
PY
