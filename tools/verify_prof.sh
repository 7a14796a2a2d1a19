# Device time of the RANSAC-F kernels in the bench's pass with geometric verification (a --full leg).
#   OUT=<dir> tools/verify_prof.sh      (OUT: where the trace goes while it is read; default the working directory)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${OUT:-.}" && cd "${OUT:-.}" && pwd)
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_v
rocprofv3 --kernel-trace --stats -d $OUT/prof_v -- python $R/bench.py --full --no-ba --no-cpu-baseline --steps 2 --warmup 1 > $OUT/prof_v.log 2>&1
db=$(find $OUT/prof_v -name "*.db" | head -1)
python $R/tools/rocpd_stats.py $db | grep -i "ransac\|gather_inl" | cut -c1-130
rm -rf $OUT/prof_v
