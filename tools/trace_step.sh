R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${OUT:-.}" && cd "${OUT:-.}" && pwd)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d $OUT/trace1 -- python $R/bench.py --full --no-ba --no-verify --no-cpu-baseline --steps 2 --warmup 1 > $OUT/trace1.log 2>&1
find $OUT/trace1 -name "*.csv" | head
