#!/bin/bash
# Counters of match_finish_kernel, for the product and for every other build of the library named as an argument
# (paths below the repository root, e.g. orthosfm_amd/lib/exp/lib_parent.so): one rocprofv3 --pmc pass per counter
# set and build, nothing else collected in those passes.
#   PMC_SETS="FETCH_SIZE;WRITE_SIZE"   replaces the default sets (semicolon-separated)
#   BENCH_ARGS="--steps 1 --warmup 0"  replaces the workload (default: one step of the full bench at 24 views)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${OUT:-.}" && cd "${OUT:-.}" && pwd)
cd /tmp && export TMPDIR=/tmp
SETS=${PMC_SETS:-"SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_VMEM_RD;SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INST_CYCLES_VMEM SQ_ACTIVE_INST_VMEM SQ_INSTS_LDS SQ_ACTIVE_INST_LDS;TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum TCC_REQ_sum;TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum TCP_TA_TCP_STATE_READ_sum TCP_PENDING_STALL_CYCLES_sum"}
ARGS=${BENCH_ARGS:-"--full --views 24 --steps 1 --warmup 0"}
for lib in "" "$@"; do
  tag=$( [ -z "$lib" ] && echo product || basename "$lib" .so )
  if [ -z "$lib" ]; then unset OSFM_HIP_LIBRARY; else export OSFM_HIP_LIBRARY=$R/$lib; fi
  i=0
  echo "$SETS" | tr ';' '\n' | while read -r set; do
    i=$((i+1))
    echo "== $tag: $set"
    timeout -k 10 300 rocprofv3 --pmc $set --kernel-include-regex "match_finish_kernel" --output-format csv -d $OUT/pmcf_${tag}_$i -- python $R/bench.py $ARGS --no-ba --no-verify --no-cpu-baseline > $OUT/pmcf_${tag}_$i.log 2>&1 || echo "set $i failed"
    f=$(find $OUT/pmcf_${tag}_$i -name "*counter_collection.csv" | head -1)
    [ -n "$f" ] && python $R/tools/pmc_summary.py $f match_finish_kernel
    rm -rf $OUT/pmcf_${tag}_$i
  done
done
