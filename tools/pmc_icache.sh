#!/bin/bash
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$GRAFT_REPO_ROOT/gpurun_out/$1; shift
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --pmc SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE SQ_IFETCH SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES --output-format csv -d $OUT/ic -- python3 $R/bench.py --steps 5 --warmup 1 --full --no-cpu-baseline > $OUT/ic.log 2>&1
rocprofv3 --kernel-trace --pmc SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_IFETCH_LEVEL SQ_INST_LEVEL_LDS SQ_BUSY_CU_CYCLES SQ_INSTS_SALU SQ_INSTS_LDS --output-format csv -d $OUT/ic2 -- python3 $R/bench.py --steps 5 --warmup 1 --full --no-cpu-baseline > $OUT/ic2.log 2>&1
python3 $GRAFT_REPO_ROOT/tools/pmc_summarize.py $OUT
