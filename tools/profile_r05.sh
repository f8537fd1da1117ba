#!/bin/bash
# Round-5 profiles of the headline workload (partialorder_14), taken for several engine libraries in ONE job so that before and
# after come from the same box: per library one rocprofv3 kernel-trace stats run with STCSP_STREAM_EXPORT=0 (the kernel by itself,
# see profile_r04.sh) and one PMC pass of its own for the instruction counters (counters never together with tracing).
# usage: tools/profile_r05.sh tag=/path/to/libstcsp_hip.so [tag=...]     (e.g. before=... after=...)
# Raw output under $STCSP_PROFILE_RAW (default: profile_raw/r05/ in the repository, ignored by git); tools/profile_r05_summaries.py
# turns it into the files committed under profiles/.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
export TMPDIR=/tmp
OUT=${STCSP_PROFILE_RAW:-$R/profile_raw/r05}
mkdir -p $OUT
cd /tmp
B="python3 $R/bench.py --full --no-cpu-baseline --no-other-workloads"
for spec in "$@"; do
  tag=${spec%%=*}
  export STCSP_HIP_LIB=${spec#*=}
  STCSP_STREAM_EXPORT=0 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats_$tag -- $B --steps 5 --warmup 2 > $OUT/stats_$tag.json 2> $OUT/stats_$tag.err
  echo "stats $tag done"
  timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_SMEM SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVES SQ_WAVE_CYCLES --output-format csv -d $OUT/pmc_$tag -- $B --steps 1 --warmup 0 > $OUT/pmc_$tag.json 2> $OUT/pmc_$tag.err
  echo "pmc $tag done"
done
