#!/bin/bash
# Kernel trace of a bench command -> per-kernel table.  bash tools/trace_bench.sh TAG [bench args...]
TAG=$1; shift
OUT=${OUT:-tool_out}
export TMPDIR=/tmp
mkdir -p "$OUT"
rm -rf $OUT/${TAG}_prof
rocprofv3 --kernel-trace -d $OUT/${TAG}_prof -- python bench.py --full --no_cpu_baseline --no_roofline --no_children --steps 10 --warmup 3 "$@" > $OUT/${TAG}_prof.log 2>&1
DB=$(find $OUT/${TAG}_prof -name '*.db' | head -1)
python tools/rocpd_stats.py $DB 70 $TRACE_PAT > $OUT/${TAG}_kernel_trace_stats.txt 2>&1
rm -rf $OUT/${TAG}_prof
tail -1 $OUT/${TAG}_prof.log | cut -c1-200
