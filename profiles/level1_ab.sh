#!/bin/bash
# Lowering level 1 against level 0 in one tree on one box (GFHIP_LEVEL=0 runs the code object of the lowering without a level).
#     bash profiles/level1_ab.sh <output directory>          from the repository root, after __graft_entry__.build()
# Bits first: the dumped outputs of both levels must be byte-identical before anything is timed.  Then three alternating pairs of
# the same bench command, one bench.py at its defaults, rocprofv3 --kernel-trace --stats at both levels, and the counters in runs
# of their own (no trace domain next to --pmc).  profiles/summarize.py turns the directories into level1_kernel_stats.csv,
# level1_pmc_summary.csv and the entries of traffic.json; the bench lines are level1_ab.jsonl.
# Every step that uses the GPU runs under a time limit of its own, and the script ends at the first one that fails.
set -o pipefail
R=$(pwd); OUT=$(mkdir -p "$1" && cd "$1" && pwd) || exit 2
D=$(mktemp -d); mkdir -p $D/l0 $D/l1
B="python3 $R/bench.py --no-cpu-baseline --no-extra"
GFHIP_LEVEL=0 timeout -k 10 300 $B --dump-outputs $D/l0 > $OUT/dump_level0.json 2> $OUT/dump_level0.err || exit 1
timeout -k 10 300 $B --dump-outputs $D/l1 > $OUT/dump_level1.json 2> $OUT/dump_level1.err || exit 1
for f in $D/l0/*.npy; do
    if cmp -s $f $D/l1/$(basename $f); then echo "identical $(basename $f) $(stat -c %s $f) bytes"; else echo "DIFFERENT $(basename $f)"; fi
done | tee $OUT/dump_compare.txt
grep -q DIFFERENT $OUT/dump_compare.txt && { echo "the dumped outputs differ: nothing is timed"; exit 1; }
[ $(grep -c identical $OUT/dump_compare.txt) -ge 9 ] || { echo "dump files are missing"; exit 1; }
rm -rf $D
for pair in 1 2 3; do
    GFHIP_LEVEL=0 timeout -k 10 300 $B > $OUT/level0_$pair.json 2>> $OUT/bench.err || exit 1
    timeout -k 10 300 $B > $OUT/level1_$pair.json 2>> $OUT/bench.err || exit 1
done
timeout -k 10 500 python3 $R/bench.py --gpus 1 > $OUT/bench_default.json 2>> $OUT/bench.err || exit 1
cd /tmp && export TMPDIR=/tmp
for level in 0 1; do
    export GFHIP_LEVEL=$level
    timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats_level$level -- $B --steps 200 --warmup 10 > $OUT/stats_level$level.log 2>&1 || exit 1
    timeout -k 10 400 rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES --output-format csv -d $OUT/pmc_sq_level$level -- $B --steps 20 --warmup 2 > $OUT/pmc_sq_level$level.log 2>&1 || exit 1
    timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch_level$level -- $B --steps 20 --warmup 2 > $OUT/pmc_fetch_level$level.log 2>&1 || exit 1
    timeout -k 10 400 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write_level$level -- $B --steps 20 --warmup 2 > $OUT/pmc_write_level$level.log 2>&1 || exit 1
    (cd $R && python3 profiles/summarize.py traffic $OUT/pmc_fetch_level$level.log $OUT/traffic_level$level.json gfhip_solver_kernel=$OUT/pmc_fetch_level$level,$OUT/pmc_write_level$level) || exit 1
done
unset GFHIP_LEVEL
cd $R && python3 profiles/summarize.py round $OUT $OUT/level1
echo collected
