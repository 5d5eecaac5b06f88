#!/bin/bash
# profiles/ab_i8_sample.sh <parent libexpann_hip.so> [rounds] [part] -- the int8 sampled pass of a speculating int8-filter
# search (option "i8_sample") against the parent commit's build on one MI355X, as
# profiles/ab_rerank_rounds.sh.  part "ab" (default): bench.py --steps 60 --warmup 5 at the default shape (C2), three
# arms alternating: the parent's library, this build, this build with EXPANN_I8_SAMPLE=0 (the fp16 pass: what the
# other changes of the commit -- the statistics sum's place in the select -- are worth alone).  part "guard": the guard
# shapes, parent and new alternating (GUARD_ROUNDS, default 2).  part "trace": one kernel trace per arm (rocprofv3
# --kernel-trace --stats, a run of its own, never timed against the others): the per-kernel statistics, the step's tail
# and the select stages' start / end times (profiles/redo_tail_overlap.py).  Every GPU step runs under its own timeout
# and the script stops at the first step that fails.
PARENT=${1:?path of the parent build\'s libexpann_hip.so}
ROUNDS=${2:-5}
PART=${3:-ab}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
D=${OUT_DIR:-bench_out}  # where the lines, the traces and the error logs go
mkdir -p "$D"
OUT=$D/i8_sample_$PART.txt
line() { python -c "
import sys,json
j=json.loads([l for l in sys.stdin.read().splitlines() if l.startswith('{\"metric\"')][-1]); r=j['roofline']
print('%-34s %.4f %-28s %.4f %s' % ('$1', j['ms_per_step'], r['kernel'], r['kernel_ms'], r['candidates_per_query']))"; }
run() {  # run <tag> <lib or ""> bench args...
  local tag=$1 lib=$2; shift 2
  EXPANN_LIB=$lib timeout -k 10 240 python bench.py "$@" 2>$D/i8_sample.err | line $tag > $D/i8_sample.line || { tail -5 $D/i8_sample.err; exit 1; }
  cat $D/i8_sample.line | tee -a $OUT
}
if [ "$PART" = ab ]; then
  : > $OUT
  for i in $(seq 1 $ROUNDS); do
    run c2_parent_$i "$PARENT" --gpus 1 --steps 60 --warmup 5
    run c2_new_$i "" --gpus 1 --steps 60 --warmup 5
    EXPANN_I8_SAMPLE=0 run c2_new_i8_sample_0_$i "" --gpus 1 --steps 60 --warmup 5
  done
elif [ "$PART" = guard ]; then
  : > $OUT
  for i in $(seq 1 ${GUARD_ROUNDS:-2}); do
    for shape in "k100_rows1.25M --rows 1250000 --k 100 --steps 30" "queries1000 --queries 1000 --steps 60" \
                 "clustered_1000 --clustered 1000 --steps 30" "sift_like --sift-like --steps 40"; do
      set -- $shape; tag=$1; shift
      run ${tag}_parent_$i "$PARENT" "$@" --warmup 5
      run ${tag}_new_$i "" "$@" --warmup 5
    done
  done
else
  for arm in parent new; do
    lib=""; [ $arm = parent ] && lib=$PARENT
    rm -rf $D/trace_$arm
    EXPANN_LIB=$lib timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $D/trace_$arm -o t -- \
      python bench.py --gpus 1 --steps 20 --warmup 5 > $D/trace_$arm.log 2>&1 || { tail -5 $D/trace_$arm.log; exit 1; }
    cp "$(find $D/trace_$arm -name '*kernel_stats.csv' | head -1)" $D/i8_sample_kernel_stats_$arm.csv || exit 1
    python profiles/redo_tail_overlap.py "$(find $D/trace_$arm -name '*kernel_trace.csv' | head -1)" | tee $D/i8_sample_overlap_$arm.txt || exit 1
  done
fi
