#!/bin/bash
# profiles/ab_rerank_rounds.sh <parent libexpann_hip.so> [rounds] [part] -- the select's two-round exact re-rank of the
# int8 filter's lists against the parent commit's build on one MI355X.  part "ab" (default): bench.py
# --steps 60 --warmup 5 at the default shape (C2), the two libraries alternating (EXPANN_LIB), then one arm of the
# new build with rerank_rounds = 1; PART1_LIB (optional): a build of the new select alone, without bp in the hit logs'
# fourth word, as a third alternating arm -- each part's share.  part "guard": the guard shapes, parent and new alternating (GUARD_ROUNDS,
# default 2).  part "rows": the rows the selects re-score per query at C2 with one round and two (untimed,
# profiles/rerank_rows_c2.py).  part "trace": one kernel trace per arm (rocprofv3 --kernel-trace --stats, a run of its
# own), the per-kernel statistics and the select stages' start / end times.  Every GPU step runs under its own
# timeout and the script stops at the first step that fails.
PARENT=${1:?path of the parent build\'s libexpann_hip.so}
ROUNDS=${2:-3}
PART=${3:-ab}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
D=${OUT_DIR:-bench_out}  # where the lines, the traces and the error logs go
mkdir -p "$D"
OUT=$D/rerank_rounds_$PART.txt
line() { python -c "
import sys,json
j=json.loads([l for l in sys.stdin.read().splitlines() if l.startswith('{\"metric\"')][-1]); r=j['roofline']
print('%-34s %.4f %-28s %.4f %s' % ('$1', j['ms_per_step'], r['kernel'], r['kernel_ms'], r['candidates_per_query']))"; }
run() {  # run <tag> <lib or ""> bench args...
  local tag=$1 lib=$2; shift 2
  EXPANN_LIB=$lib timeout -k 10 240 python bench.py "$@" 2>$D/rerank_rounds.err | line $tag > $D/rerank_rounds.line || { tail -5 $D/rerank_rounds.err; exit 1; }
  cat $D/rerank_rounds.line | tee -a $OUT
}
if [ "$PART" = ab ]; then
  : > $OUT
  for i in $(seq 1 $ROUNDS); do
    run c2_parent_$i "$PARENT" --gpus 1 --steps 60 --warmup 5
    run c2_new_$i "" --gpus 1 --steps 60 --warmup 5
    [ -n "$PART1_LIB" ] && run c2_new_select_only_$i "$PART1_LIB" --gpus 1 --steps 60 --warmup 5
  done
  EXPANN_RERANK_ROUNDS=1 run c2_new_rerank_rounds_1 "" --gpus 1 --steps 60 --warmup 5
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
elif [ "$PART" = rows ]; then
  timeout -k 10 300 python profiles/rerank_rows_c2.py 2>$D/rerank_rounds.err | tee $OUT || { tail -5 $D/rerank_rounds.err; exit 1; }
else
  for arm in parent new; do
    lib=""; [ $arm = parent ] && lib=$PARENT
    rm -rf $D/trace_$arm
    EXPANN_LIB=$lib timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $D/trace_$arm -o t -- \
      python bench.py --gpus 1 --steps 20 --warmup 5 > $D/trace_$arm.log 2>&1 || { tail -5 $D/trace_$arm.log; exit 1; }
    cp "$(find $D/trace_$arm -name '*kernel_stats.csv' | head -1)" $D/rerank_rounds_kernel_stats_$arm.csv || exit 1
    python profiles/redo_tail_overlap.py "$(find $D/trace_$arm -name '*kernel_trace.csv' | head -1)" | tee $D/rerank_rounds_overlap_$arm.txt || exit 1
  done
fi
