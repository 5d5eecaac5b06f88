#!/bin/bash
# profiles/ab_spec_tau.sh <parent libexpann_hip.so> [rounds] -- speculative thresholds against the
# parent commit's build on one MI355X: bench.py --steps 60 --warmup 5 at the default shape, the two libraries
# alternating (EXPANN_LIB), then the other shapes once per arm and round.  Every GPU step runs under its own
# timeout and the script stops at the first step that fails.
PARENT=${1:?path of the parent build\'s libexpann_hip.so}
ROUNDS=${2:-3}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
D=${OUT_DIR:-bench_out}  # where the lines and the error logs go
mkdir -p "$D"
OUT=$D/ab_spec_tau.txt
: > $OUT
line() { python -c "
import sys,json
j=json.loads([l for l in sys.stdin.read().splitlines() if l.startswith('{\"metric\"')][-1]); r=j['roofline']
print('%-34s %.4f %-28s %.4f %s' % ('$1', j['ms_per_step'], r['kernel'], r['kernel_ms'], r['candidates_per_query']))"; }
run() {  # run <tag> <lib or ""> bench args...
  local tag=$1 lib=$2; shift 2
  EXPANN_LIB=$lib timeout -k 10 240 python bench.py "$@" 2>$D/ab_spec_tau.err | line $tag > $D/ab_spec_tau.line || { tail -5 $D/ab_spec_tau.err; exit 1; }
  cat $D/ab_spec_tau.line | tee -a $OUT
}
for i in $(seq 1 $ROUNDS); do
  run c2_parent_$i "$PARENT" --steps 60 --warmup 5
  run c2_new_$i "" --steps 60 --warmup 5
done
for i in $(seq 1 $ROUNDS); do
  for shape in "clustered_1000 --clustered 1000 --steps 30" "k100_rows1.25M --rows 1250000 --k 100 --steps 30" "queries1000 --queries 1000 --steps 60" \
               "dim64 --dim 64 --steps 40" "sift_like --sift-like --steps 40"; do
    set -- $shape; tag=$1; shift
    run ${tag}_parent_$i "$PARENT" "$@" --warmup 5
    run ${tag}_new_$i "" "$@" --warmup 5
  done
done
