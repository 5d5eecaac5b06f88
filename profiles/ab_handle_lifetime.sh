#!/bin/bash
# profiles/ab_handle_lifetime.sh <parent libexpann_hip.so> [rounds] -- the handle's regrouped host state against the
# parent commit's build on one MI355X: bench.py --steps 60 --warmup 5 at the default shape, the two libraries
# alternating (EXPANN_LIB), then the medians.  The device code of the two builds is byte-identical, so the expectation
# is no difference: the new build's median step time must lie within the min-max range of the parent's own runs, and a
# parent spread beyond 2 % of its median says the machine was busy (repeat the call).  Every GPU step runs under its
# own timeout and the script stops at the first step that fails.  Lines go to $OUT_DIR/handle_lifetime_ab.txt.
PARENT=${1:?path of the parent build\'s libexpann_hip.so}
ROUNDS=${2:-3}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
D=${OUT_DIR:-bench_out}
mkdir -p "$D"
OUT=$D/handle_lifetime_ab.txt
: > $OUT
run() {  # run <tag> <lib or "">
  EXPANN_LIB=$2 timeout -k 10 240 python bench.py --gpus 1 --steps 60 --warmup 5 2>$D/handle_lifetime_ab.err > $D/handle_lifetime_ab.run \
    || { tail -5 $D/handle_lifetime_ab.err; exit 1; }
  python -c "
import sys,json
j=json.loads([l for l in open('$D/handle_lifetime_ab.run').read().splitlines() if l.startswith('{\"metric\"')][-1]); r=j['roofline']
print('%-12s %.4f %-28s %.4f %s' % ('$1', j['ms_per_step'], r['kernel'], r['kernel_ms'], r['candidates_per_query']))" | tee -a $OUT
}
for i in $(seq 1 $ROUNDS); do
  run parent_$i "$PARENT" || exit 1
  run new_$i "" || exit 1
done
python -c "
import statistics as s
rows=[l.split() for l in open('$OUT')]
p=[float(r[1]) for r in rows if r[0].startswith('parent_')]; n=[float(r[1]) for r in rows if r[0].startswith('new_')]
mp, mn = s.median(p), s.median(n)
print('parent ms_per_step: median %.4f min %.4f max %.4f spread %.2f %% of the median' % (mp, min(p), max(p), 100 * (max(p) - min(p)) / mp))
print('new    ms_per_step: median %.4f min %.4f max %.4f' % (mn, min(n), max(n)))
print('new median within the parent\'s min-max range: %s' % ('yes' if min(p) <= mn <= max(p) else 'NO'))" | tee -a $OUT
