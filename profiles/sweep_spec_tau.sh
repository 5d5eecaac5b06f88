#!/bin/bash
# profiles/sweep_spec_tau.sh [bench args...] -- the rank j of the speculative threshold (EXPANN_SPEC_RANK; j = k: off)
# against the sampled share 1/frac (--sample-frac) at one shape, three rounds, bench.py --steps 40 --warmup 5.
# SWEEP_J / SWEEP_FRAC name the grid.  One line per run: j frac ms_per_step scan_ms candidates_per_query.
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
D=${OUT_DIR:-bench_out}  # where the lines and the error logs go
mkdir -p "$D"
for i in 1 2 3; do
  for f in ${SWEEP_FRAC:-16 24 32}; do
    for j in ${SWEEP_J:-3 4 5 10}; do
      EXPANN_SPEC_RANK=$j timeout -k 10 240 python bench.py --steps 40 --warmup 5 --sample-frac $f "$@" 2>$D/sweep_spec_tau.err | python -c "
import sys,json
j=json.loads([l for l in sys.stdin.read().splitlines() if l.startswith('{\"metric\"')][-1]); r=j['roofline']
print('j %3d frac %3d round $i  %.4f ms  scan %.4f ms  %s cand/q  %s' % ($j, $f, j['ms_per_step'], r['kernel_ms'], r['candidates_per_query'], r['kernel']))" || { tail -5 $D/sweep_spec_tau.err; exit 1; }
    done
  done
done
