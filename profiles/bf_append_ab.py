"""What an append to a built brute-force index costs (expann_append), on one MI355X, and that an index
which is never appended to searches as fast as the parent commit's.

    python profiles/bf_append_ab.py --parent-lib DIR [--rounds 3] > profiles/bf_append_ab.txt

DIR holds the other build's libexpann_hip.so (the parent commit's).  Every part runs in processes of its own, one at
a time, each under a time limit; the first that fails ends the run.
  (a) C2's plain search, `bench.py --gpus 1 --steps 60 --warmup 5`: per round the other build first and then this one,
      so the two alternate; this build's median is compared with the smallest and the largest of the other build's runs.
  (b) the other build, 1 M x d128 fp32 rows: expann_build at default options (upload + the fp16 copy) and under
      "scan_kernel" 1 set before the build (upload only, the copy is not made at build): the difference is ensure_f16,
      per row what converting a row costs there.
  (c) this build, the same index, 10 000 queries, k = 10, host-to-host wall times: destroy + add + build of the whole;
      appends of 1 / 1 000 / 100 000 rows within a reserved capacity, and of 1 000 rows without a reserve (the base and
      the fp16 copy grow by half: both are copied once); the first search after an append (the int8 filter's copy was
      dropped and is made again) against steady-state searches; searches of the appended index against searches of a
      fresh index of the same rows, the two in turn."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, D, MQ, K = 1_000_000, 128, 10_000, 10


def _data(extra):
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((N + extra, D), dtype=np.float32)
    top = int(np.argmax(np.abs(rows).max(axis=1)))
    rows[[0, top]] = rows[[top, 0]]  # (max |v| in the initial part: the appends extend the fp16 copy)
    return rows, rng.standard_normal((MQ, D), dtype=np.float32)


def _ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def parent_child():
    """(b) with whichever library EXPANN_LIB names; prints one JSON line"""
    from expann_amd import GpuBruteForceEngine
    rows, _ = _data(0)
    out = {"build_ms": [], "build_no_copy_ms": []}
    for _ in range(3):
        for key, opts in (("build_ms", ()), ("build_no_copy_ms", (("scan_kernel", 1),))):
            eng = GpuBruteForceEngine(D, "l2")
            for name, v in opts:
                eng.set_option(name, v)
            eng.store_many_vectors(rows)
            out[key].append(_ms(eng.build))
            eng.close()
    print(json.dumps(out))


def this_child():
    """(c) in this process; prints one JSON line"""
    from expann_amd import GpuBruteForceEngine
    extra = 1 + 1000 + 100_000
    rows, queries = _data(extra)
    out = {}

    def fresh(n, reserve=0):
        eng = GpuBruteForceEngine(D, "l2")
        if reserve:
            eng.reserve(reserve)
        eng.store_many_vectors(rows[:n])
        eng.build()
        return eng

    def searches(eng, count):
        return [_ms(lambda: eng.query_k_batch(queries, K)) for _ in range(count)]

    # destroy + add + build of the whole index: what a caller had to do for one more row
    eng = fresh(N)
    rebuild = []
    for _ in range(3):
        t = time.perf_counter()
        eng.close()
        eng = fresh(N)
        rebuild.append((time.perf_counter() - t) * 1e3)
    out["rebuild_ms"] = rebuild
    eng.close()
    # appends within a reserved capacity
    eng = fresh(N, reserve=N + extra)
    searches(eng, 3)
    steady0 = searches(eng, 5)
    n = N
    app, first = {}, {}
    for r in (1, 1000, 100_000):
        app[r] = _ms(lambda: eng.append(rows[n:n + r]))
        n += r
        first[r] = searches(eng, 1)[0]  # (the int8 filter's copy is made again inside this search)
        searches(eng, 2)
    out["append_ms"] = app
    out["first_search_ms"] = first
    out["steady_before_ms"] = steady0
    ids_a, d_a = eng.query_k_batch(queries, K)
    out["stats"] = {s: eng.get_stat(s) for s in ("append_extends", "append_rebuilds", "base_reallocs", "base_capacity_rows")}
    whole = fresh(n)
    searches(whole, 3)
    out["fresh_ms"], out["appended_ms"] = [], []
    for _ in range(9):  # (the two indexes in turn, so that neither has the quieter moment)
        out["fresh_ms"] += searches(whole, 1)
        out["appended_ms"] += searches(eng, 1)
    eng.close()
    ids_f, d_f = whole.query_k_batch(queries, K)
    out["same_answers"] = bool(np.array_equal(ids_a, ids_f) and np.array_equal(d_a.view(np.uint32), d_f.view(np.uint32)))
    whole.close()
    # without a reserve: the base and the fp16 copy are reallocated (x 1.5) and copied
    eng = fresh(N)
    out["append_1000_realloc_ms"] = _ms(lambda: eng.append(rows[N:N + 1000]))
    out["append_1000_after_ms"] = _ms(lambda: eng.append(rows[N + 1000:N + 2000]))
    out["stats_realloc"] = {s: eng.get_stat(s) for s in ("append_extends", "base_reallocs", "base_capacity_rows")}
    eng.close()
    print(json.dumps(out))


def _child(flag, env, limit):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), flag], check=True, capture_output=True, text=True,
                         env=env, timeout=limit)
    return json.loads(out.stdout.strip().splitlines()[-1])


def main(parent_dir, rounds):
    import torch
    print(f"# device: {torch.cuda.get_device_name(0)}")
    builds = (("parent", parent_dir), ("this", os.path.join(ROOT, "expann_amd")))
    envs = {name: dict(os.environ, EXPANN_LIB=os.path.join(d, "libexpann_hip.so")) for name, d in builds}
    step = {name: [] for name, _ in builds}
    print("# (a) C2's plain search: bench.py --gpus 1 --steps 60 --warmup 5")
    for r in range(rounds):
        for name, _ in builds:
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "5"],
                                 check=True, capture_output=True, text=True, env=envs[name], timeout=240)
            b = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')][-1])
            step[name].append(b["ms_per_step"])
            print(f"round {r} {name:6s}: {b['ms_per_step']:.4f} ms per step ({b['roofline']['kernel']})", flush=True)
    p, t = step["parent"], statistics.median(step["this"])
    print(f"bench ms per step: parent runs {p} (min {min(p)}, max {max(p)}, median {statistics.median(p)}); this build runs "
          f"{step['this']}, median {t} -> {'within' if min(p) <= t <= max(p) else ('BELOW (faster than)' if t < min(p) else 'ABOVE (slower than)')} "
          f"the parent's min-max spread")

    print(f"# (b) parent build: expann_build of {N} x d{D} fp32 rows")
    pb = _child("--parent-child", envs["parent"], 300)
    f16_ms = statistics.median(pb["build_ms"]) - statistics.median(pb["build_no_copy_ms"])
    print(f"build (upload + fp16 copy) {[round(x, 1) for x in pb['build_ms']]} ms; under scan_kernel 1 (upload only) "
          f"{[round(x, 1) for x in pb['build_no_copy_ms']]} ms -> ensure_f16 {f16_ms:.1f} ms = {f16_ms * 1e6 / N:.1f} ns per row")

    print(f"# (c) this build: {N} x d{D} fp32 rows, {MQ} queries, k = {K}; host-to-host wall times")
    c = _child("--this-child", envs["this"], 560)
    rebuild = statistics.median(c["rebuild_ms"])
    print(f"destroy + add + build of the whole: {[round(x, 1) for x in c['rebuild_ms']]} ms (median {rebuild:.1f})")
    for r, ms in c["append_ms"].items():
        print(f"append of {int(r):7d} rows within the reserved capacity: {ms:9.3f} ms = {ms * 1e6 / int(r):10.1f} ns per row "
              f"-> x {rebuild / ms:.0f} faster than the rebuild")
    print(f"append of    1000 rows without a reserve (base and fp16 copy grow x 1.5 and are copied): {c['append_1000_realloc_ms']:.3f} ms "
          f"-> x {rebuild / c['append_1000_realloc_ms']:.1f} faster than the rebuild; the next 1000 rows: {c['append_1000_after_ms']:.3f} ms; "
          f"{c['stats_realloc']}")
    print(f"THE CONDITION: the 1000-row append is faster than the rebuild: "
          f"{'yes' if c['append_ms']['1000'] < rebuild and c['append_1000_realloc_ms'] < rebuild else 'NO'} "
          f"(x {rebuild / c['append_ms']['1000']:.0f} reserved, x {rebuild / c['append_1000_realloc_ms']:.1f} with the reallocation)")
    print(f"statistics after the three appends: {c['stats']}")
    steady = statistics.median(c["steady_before_ms"])
    print(f"steady-state search before the appends: {[round(x, 2) for x in c['steady_before_ms']]} ms (median {steady:.2f})")
    for r, ms in c["first_search_ms"].items():
        print(f"first search after the append of {int(r):7d} rows (the int8 filter's copy is made again): {ms:.2f} ms "
              f"= steady + {ms - steady:.2f} ms")
    fa, ff = c["appended_ms"], c["fresh_ms"]
    print(f"search of the appended index {[round(x, 2) for x in fa]} ms (median {statistics.median(fa):.2f}); of a fresh index of "
          f"the same rows {[round(x, 2) for x in ff]} ms (median {statistics.median(ff):.2f}, min {min(ff):.2f}, max {max(ff):.2f}) -> "
          f"{'within' if min(ff) <= statistics.median(fa) <= max(ff) else ('BELOW (faster than)' if statistics.median(fa) < min(ff) else 'ABOVE (slower than)')} "
          f"the fresh index's min-max spread; "
          f"same ids and distance bits: {c['same_answers']}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="directory with the libexpann_hip.so of the build to compare with")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--this-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.parent_child:
        parent_child()
    elif a.this_child:
        this_child()
    else:
        main(os.path.abspath(a.parent_lib), a.rounds)
