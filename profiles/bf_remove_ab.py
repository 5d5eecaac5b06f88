"""What removing rows from a built brute-force index costs (expann_remove), on one MI355X, and that an
index which never removes searches as fast as the parent commit's.

    python profiles/bf_remove_ab.py --parent-lib DIR [--rounds 3] > profiles/bf_remove_ab.txt

DIR holds the other build's libexpann_hip.so (the parent commit's).  Every part runs in processes of its own, one at
a time, each under a time limit; the first that fails ends the run.
  (a) C2's plain search, `bench.py --gpus 1 --steps 60 --warmup 5`: per round the other build first and then this one,
      so the two alternate; this build's median is compared with the smallest and the largest of the other build's
      runs.  The one pass/fail number.
  (b) this build, 1 M x d128 fp32 rows, 10 000 queries, k = 10, host-to-host wall times, the arms in turn: removing
      1 / 1 000 / 100 000 / 500 000 random rows against destroy + add + build of the same survivors; the first search
      after a remove against steady-state searches; searches of the index after the remove against searches of a fresh
      index of the same rows; a search under a 50 % row filter against the search after compact_row_filter of the
      same filter.
  (c) the device time of the launches of one remove of 1 000 rows (rocprofv3 --kernel-trace --stats, a run of its
      own): the bytes each compaction launch reads and writes over its time, against the HBM peak."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, D, MQ, K = 1_000_000, 128, 10_000, 10
HBM_PEAK_TBS = 8.0  # MI355X: 8 TB/s by the specification; a plain 16-byte-per-lane copy reaches about 6.3


def _data():
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((N, D), dtype=np.float32)
    top = int(np.argmax(np.abs(rows).max(axis=1)))
    rows[[0, top]] = rows[[top, 0]]  # (max |v| in row 0, which stays: the removes compact the fp16 copy)
    return rows, rng.standard_normal((MQ, D), dtype=np.float32)


def _ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def _ids(r, seed):
    return (np.random.default_rng(seed).choice(N - 1, r, replace=False) + 1).astype(np.uint64)  # (never row 0)


def this_child():
    """(b) in this process; prints one JSON line"""
    from expann_amd import GpuBruteForceEngine
    rows, queries = _data()
    out = {"remove_ms": {}, "rebuild_ms": {}, "first_search_ms": {}, "stats": {}}

    def fresh(r):
        eng = GpuBruteForceEngine(D, "l2")
        eng.store_many_vectors(r)
        eng.build()
        return eng

    def searches(eng, count):
        return [_ms(lambda: eng.query_k_batch(queries, K)) for _ in range(count)]

    eng = fresh(rows)
    searches(eng, 3)
    out["steady_ms"] = searches(eng, 5)
    eng.close()
    for r in (1, 1000, 100_000, 500_000):
        rm, rb, first = [], [], []
        for rep in range(3):  # the two arms in turn
            ids = _ids(r, 100 * rep + 7)
            keep = np.ones(N, dtype=bool)
            keep[ids.astype(np.int64)] = False
            eng = fresh(rows)
            searches(eng, 2)
            rm.append(_ms(lambda: eng.remove(ids)))
            first.append(searches(eng, 1)[0])  # (the int8 filter's copy is made again inside this search)
            t = time.perf_counter()
            eng.close()
            surv = rows[keep]  # (gathering the survivors on the host is part of what the caller had to do)
            eng = fresh(surv)
            rb.append((time.perf_counter() - t) * 1e3)
            eng.close()
        out["remove_ms"][r], out["rebuild_ms"][r], out["first_search_ms"][r] = rm, rb, first
    # the index after a remove against a fresh one of the same rows
    ids = _ids(100_000, 7)
    keep = np.ones(N, dtype=bool)
    keep[ids.astype(np.int64)] = False
    eng = fresh(rows)
    eng.remove(ids)
    out["stats"] = {s: eng.get_stat(s) for s in ("remove_calls", "remove_rows", "remove_compacts", "remove_rebuilds",
                                                 "base_reallocs", "base_capacity_rows")}
    whole = fresh(rows[keep])
    searches(eng, 3)
    searches(whole, 3)
    out["fresh_ms"], out["removed_ms"] = [], []
    for _ in range(9):
        out["fresh_ms"] += searches(whole, 1)
        out["removed_ms"] += searches(eng, 1)
    a, b = eng.query_k_batch(queries, K), whole.query_k_batch(queries, K)
    out["same_answers"] = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))
    out["same_digest"] = eng.get_stat("copies_digest") == whole.get_stat("copies_digest") != 0
    eng.close()
    whole.close()
    # tombstones against compaction: a 50 % filter
    allow = np.random.default_rng(5).random(N) < 0.5
    allow[0] = True
    tomb, comp = fresh(rows), fresh(rows)
    tomb.set_row_filter(allow)
    comp.set_row_filter(allow)
    out["compact_filter_ms"] = _ms(comp.compact_row_filter)
    searches(tomb, 3)
    searches(comp, 3)
    out["tombstone_ms"], out["compacted_ms"] = [], []
    for _ in range(9):
        out["tombstone_ms"] += searches(tomb, 1)
        out["compacted_ms"] += searches(comp, 1)
    tomb.close()
    comp.close()
    print(json.dumps(out))


def trace_child():
    """(c): one remove of 1 000 rows, to be run under the profiler"""
    from expann_amd import GpuBruteForceEngine
    rows, queries = _data()
    eng = GpuBruteForceEngine(D, "l2")
    eng.store_many_vectors(rows)
    eng.build()
    eng.query_k_batch(queries[:256], K)
    eng.remove(_ids(1000, 7))
    eng.close()


def _run(cmd, env, limit):
    """one step in a process of its own, under its time limit; a step that fails ends the run and says why"""
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=limit)
    if out.returncode != 0:
        sys.exit(f"{' '.join(cmd)}: exit status {out.returncode}\n{out.stderr[-4000:]}")
    return out.stdout


def _child(flag, env, limit):
    return json.loads(_run([sys.executable, os.path.abspath(__file__), flag], env, limit).strip().splitlines()[-1])


def _spread(v):
    return f"{[round(x, 2) for x in v]} ms (median {statistics.median(v):.2f}, min {min(v):.2f}, max {max(v):.2f})"


def _where(x, ref):
    return "within" if min(ref) <= x <= max(ref) else ("BELOW (faster than)" if x < min(ref) else "ABOVE (slower than)")


def main(parent_dir, rounds, skip_bench):
    import torch
    print(f"# device: {torch.cuda.get_device_name(0)}")
    builds = (("parent", parent_dir), ("this", os.path.join(ROOT, "expann_amd")))
    envs = {name: dict(os.environ, EXPANN_LIB=os.path.join(d, "libexpann_hip.so")) for name, d in builds}
    if not skip_bench:
        step = {name: [] for name, _ in builds}
        print("# (a) C2's plain search: bench.py --gpus 1 --steps 60 --warmup 5")
        for r in range(rounds):
            for name, _ in builds:
                out = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "5"],
                           envs[name], 240)
                b = json.loads([ln for ln in out.splitlines() if ln.startswith('{"metric"')][-1])
                step[name].append(b["ms_per_step"])
                print(f"round {r} {name:6s}: {b['ms_per_step']:.4f} ms per step ({b['roofline']['kernel']})", flush=True)
        p, t = step["parent"], statistics.median(step["this"])
        print(f"bench ms per step: parent runs {p} (min {min(p)}, max {max(p)}, median {statistics.median(p)}); this build runs "
              f"{step['this']}, median {t} -> {_where(t, p)} the parent's min-max spread", flush=True)

    print(f"# (b) this build: {N} x d{D} fp32 rows, {MQ} queries, k = {K}; host-to-host wall times, three repetitions, the arms in turn")
    c = _child("--this-child", envs["this"], 900)
    steady = statistics.median(c["steady_ms"])
    for r in c["remove_ms"]:
        rm, rb = c["remove_ms"][r], c["rebuild_ms"][r]
        ratio = statistics.median(rb) / statistics.median(rm)
        print(f"remove of {int(r):7d} random rows: {_spread(rm)}; destroy + gather + add + build of the survivors: {_spread(rb)} "
              f"-> the remove is x {ratio:.1f} faster")
    r1000 = statistics.median(c["rebuild_ms"]["1000"]) / statistics.median(c["remove_ms"]["1000"])
    print(f"THE CONDITION: the 1000-row remove is clearly faster than the rebuild: {'yes' if r1000 > 2 else 'NO'} (x {r1000:.1f})")
    print(f"steady-state search before a remove: {_spread(c['steady_ms'])}")
    for r, v in c["first_search_ms"].items():
        print(f"first search after the remove of {int(r):7d} rows (the int8 filter's copy is made again): {_spread(v)} "
              f"= steady + {statistics.median(v) - steady:.2f} ms")
    fa, ff = c["removed_ms"], c["fresh_ms"]
    print(f"search of the index after removing 100000 rows: {_spread(fa)}; of a fresh index of the same rows: {_spread(ff)} -> "
          f"{_where(statistics.median(fa), ff)} the fresh index's min-max spread; same ids and distance bits: {c['same_answers']}; "
          f"same copies_digest: {c['same_digest']}; {c['stats']}")
    tm, cm = c["tombstone_ms"], c["compacted_ms"]
    print(f"search under a 50 % row filter (tombstones): {_spread(tm)}; after compact_row_filter of the same filter "
          f"({c['compact_filter_ms']:.2f} ms, once): {_spread(cm)} -> the compacted index searches x "
          f"{statistics.median(tm) / statistics.median(cm):.2f} faster")

    print("# (c) device time of one remove of 1000 rows from the same index (rocprofv3 --kernel-trace --stats, a run of its own)")
    with tempfile.TemporaryDirectory() as tmp:
        _run(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "remove", "--output-format", "csv", "--",
              sys.executable, os.path.abspath(__file__), "--trace-child"], envs["this"], 400)
        files = [f for f in glob.glob(os.path.join(tmp, "**", "*.csv"), recursive=True) if "kernel_trace" in os.path.basename(f)]
        dur = {}
        for f in files:
            for row in csv.DictReader(open(f)):
                name = row.get("Kernel_Name", "")
                for key in ("compact_rows_kernel", "survivor_maxima_kernel", "remove_mark_kernel", "remove_word_rank_kernel",
                            "filter_count_kernel"):
                    if key in name:
                        dur.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    survivors = N - 1000
    moved = {"base rows": 2 * survivors * D * 4, "fp16 rows and terms": 2 * survivors * (D * 2 + 8)}
    for (what, nbytes), us in zip(moved.items(), dur.get("compact_rows_kernel", [])):
        tbs = nbytes / (us * 1e-6) / 1e12
        print(f"compact_rows_kernel, {what}: {us:.1f} us for {nbytes / 1e6:.0f} MB read + written = {tbs:.2f} TB/s "
              f"= {100 * tbs / HBM_PEAK_TBS:.0f} % of the {HBM_PEAK_TBS:.0f} TB/s HBM peak (a plain wide copy reaches about 6.3 TB/s)")
    for key in ("survivor_maxima_kernel", "remove_mark_kernel", "filter_count_kernel", "remove_word_rank_kernel"):
        for us in dur.get(key, []):
            extra = f" ({survivors * D * 4 / (us * 1e-6) / 1e12:.2f} TB/s read, 4 bytes per lane)" if key == "survivor_maxima_kernel" else ""
            print(f"{key}: {us:.1f} us{extra}")
    if not dur:
        print("no kernel of the remove found in the trace")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="directory with the libexpann_hip.so of the build to compare with")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-bench", action="store_true", help="leave part (a) out")
    ap.add_argument("--this-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.this_child:
        this_child()
    elif a.trace_child:
        trace_child()
    else:
        main(os.path.abspath(a.parent_lib) if a.parent_lib else os.path.join(ROOT, "expann_amd"), a.rounds, a.skip_bench)
