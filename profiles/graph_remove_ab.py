"""What removing rows from a built graph engine costs and what it does to recall (AntitopoEngine.remove; DESIGN.md
4.9l), on one MI355X, against the only route the parent commit has -- a new engine, store_many_vectors_batched of the
survivors + build() -- and that an engine which never removes walks as fast as the parent commit's.

    python profiles/graph_remove_ab.py --parent-tree DIR [--parts time,recall,bench] [--rounds 5] > profiles/graph_remove_ab.txt

DIR is a built checkout of the parent commit (its own libexpann_hip.so), needed by `bench` alone.  Every part runs in
processes of its own, one at a time, each under a time limit; the first that fails ends the run.
  time    the C4 graph -- 1 M x d128 SIFT-like rows, M = 60, ef_construction = 480, built by the batched builder: the
          handle's first remove (1 row: the one-time upload of the builder's state), then removes of 1 / 1 000 /
          100 000 random rows, host-to-host, with "remove_repair_ns", the table remake ("append_tables_ns") and the
          host's compaction of its vectors (timed on a copy, the same loop) reported apart; and the rebuild of the
          survivors in a new engine.
  recall  recall@10 at ef_search = 60 of 1 000 queries and the time of that search at 1 % / 10 % / 50 % removed: the
          repaired graph, the fresh rebuild of the survivors, and the old graph under a tombstone row filter.
  bench   `bench.py --workload c4` (each run builds its own graph): the parent's tree and this one in turn, the order
          swapped every round; this build's median is compared with the smallest and the largest of the parent's runs."""
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
N, D, M, EFC, EFS = 1_000_000, 128, 60, 480, 60
BLOCKS = (1, 1000, 100_000)
FRACTIONS = (0.01, 0.10, 0.50)


def _data(n=N):
    rng = np.random.default_rng(4)
    x = rng.standard_normal((n, D), dtype=np.float32)
    return np.clip(np.round(np.abs(x) * 40.0), 0, 255).astype(np.float32)


def _ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def _built(rows):
    from expann_amd import AntitopoEngine
    eng = AntitopoEngine(M, EFC, 1, 0, False, dim=D)
    ms = _ms(lambda: eng.store_many_vectors_batched(rows))
    return eng, ms, _ms(eng.build)


def _host_compaction_ms(rows, keep):
    """the engine's loop over its own copy of the vectors: survivors moved down in order"""
    a = rows.copy()
    idx = np.nonzero(keep)[0]
    return _ms(lambda: a.__setitem__(slice(0, len(idx)), a[idx]))


def time_child():
    rows = _data()
    rng = np.random.default_rng(5)
    out = {}
    eng, out["store_ms"], out["build_ms"] = _built(rows)
    q = rows[:1000] + 0.5
    eng.set_ef_search(EFS)
    eng.query_many(q, 10)
    out["first_remove_ms"] = _ms(lambda: eng.remove(rng.choice(eng.size(), 1)))  # the one-time upload of the builder's state
    out["remove_ms"], out["repair_ns"], out["tables_ns"], out["touched"], out["truncated"], out["host_compact_ms"] = {}, {}, {}, {}, {}, {}
    for r in (1,) + BLOCKS:  # (one more single row first: the first steady-state remove)
        n = eng.size()
        ids = rng.choice(n, r, replace=False).astype(np.uint64)
        t0, c0 = eng.stat("remove_touched_rows"), eng.stat("remove_truncated_rows")
        out["remove_ms"].setdefault(str(r), []).append(_ms(lambda: eng.remove(ids)))
        out["repair_ns"][str(r)] = eng.stat("remove_repair_ns")
        out["tables_ns"][str(r)] = eng.stat("append_tables_ns")
        out["touched"][str(r)] = eng.stat("remove_touched_rows") - t0
        out["truncated"][str(r)] = eng.stat("remove_truncated_rows") - c0
        keep = np.ones(n, bool)
        keep[ids.astype(np.int64)] = False
        out["host_compact_ms"][str(r)] = _host_compaction_ms(rows[:n], keep)
    out["search_after_ms"] = [_ms(lambda: eng.query_many(q, 10)) for _ in range(3)]
    out["stats"] = {s: eng.stat(s) for s in ("remove_calls", "remove_rows", "remove_device", "remove_host", "capacity_rows")}
    out["rows"] = eng.size()
    eng.close()
    # the parent's only route: a new engine over the survivors (the same count; which rows does not matter for the time)
    out["rebuild_ms"] = {}
    for r in BLOCKS:
        eng, s, b = _built(rows[:N - r])
        out["rebuild_ms"][str(r)] = s + b
        eng.close()
    print(json.dumps(out))


def _recall(ids, truth):
    return float(np.mean([len(set(ids[i].tolist()) & set(truth[i].tolist())) / 10.0 for i in range(len(ids))]))


def recall_child(frac):
    from expann_amd import GpuBruteForceEngine
    rows = _data()
    rng = np.random.default_rng(6)
    q = rows[rng.choice(N, 1000, replace=False)] + rng.uniform(0, 0.99, (1000, D)).astype(np.float32)
    gone = rng.choice(N, int(N * frac), replace=False)
    keep = np.ones(N, bool)
    keep[gone] = False
    survivors = np.ascontiguousarray(rows[keep])
    bf = GpuBruteForceEngine(D)
    bf.store_many_vectors(survivors)
    bf.build()
    truth, _ = bf.query_k_batch(q, 10)
    bf.close()
    old_id = np.nonzero(keep)[0]
    out = {"frac": frac}
    eng, _, _ = _built(rows)
    eng.set_ef_search(EFS)
    eng.set_row_filter(keep)  # tombstones: the old graph under a row filter
    ids, _ = eng.query_many(q, 10)
    out["filter_ms"] = min(_ms(lambda: eng.query_many(q, 10)) for _ in range(3))
    new_of_old = np.full(N, -1, np.int64)
    new_of_old[old_id] = np.arange(len(old_id))
    mapped = np.where(ids == np.uint64(2 ** 64 - 1), -1, new_of_old[np.minimum(ids, N - 1).astype(np.int64)])
    out["filter_recall"] = _recall(mapped, truth)
    eng.set_row_filter(None)
    out["remove_ms"] = _ms(lambda: eng.remove(gone))
    out["repair_ns"] = eng.stat("remove_repair_ns")
    out["touched"], out["truncated"] = eng.stat("remove_touched_rows"), eng.stat("remove_truncated_rows")
    ids, _ = eng.query_many(q, 10)
    out["repaired_ms"] = min(_ms(lambda: eng.query_many(q, 10)) for _ in range(3))
    out["repaired_recall"] = _recall(ids, truth)
    eng.close()
    eng, s, b = _built(survivors)
    out["rebuild_ms"] = s + b
    eng.set_ef_search(EFS)
    ids, _ = eng.query_many(q, 10)
    out["fresh_ms"] = min(_ms(lambda: eng.query_many(q, 10)) for _ in range(3))
    out["fresh_recall"] = _recall(ids, truth)
    eng.close()
    print(json.dumps(out))


def _child(args, env, limit):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, check=True, capture_output=True, text=True,
                         env=env, timeout=limit)
    return json.loads(out.stdout.strip().splitlines()[-1])


def part_time():
    print(f"# time: {N} x d{D} SIFT-like rows, M = {M}, ef_construction = {EFC}; host-to-host wall times")
    c = _child(["--time-child"], dict(os.environ), 1100)
    print(f"store_many_vectors_batched of the {N} rows {c['store_ms'] / 1e3:.1f} s, build() {c['build_ms'] / 1e3:.2f} s")
    print(f"the handle's FIRST remove (1 row; to_strided of the host graph and the one-time upload of the builder's state): "
          f"{c['first_remove_ms']:.1f} ms")
    for r in BLOCKS:
        k = str(r)
        for ms in c["remove_ms"][k]:
            print(f"remove of {r:7d} rows: {ms:10.2f} ms | a new engine over the survivors, store_many_vectors_batched + build(): "
                  f"{c['rebuild_ms'][k]:10.1f} ms -> x {c['rebuild_ms'][k] / ms:.1f}")
        print(f"    of which on the device: touch + gather + prune {c['repair_ns'][k] / 1e6:.3f} ms ({c['touched'][k]} touched rows, "
              f"{c['truncated'][k]} truncated), table remake {c['tables_ns'][k] / 1e6:.3f} ms; the host's compaction of its vectors "
              f"(the same move, timed on a copy) {c['host_compact_ms'][k]:.1f} ms")
    print(f"search of 1000 queries after the removes: {[round(x, 2) for x in c['search_after_ms']]} ms")
    print(f"statistics: {c['stats']}, rows left {c['rows']}")


def part_recall():
    print(f"# recall: recall@10 of 1000 queries at ef_search = {EFS} against the exact top-10 over the survivors, and the time of that search")
    for frac in FRACTIONS:
        c = _child(["--recall-child", str(frac)], dict(os.environ), 1100)
        print(f"{frac * 100:4.0f} % removed: repaired {c['repaired_recall']:.4f} in {c['repaired_ms']:.2f} ms | fresh rebuild "
              f"{c['fresh_recall']:.4f} in {c['fresh_ms']:.2f} ms (rebuilt in {c['rebuild_ms'] / 1e3:.1f} s) | old graph under a tombstone "
              f"filter {c['filter_recall']:.4f} in {c['filter_ms']:.2f} ms | the remove took {c['remove_ms']:.0f} ms (first on its handle: "
              f"with the one-time upload), repair {c['repair_ns'] / 1e6:.1f} ms on the device, {c['touched']} touched rows, "
              f"{c['truncated']} truncated", flush=True)


def part_bench(parent_tree, rounds):
    print("# bench: python bench.py --workload c4")
    trees = (("parent", parent_tree), ("this", ROOT))
    qps = {name: [] for name, _ in trees}
    for r in range(rounds):
        for name, tree in (trees if r % 2 == 0 else trees[::-1]):  # (neither build always runs behind the other)
            out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--workload", "c4"], check=True,
                                 capture_output=True, text=True, cwd=tree, timeout=400)
            b = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')][-1])
            qps[name].append(b["value"])
            print(f"round {r} {name:6s}: {b['value']:.1f} queries/s, kernel {b['roofline']['kernel_ms']} ms, recall "
                  f"{b['config']['recall']}, build {b['config']['build_s']} s", flush=True)
    p, t = qps["parent"], statistics.median(qps["this"])
    verdict = "within" if min(p) <= t <= max(p) else ("ABOVE (faster than)" if t > max(p) else "BELOW (slower than)")
    print(f"bench queries/s: parent runs {p} (min {min(p)}, max {max(p)}, median {statistics.median(p)}); this build runs "
          f"{qps['this']}, median {t} -> {verdict} the parent's min-max spread")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the commit to compare with (bench)")
    ap.add_argument("--parts", default="time,recall,bench")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--time-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--recall-child", type=float, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.time_child:
        time_child()
    elif a.recall_child is not None:
        recall_child(a.recall_child)
    else:
        import torch
        print(f"# device: {torch.cuda.get_device_name(0)}", flush=True)
        for part in a.parts.split(","):
            if part == "time":
                part_time()
            elif part == "recall":
                part_recall()
            elif part == "bench":
                part_bench(os.path.abspath(a.parent_tree), a.rounds)
