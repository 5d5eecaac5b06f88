"""What an append to a built graph engine costs (AntitopoEngine.append), on one MI355X, against the
route every engine took before -- store_many_vectors_batched + build() -- and that an engine which is never appended
to walks as fast as the parent commit's.

    python profiles/graph_append_ab.py --parent-tree DIR [--parts append,bench] [--rounds 5] > profiles/graph_append_ab.txt

DIR is a built checkout of the parent commit (its own libexpann_hip.so and expann_graph_tool).  Every part runs in
processes of its own, one at a time, each under a time limit; the first that fails ends the run.
  append  the C4 graph -- 1 M x d128 SIFT-like rows, M = 60, ef_construction = 480, built by the batched builder --
          in this build: reserve, the handle's first append (the one-time upload of the builder's state), appends of
          1 / 1 000 / 100 000 rows within the reserved capacity, the device time of the table-rebuild kernels, and what
          the next save costs (the download and from_strided); then the same graph under the PARENT's library, where
          the same rows go through store_many_vectors_batched + build().  Host-to-host wall times.
  bench   `bench.py --workload c4` (each run builds its own graph): the parent's tree and this one in turn, the order
          swapped every round; this build's median is compared with the smallest and the largest of the parent's runs."""
import argparse
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
N, D, M, EFC = 1_000_000, 128, 60, 480
BLOCKS = (1, 1000, 100_000)
HBM_PEAK_GBS = 8000.0  # MI355X


def _data():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((N + 2 + sum(BLOCKS), D), dtype=np.float32)
    return np.clip(np.round(np.abs(x) * 40.0), 0, 255).astype(np.float32)


def _ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def _built(rows):
    from expann_amd import AntitopoEngine
    eng = AntitopoEngine(M, EFC, 1, 0, False, dim=D)
    ms = _ms(lambda: eng.store_many_vectors_batched(rows[:N]))
    return eng, ms, _ms(eng.build)


def this_child():
    rows = _data()
    out = {}
    eng, out["store_ms"], out["build_ms"] = _built(rows)
    q = rows[:1000] + 0.5
    eng.set_ef_search(60)
    eng.query_many(q, 10)
    out["reserve_ms"] = _ms(lambda: eng.reserve(N + 2 + sum(BLOCKS)))
    n = N
    out["first_append_ms"] = _ms(lambda: eng.append(rows[n:n + 1]))  # the one-time upload of the builder's state
    n += 1
    out["append_ms"], out["tables_ns"], out["batches"] = {}, {}, {}
    for r in (1,) + BLOCKS:  # (one more single row first: the first steady-state append)
        b0 = eng.stat("append_batches")
        ms = _ms(lambda: eng.append(rows[n:n + r]))
        n += r
        out["append_ms"].setdefault(str(r), []).append(ms)
        out["tables_ns"][str(r)] = eng.stat("append_tables_ns")
        out["batches"][str(r)] = eng.stat("append_batches") - b0
    out["search_after_ms"] = [_ms(lambda: eng.query_many(q, 10)) for _ in range(3)]
    out["stats"] = {s: eng.stat(s) for s in ("append_calls", "append_rows", "append_device", "append_host", "graph_reallocs",
                                             "capacity_rows", "append_edges")}
    out["rows"] = n
    with tempfile.TemporaryDirectory() as tmp:
        out["save_stale_ms"] = _ms(lambda: eng.save_index(os.path.join(tmp, "a.index")))  # download + from_strided + write
        out["save_again_ms"] = _ms(lambda: eng.save_index(os.path.join(tmp, "b.index")))  # write only
    eng.close()
    print(json.dumps(out))


def parent_child():
    """the same rows through store_many_vectors_batched + build() with whichever library EXPANN_LIB names"""
    rows = _data()
    out = {}
    eng, out["store_ms"], out["build_ms"] = _built(rows)
    n = N
    out["route_ms"] = {}
    for r in (1,) + BLOCKS:
        def route():
            eng.store_many_vectors_batched(rows[n:n + r])
            eng.build()
        out["route_ms"].setdefault(str(r), []).append(_ms(route))
        n += r
    eng.close()
    print(json.dumps(out))


def _child(flag, env, limit):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), flag], check=True, capture_output=True, text=True,
                         env=env, timeout=limit)
    return json.loads(out.stdout.strip().splitlines()[-1])


def part_append(parent_tree):
    print(f"# append: {N} x d{D} SIFT-like rows, M = {M}, ef_construction = {EFC}; host-to-host wall times")
    c = _child("--this-child", dict(os.environ), 900)
    print(f"this build: store_many_vectors_batched of the {N} rows {c['store_ms'] / 1e3:.1f} s, build() {c['build_ms'] / 1e3:.2f} s")
    print(f"reserve({N + 2 + sum(BLOCKS)}): {c['reserve_ms']:.1f} ms")
    print(f"the handle's FIRST append (1 row; to_strided of the host graph and the one-time upload of the builder's state): "
          f"{c['first_append_ms']:.1f} ms")
    p = _child("--parent-child", dict(os.environ, EXPANN_LIB=os.path.join(parent_tree, "expann_amd", "libexpann_hip.so")), 900)
    print(f"parent's library: store_many_vectors_batched of the {N} rows {p['store_ms'] / 1e3:.1f} s, build() {p['build_ms'] / 1e3:.2f} s")
    for r in BLOCKS:  # (two single-row appends: the first steady-state one, then another)
        for i, ms in enumerate(c["append_ms"][str(r)]):
            route = p["route_ms"][str(r)][i]
            print(f"append of {r:7d} rows within the reserved capacity: {ms:10.2f} ms ({c['batches'][str(r)]} batches) | the parent's "
                  f"route, store_many_vectors_batched + build(): {route:10.1f} ms -> x {route / ms:.1f}")
    e = c["stats"]["append_edges"]
    n = c["rows"]
    stride_adj = (2 * M + 3) // 4 * 4
    # bytes the rebuild kernels move, counted from the algorithm: the layer-0 table (degrees and ids read, rows written),
    # the degree pass (written once), the scan (read twice, written once), the fill (offsets read, ids read and written)
    for r in map(str, BLOCKS):
        ns = c["tables_ns"][r]
        lo = 4 * n + 4 * e + 4 * n * stride_adj + 8 * e
        print(f"table rebuild after the append of {int(r):7d} rows: {ns / 1e6:.3f} ms on the device; at least {lo / 1e9:.3f} GB moved "
              f"(layer-0 table and edges alone, the final sizes) -> {lo / ns:.1f} GB/s = {lo / ns / HBM_PEAK_GBS * 100:.1f} % of the HBM peak")
    print(f"search of 1000 queries after the appends: {[round(x, 2) for x in c['search_after_ms']]} ms")
    print(f"save after the appends: {c['save_stale_ms'] / 1e3:.2f} s (download, from_strided, write); the same save again "
          f"{c['save_again_ms'] / 1e3:.2f} s (write only) -> the refresh costs {(c['save_stale_ms'] - c['save_again_ms']) / 1e3:.2f} s")
    print(f"statistics: {c['stats']}")


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
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the commit to compare with")
    ap.add_argument("--parts", default="append,bench")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--this-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.parent_child:
        parent_child()
    elif a.this_child:
        this_child()
    else:
        import torch
        print(f"# device: {torch.cuda.get_device_name(0)}", flush=True)
        for part in a.parts.split(","):
            if part == "append":
                part_append(os.path.abspath(a.parent_tree))
            elif part == "bench":
                part_bench(os.path.abspath(a.parent_tree), a.rounds)
