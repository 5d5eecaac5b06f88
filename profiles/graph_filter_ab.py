"""The graph engine's row filter, measured on the C4 graph (1 M x d128 SIFT-like rows, M = 60, ef_construction = 480,
batched build; 10 k queries, k = 10, ef_search = 60) on one MI355X.

    python profiles/graph_filter_ab.py --parent-lib /path/to/parent/libexpann_hip.so > profiles/graph_filter_ab.txt

  1. the UNFILTERED walk's kernel time in this build and in the parent build (EXPANN_LIB selects the library; one
     process per run, the two builds interleaved): this build's median must lie inside the parent's own min .. max,
     or filtered code has leaked into the unfiltered instances;
  2. the FILTERED walk ("filter_flat_rows" = 1) at allowed shares 100 / 50 / 10 / 1 / 0.1 % of random rows (fixed
     seed): kernel ms, queries the redo launch served, final overflows, and recall@10 against the exact answer of the
     brute-force index under the same filter (expann_set_row_filter: an independent ground truth);
  3. the SCAN against the walk at allowed counts doubling from 1 k, until the walk is faster: the automatic value of
     "filter_flat_rows" is the largest count at which the scan still beats the walk or the walk still overflows.
Medians of --repeats runs with their min .. max."""
import argparse
import ctypes as C
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
sys.path.insert(0, os.path.join(ROOT, "profiles"))
N, D, M_Q, K, EF, GRAPH_M, EFC = 1_000_000, 128, 10_000, 10, 60, 60, 480


def med(x):
    return f"{statistics.median(x):8.3f} [{min(x):8.3f} .. {max(x):8.3f}]"


def build(tmp, rows):
    """the graph through the batched builder; base, queries and the CSR form of the index go to one .npz"""
    from expann_amd import AntitopoEngine
    from graph_device_latency import read_index_csr, sift_like
    rng = np.random.RandomState(7)
    base = sift_like(rng, rows, D)
    q = sift_like(rng, M_Q, D, frac=True)
    t0 = time.perf_counter()
    eng = AntitopoEngine(GRAPH_M, EFC, 1, 0, False, dim=D)
    eng.store_many_vectors_batched(base, False)
    eng.build()
    idx = os.path.join(tmp, "c4.index")
    eng.save_index(idx)
    eng.close()
    t1 = time.perf_counter()
    sv, n_layers, off, nb = read_index_csr(idx)
    os.remove(idx)
    path = os.path.join(tmp, "c4.npz")
    np.savez(path, base=base, q=q, sv=sv, n_layers=n_layers, off=off, nb=nb)
    print(f"# graph: {rows} x d{D} SIFT-like rows, batched builder, M = {GRAPH_M}, ef_construction = {EFC}, {n_layers} "
          f"layers, built in {t1 - t0:.1f} s; {M_Q} queries, k = {K}, ef_search = {EF}", flush=True)
    return path


def open_graph(path):
    from expann_amd import _lib
    L = _lib.load()
    z = np.load(path)
    base, q = np.ascontiguousarray(z["base"]), np.ascontiguousarray(z["q"])
    off, nb = np.ascontiguousarray(z["off"]), np.ascontiguousarray(z["nb"])  # (held: the call reads them)
    assert off.dtype == np.uint64 and nb.dtype == np.uint32
    h = C.c_void_p()
    rc = L.expann_graph_create(D, 0, base.ctypes.data, base.shape[0], int(z["n_layers"]), int(z["sv"]),
                               off.ctypes.data, nb.ctypes.data, C.byref(h))
    assert rc == 0, L.expann_graph_last_error(None)
    return L, h, base, q


class Searcher:
    def __init__(self, L, h, q):
        import torch
        self.L, self.h, self.torch = L, h, torch
        self.tq = torch.from_numpy(q).cuda()
        self.ids = torch.zeros((q.shape[0], K), dtype=torch.int64, device="cuda")
        self.dists = torch.zeros((q.shape[0], K), dtype=torch.float32, device="cuda")
        self.st = torch.cuda.Stream()
        torch.cuda.synchronize()

    def stat(self, name):
        out = C.c_uint64()
        assert self.L.expann_graph_get_stat(self.h, name, C.byref(out)) == 0
        return out.value

    def run(self):
        """one device-buffer search and its sync: (kernel ms, redo queries, overflowed)"""
        L, h = self.L, self.h
        rc = L.expann_graph_search_device(h, self.tq.data_ptr(), self.tq.shape[0], K, EF, 0, self.ids.data_ptr(),
                                          self.dists.data_ptr(), None, self.st.cuda_stream)
        assert rc == 0, L.expann_graph_last_error(h)
        rc = L.expann_graph_sync(h)
        assert rc in (0, 6), L.expann_graph_last_error(h)
        return L.expann_graph_last_kernel_ms(h), self.stat(b"redo_queries"), rc == 6

    def timed(self, repeats):
        self.run()  # warm
        runs = [self.run() for _ in range(repeats)]
        return [r[0] for r in runs], runs[-1][1], sum(r[2] for r in runs)


def worker_unfiltered(path, repeats):
    L, h, base, q = open_graph(path)
    ms, _, _ = Searcher(L, h, q).timed(repeats)
    print(json.dumps({"kernel_ms": ms}))
    L.expann_graph_destroy(h)


def worker_filtered(path, repeats):
    from expann_amd import GpuBruteForceEngine, pack_row_filter
    L, h, base, q = open_graph(path)
    n = base.shape[0]
    s = Searcher(L, h, q)
    bf = GpuBruteForceEngine(D, "l2")
    bf.store_many_vectors(base)
    bf.build()

    def set_filter(allow, flat_rows):
        words = pack_row_filter(allow)
        assert L.expann_graph_set_option(h, b"filter_flat_rows", flat_rows) == 0
        assert L.expann_graph_set_row_filter(h, words.ctypes.data, words.size) == 0, L.expann_graph_last_error(h)
        bf.set_row_filter(allow)

    def recall():
        truth, _ = bf.query_k_batch(q, K)
        got = s.ids.cpu().numpy().view(np.uint64)
        hit = sum(len(set(t[t != np.uint64(2 ** 64 - 1)].tolist()) & set(g.tolist())) for t, g in zip(truth, got))
        return hit / float((truth != np.uint64(2 ** 64 - 1)).sum())

    unf, _, _ = s.timed(repeats)
    truth_unf, _ = bf.query_k_batch(q, K)
    print(f"\n# 2. filtered walk (\"filter_flat_rows\" = 1), random rows, seed 11; kernel ms: median [min .. max] of "
          f"{repeats} runs\nunfiltered            : {med(unf)}", flush=True)
    print("share    allowed rows | kernel ms                        | redo queries | overflowed searches | recall@10")
    rng = np.random.RandomState(11)
    u = rng.rand(n)
    for share in (1.0, 0.5, 0.1, 0.01, 0.001):
        allow = u < share
        set_filter(allow, 1)
        ms, redo, over = s.timed(repeats)
        print(f"{100 * share:6.1f} % {int(allow.sum()):12d} | {med(ms)} | {redo:12d} | {over:3d} of {repeats:3d}          | "
              f"{recall():.4f}" + (f"   (x {statistics.median(ms) / statistics.median(unf):.3f} of unfiltered)"
                                   if share == 1.0 else ""), flush=True)
    print("\n# 3. scan (\"filter_flat_rows\" = the count) against walk (\"filter_flat_rows\" = 1) at the same random filter")
    print("allowed rows | scan kernel ms                   | walk kernel ms                   | walk redo queries | walk "
          "overflowed | scan recall | walk recall")
    count, chosen = 1000, 0
    order = rng.permutation(n)
    while count <= n:
        allow = np.zeros(n, bool)
        allow[order[:count]] = True
        set_filter(allow, count)
        flat = s.stat(b"flat_searches")
        scan_ms, _, _ = s.timed(repeats)
        assert s.stat(b"flat_searches") == flat + repeats + 1
        r_scan = recall()
        set_filter(allow, 1)
        walk_ms, redo, over = s.timed(repeats)
        r_walk = recall()
        print(f"{count:12d} | {med(scan_ms)} | {med(walk_ms)} | {redo:17d} | {over:3d} of {repeats:3d}      | {r_scan:.4f}"
              f"      | {r_walk:.4f}", flush=True)
        scan_wins = statistics.median(scan_ms) < statistics.median(walk_ms)
        if scan_wins or over:
            chosen = count
        if not scan_wins and not over:
            break
        count *= 2
    print(f"# largest measured count at which the scan still beats the walk or the walk still overflows: {chosen}")
    bf.close()
    L.expann_graph_destroy(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent build's libexpann_hip.so")
    ap.add_argument("--rows", type=int, default=N)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--graph", default=None)
    a = ap.parse_args()
    if a.worker == "unfiltered":
        return worker_unfiltered(a.graph, a.repeats)
    if a.worker == "filtered":
        return worker_filtered(a.graph, a.repeats)
    with tempfile.TemporaryDirectory() as tmp:
        path = build(tmp, a.rows)
        me = [sys.executable, os.path.abspath(__file__), "--graph", path, "--repeats", str(a.repeats)]
        if a.parent_lib:
            print(f"\n# 1. unfiltered walk, kernel ms, one process per run, {a.rounds} rounds of parent then this build, "
                  f"{a.repeats} timed searches each after a warm one")
            series = {"parent": [], "this": []}
            for r in range(a.rounds):
                for name in ("parent", "this"):
                    env = dict(os.environ)
                    env.pop("EXPANN_LIB", None)
                    if name == "parent":
                        env["EXPANN_LIB"] = os.path.abspath(a.parent_lib)
                    out = subprocess.run(me + ["--worker", "unfiltered"], check=True, capture_output=True, text=True, env=env)
                    ms = json.loads(out.stdout.strip().splitlines()[-1])["kernel_ms"]
                    series[name] += ms
                    print(f"round {r} {name:6s}: {med(ms)}", flush=True)
            p, t = series["parent"], series["this"]
            inside = min(p) <= statistics.median(t) <= max(p)
            print(f"parent: {med(p)}\nthis  : {med(t)}\nthis build's median is {'INSIDE' if inside else 'OUTSIDE'} the "
                  f"parent's min .. max", flush=True)
        sys.stdout.flush()
        subprocess.run(me + ["--worker", "filtered"], check=True)


if __name__ == "__main__":
    main()
