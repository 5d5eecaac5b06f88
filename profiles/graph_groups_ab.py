"""The graph engine's row groups, measured on the C4 graph of profiles/graph_filter_ab.py (1 M x d128 SIFT-like rows,
M = 60, ef_construction = 480, batched build; 10 k queries, k = 10, ef_search = 60) on one MI355X.

    python profiles/graph_groups_ab.py --parent-lib /path/to/parent/libexpann_hip.so > profiles/graph_groups_ab.txt

  1. the PLAIN unfiltered walk's kernel time in this build and in the parent build (graph_filter_ab's section 1: one
     process per run, the builds interleaved): this build's median must lie inside the parent's min .. max;
  2. an ALL-ANY batch through the grouped entry against the plain search of this build: the ratio, printed beside the
     bitmap's all-ones figure (x 1.045, profiles/graph_filter_ab.txt);
  3. THE CASE THIS IS FOR: 1 000 groups of 1 000 rows, every query names a random group.  One grouped call against
     what a caller does without groups: per distinct group one expann_graph_set_row_filter plus one search of that
     group's queries.  Both host to host (wall clock around enqueue .. sync); the directory's set time separately;
  4. CROSSOVER: one group size per run (1 k .. 256 k rows, every query in it), the grouped scan ("filter_flat_rows" =
     the size) against the grouped walk ("filter_flat_rows" = 1): the rows to read beside section 3 of
     profiles/graph_filter_ab.txt.
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
from graph_filter_ab import EF, K, N, Searcher, build, med, open_graph, worker_unfiltered  # noqa: E402

ANY = 0xFFFFFFFF


class GroupedSearcher(Searcher):
    def set_groups(self, labels, flat_rows):
        L, h = self.L, self.h
        labels = np.ascontiguousarray(labels, dtype=np.uint32)
        assert L.expann_graph_set_option(h, b"filter_flat_rows", flat_rows) == 0
        t0 = time.perf_counter()
        assert L.expann_graph_set_row_groups(h, labels.ctypes.data, labels.size) == 0, L.expann_graph_last_error(h)
        return (time.perf_counter() - t0) * 1e3

    def set_query_groups(self, qg):
        self.tqg = self.torch.from_numpy(np.ascontiguousarray(qg, dtype=np.uint32).view(np.int32)).cuda()
        self.torch.cuda.synchronize()

    def run_grouped(self):
        """one grouped device-buffer search and its sync: (kernel ms, wall ms, redo queries, overflowed)"""
        L, h = self.L, self.h
        t0 = time.perf_counter()
        rc = L.expann_graph_search_grouped_device(h, self.tq.data_ptr(), self.tqg.data_ptr(), self.tq.shape[0], K, EF, 0,
                                                  self.ids.data_ptr(), self.dists.data_ptr(), None, self.st.cuda_stream)
        assert rc == 0, L.expann_graph_last_error(h)
        rc = L.expann_graph_sync(h)
        wall = (time.perf_counter() - t0) * 1e3
        assert rc in (0, 6), L.expann_graph_last_error(h)
        return L.expann_graph_last_kernel_ms(h), wall, self.stat(b"redo_queries"), rc == 6

    def timed_grouped(self, repeats):
        self.run_grouped()  # warm
        runs = [self.run_grouped() for _ in range(repeats)]
        return [r[0] for r in runs], [r[1] for r in runs], runs[-1][2], sum(r[3] for r in runs)


def worker_grouped(path, repeats):
    from expann_amd import pack_row_filter
    L, h, base, q = open_graph(path)
    n, m = base.shape[0], q.shape[0]
    s = GroupedSearcher(L, h, q)
    rng = np.random.RandomState(23)
    # 2. all-ANY against the plain search
    plain, _, _ = s.timed(repeats)
    s.set_groups(np.zeros(n, np.uint32), 0)
    s.set_query_groups(np.full(m, ANY, np.uint32))
    any_ms, _, _, _ = s.timed_grouped(repeats)
    ratio = statistics.median(any_ms) / statistics.median(plain)
    print(f"\n# 2. all-ANY batch through the grouped entry against the plain search; kernel ms: median [min .. max] of "
          f"{repeats} runs\nplain   : {med(plain)}\nall-ANY : {med(any_ms)}   (x {ratio:.3f} of plain; the bitmap's all-ones "
          f"filter: x 1.045)", flush=True)
    # 3. 1 000 groups of 1 000 rows, every query names a random group
    G, per = 1000, n // 1000
    labels = np.full(n, ANY, np.uint32)
    perm = rng.permutation(n)
    for g in range(G):
        labels[perm[g * per:(g + 1) * per]] = g
    qg = rng.randint(0, G, m).astype(np.uint32)
    set_ms = [s.set_groups(labels, 0) for _ in range(3)]
    s.set_query_groups(qg)
    k_ms, wall, _, over = s.timed_grouped(repeats)
    print(f"\n# 3. {G} groups of {per} rows, {m} queries, each names a random group\nset_row_groups (host labels, the "
          f"directory made on the host): {med(set_ms)} ms\none grouped call, host to host : {med(wall)} ms (kernel "
          f"{med(k_ms)}), overflowed searches {over}", flush=True)
    assert L.expann_graph_clear_row_groups(h) == 0
    # the same without groups: per distinct group one set_row_filter plus one search of that group's queries
    order = np.argsort(qg, kind="stable")
    tq_sorted = s.torch.from_numpy(q[order]).cuda()
    bounds = np.flatnonzero(np.diff(qg[order])) + 1
    starts, ends = np.concatenate([[0], bounds]), np.concatenate([bounds, [m]])
    words = [pack_row_filter(labels == qg[order][a]) for a in starts]  # (packing the bits is not timed)
    s.torch.cuda.synchronize()
    per_tenant = []
    for _ in range(max(1, repeats // 3)):
        t0 = time.perf_counter()
        for a, b, w in zip(starts, ends, words):
            assert L.expann_graph_set_row_filter(h, w.ctypes.data, w.size) == 0
            rc = L.expann_graph_search_device(h, tq_sorted.data_ptr() + int(a) * q.shape[1] * 4, int(b - a), K, EF, 0,
                                              s.ids.data_ptr() + int(a) * K * 8, s.dists.data_ptr() + int(a) * K * 4, None,
                                              s.st.cuda_stream)
            assert rc == 0, L.expann_graph_last_error(h)
        assert L.expann_graph_sync(h) in (0, 6)
        per_tenant.append((time.perf_counter() - t0) * 1e3)
    assert L.expann_graph_clear_row_filter(h) == 0
    print(f"{len(starts)} x (set_row_filter + search), host to host: {med(per_tenant)} ms   (x "
          f"{statistics.median(per_tenant) / statistics.median(wall):.1f} of the grouped call)", flush=True)
    # 4. crossover: every query in one group of `count` rows
    print("\n# 4. grouped scan (\"filter_flat_rows\" = the size) against grouped walk (\"filter_flat_rows\" = 1), every query "
          "in one group\ngroup rows | scan kernel ms                   | walk kernel ms                   | walk redo queries | "
          "walk overflowed")
    s.set_query_groups(np.zeros(m, np.uint32))
    count = 1000
    while count <= min(n, 256000):
        labels = np.full(n, 1, np.uint32)
        labels[perm[:count]] = 0
        s.set_groups(labels, count)
        scan_ms, _, _, _ = s.timed_grouped(repeats)
        s.set_groups(labels, 1)
        walk_ms, _, redo, over = s.timed_grouped(repeats)
        print(f"{count:10d} | {med(scan_ms)} | {med(walk_ms)} | {redo:17d} | {over:3d} of {repeats:3d}", flush=True)
        count *= 2
    for name in (b"group_walk_queries", b"group_scan_queries", b"group_pad_queries"):
        print(f"# {name.decode()}: {s.stat(name)}")
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
    if a.worker == "grouped":
        return worker_grouped(a.graph, a.repeats)
    with tempfile.TemporaryDirectory() as tmp:
        path = build(tmp, a.rows)
        me = [sys.executable, os.path.abspath(__file__), "--graph", path, "--repeats", str(a.repeats)]
        if a.parent_lib:
            print(f"\n# 1. plain unfiltered walk, kernel ms, one process per run, {a.rounds} rounds of parent then this "
                  f"build, {a.repeats} timed searches each after a warm one")
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
        subprocess.run(me + ["--worker", "grouped"], check=True)


if __name__ == "__main__":
    main()
