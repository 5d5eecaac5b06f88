"""The graph engine's range search (THE RANGE WALK RULE, include/expann_hip.h), measured on one MI355X.

    python profiles/graph_range_ab.py --parent-root /path/to/a/built/checkout/of/the/parent > profiles/graph_range_ab.txt
    python profiles/graph_range_ab.py --resource-usage >> profiles/graph_range_ab.txt        (needs hipcc, no device)

  1. the PLAIN walk against the parent: `python bench.py --workload c4` in the parent's checkout and in this one,
     alternating, --bench-runs runs each (a run builds its own graph with the batched builder and times the sweep).
     Its ms_per_step (the best fp32 configuration's time over the batch) and that configuration's kernel ms: this
     build's median must lie inside the parent's min .. max.  Only the parameter struct and the LDS layout helper
     changed for the plain instances.
  2. the RANGE walk on the C4 graph of profiles/graph_filter_ab.py (1 M x d128 SIFT-like rows, M = 60, ef_construction
     = 480; 10 k queries), ef_search = 60, radii at each query's exact 10th / 100th / 1000th neighbour distance (the
     brute-force index's distances), max_results 16 / 256 / 1024: kernel ms (first launch + redo launch, device
     events), rows counted against the exact count of expann_range_search on a brute-force index of the same rows,
     "redo_queries", and that brute-force range search's own time (host clock around the call, which waits) for scale.
  3. (--resource-usage) the -Rpass-analysis=kernel-resource-usage lines of the range instances of graph_search_kernel.
Medians of --repeats runs with their min .. max."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from graph_filter_ab import D, EF, build, med, open_graph  # noqa: E402

RANKS = (10, 100, 1000)
MAX_RESULTS = (16, 256, 1024)


def bench_c4(root):
    """one `bench.py --workload c4` in the checkout at `root`: (ms_per_step, kernel ms of the best fp32 configuration)"""
    env = dict(os.environ)
    env.pop("EXPANN_LIB", None)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "c4", "--gpus", "1", "--steps", "1",
                          "--warmup", "1"], cwd=root, check=True, capture_output=True, text=True, env=env)
    j = json.loads(out.stdout.strip().splitlines()[-1])
    return j["ms_per_step"], j["roofline"]["kernel_ms"]


def section_plain(parent_root, runs, budget_s):
    t_start = time.perf_counter()
    print(f"# 1. plain walk: python bench.py --workload c4, {runs} runs each, parent then this build, alternating\n"
          "#    ms_per_step = the best fp32 configuration of the sweep over the batch; kernel ms = its walk launch")
    series = {"parent": [], "this": []}
    for r in range(runs):
        for name, root in (("parent", parent_root), ("this", ROOT)):
            step, kernel = bench_c4(root)
            series[name].append((step, kernel))
            print(f"run {r} {name:6s}: ms_per_step {step:8.3f}   kernel ms {kernel:8.3f}", flush=True)
        if budget_s and time.perf_counter() - t_start > budget_s and r + 1 < runs:
            print(f"# stopped after {r + 1} runs each: --plain-budget-s {budget_s} is used up", flush=True)
            break
    for col, what in ((0, "ms_per_step"), (1, "kernel ms  ")):
        p, t = [x[col] for x in series["parent"]], [x[col] for x in series["this"]]
        inside = min(p) <= statistics.median(t) <= max(p)
        print(f"{what} parent: {med(p)}\n{what} this  : {med(t)}   this build's median is "
              f"{'INSIDE' if inside else 'OUTSIDE'} the parent's min .. max", flush=True)


def worker_range(path, repeats):
    import torch
    from expann_amd import GpuBruteForceEngine
    L, h, base, q = open_graph(path)
    m = q.shape[0]
    bf = GpuBruteForceEngine(D, "l2")
    bf.store_many_vectors(base)
    bf.build()
    _, kd = bf.query_k_batch(q, max(RANKS))  # the exact neighbour distances: the radii
    tq = torch.from_numpy(q).cuda()
    st = torch.cuda.Stream()
    out = C.c_uint64()

    def stat(name):
        assert L.expann_graph_get_stat(h, name, C.byref(out)) == 0
        return out.value
    print(f"\n# 2. range walk, ef_search = {EF}, {m} queries; kernel ms and brute-force ms: median [min .. max] of "
          f"{repeats} runs after a warm one\nradius at rank | max_results | range walk kernel ms             | counted / true rows    "
          "| share   | returned rows | redo_queries | brute-force expann_range_search ms", flush=True)
    for rank in RANKS:
        radii = np.ascontiguousarray(kd[:, rank - 1])
        tr = torch.from_numpy(radii).cuda()
        for R in MAX_RESULTS:
            ids = torch.zeros((m, R), dtype=torch.int64, device="cuda")
            dists = torch.zeros((m, R), dtype=torch.float32, device="cuda")
            cnt = torch.zeros(m, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def run():
                rc = L.expann_graph_range_search_device(h, tq.data_ptr(), tr.data_ptr(), m, R, EF, ids.data_ptr(),
                                                        dists.data_ptr(), cnt.data_ptr(), None, st.cuda_stream)
                assert rc == 0, L.expann_graph_last_error(h)
                assert L.expann_graph_sync(h) == 0, L.expann_graph_last_error(h)
                return L.expann_graph_last_kernel_ms(h)
            run()  # warm
            ms = [run() for _ in range(repeats)]
            redo = stat(b"redo_queries")
            counted = cnt.cpu().numpy().view(np.uint32).astype(np.int64)
            returned = int((ids.cpu().numpy().view(np.uint64) != np.uint64(2 ** 64 - 1)).sum())
            bf.range_search(q, radii, R)  # warm
            bf_ms, true = [], None
            for _ in range(repeats):
                t0 = time.perf_counter()
                _, _, true = bf.range_search(q, radii, R)
                bf_ms.append((time.perf_counter() - t0) * 1e3)
            true = true.astype(np.int64)
            assert (counted <= true).all()  # the walk never counts a row that is not in range
            print(f"{rank:14d} | {R:11d} | {med(ms)} | {counted.sum():10d} / {true.sum():10d} | {counted.sum() / true.sum():7.4f} "
                  f"| {returned:13d} | {redo:12d} | {med(bf_ms)}", flush=True)
    print(f"# range_searches: {stat(b'range_searches')}")
    bf.close()
    L.expann_graph_destroy(h)


def resource_usage():
    """the compiler's resource-usage remarks for the range instances (KIND = 3) of graph_search_kernel"""
    src = os.path.join(ROOT, "expann_amd", "csrc", "expann_graph.hip")
    with tempfile.TemporaryDirectory() as tmp:
        res = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC",
                              "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "expann"),
                              "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                              os.path.join(tmp, "graph.o")], capture_output=True, text=True, check=True)
    print("\n# 3. -Rpass-analysis=kernel-resource-usage, the range instances graph_search_kernel<D, kGraphF32, 0, kFilterRange, TR>\n"
          "#    (hipcc -O3 --offload-arch=gfx950; D = 0: the run-time-dim instance; TR f = float rows, DF16_ = binary16 rows)\n"
          "D    | TR    | VGPRs | AGPRs | SGPRs | ScratchSize [bytes/lane] | Occupancy [waves/SIMD] | LDS [bytes/block, static]")
    blocks = re.split(r"(?=remark: [^\n]*Function Name: )", res.stderr)
    worst = 0
    for b in blocks:
        name = re.search(r"Function Name: (\S+)", b)
        k = name and re.match(r"_ZN6expann19graph_search_kernelILi(\d+)ELi0ELi0ELi3E(f|DF16_)E", name.group(1))
        if not k:
            continue
        f = lambda key: int(re.search(key + r": (\d+)", b).group(1))  # noqa: E731
        scratch, occ, lds = f(r"ScratchSize \[bytes/lane\]"), f(r"Occupancy \[waves/SIMD\]"), f(r"LDS Size \[bytes/block\]")
        worst = max(worst, scratch)
        print(f"{int(k.group(1)):4d} | {k.group(2):5s} | {f('VGPRs'):5d} | {f('AGPRs'):5d} | {f('SGPRs'):5d} | {scratch:24d} | "
              f"{occ:22d} | {lds:5d}")
    print(f"# largest ScratchSize over the range instances: {worst} bytes/lane")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, built (its bench.py is run there)")
    ap.add_argument("--bench-runs", type=int, default=5)
    ap.add_argument("--plain-budget-s", type=float, default=0, help="start no further pair of bench runs after this many seconds")
    ap.add_argument("--sections", default="plain,range", help="which of the sections 1 (plain) and 2 (range) to run")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--resource-usage", action="store_true")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--graph", default=None)
    a = ap.parse_args()
    if a.resource_usage:
        return resource_usage()
    if a.worker == "range":
        return worker_range(a.graph, a.repeats)
    if a.parent_root and "plain" in a.sections:
        section_plain(os.path.abspath(a.parent_root), a.bench_runs, a.plain_budget_s)
    if "range" not in a.sections:
        return
    with tempfile.TemporaryDirectory() as tmp:
        path = build(tmp, a.rows)
        sys.stdout.flush()
        subprocess.run([sys.executable, os.path.abspath(__file__), "--graph", path, "--repeats", str(a.repeats), "--worker",
                        "range"], check=True)


if __name__ == "__main__":
    main()
