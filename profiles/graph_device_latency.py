"""Host-to-host latency of a graph search: host buffers (expann_graph_search_mode) against device buffers
(expann_graph_search_device + expann_graph_sync), on one MI355X.  The two are entry points of one search path (one
set of kernel instances, one plan, the same launches), so their kernel ms should agree; what differs is the staging
and the host waits around them.

    python profiles/graph_device_latency.py [--rows 100000] [--parent-lib DIR] > profiles/graph_device_latency.txt

Part 1: a 100 k x d128 SIFT-like graph from the batched builder (M = 16, ef_construction = 80); for
m in {1, 32, 1000, 10000}, k = 10, ef = 60, modes 0 and 1, alternating within this one process
  (a) expann_graph_search_mode, pageable host buffers in and out,
  (b) expann_graph_search_device + expann_graph_sync on resident torch tensors,
  (c) 16 device searches and one sync, divided by 16,
every shape warmed up first, at least 200 calls per point or at least 0.5 s; kernel ms of (a) and (b) from the
handle's events, and the redo launch's share of (b) (no walk overflows at these shapes: it finds an empty list;
(a) reads the count after its first launch and does not enqueue one).

Part 2 (--parent-lib DIR, a directory holding another build's libexpann_hip.so): the host-buffer call's kernel
time in the C4 shape of `bench.py --workload c4` (1 M rows, M = 60, ef_construction = 480, 10 k queries, k = 10,
ef = 60), the other build and this one alternating through expann_graph_tool on one index file."""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sift_like(rng, n, d, frac=False):
    x = np.clip(np.round(np.abs(rng.standard_normal((n, d))) * 40.0), 0, 255).astype(np.float32)
    if frac:
        x = np.minimum(255.5, x + rng.uniform(0, 0.99, size=x.shape)).astype(np.float32)
    return x


def read_index_csr(path):
    """(starting vertex, n_layers, offsets uint64 [n_layers][n+1], neighbours uint32) of an index file in the
    reference's layout (src/antitopo_engine.h:932-991)"""
    raw = open(path, "rb").read()
    pos = 0

    def take(fmt):
        nonlocal pos
        v = struct.unpack_from("<" + fmt, raw, pos)
        pos += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]
    sv = take("QQQQ")[0]
    if take("B"):
        take("Q")
    take("QQ"), take("ff"), take("Q"), take("BB")
    n_layers, n = take("Q"), take("Q")
    for _ in range(n):
        d = take("Q")
        pos += 4 * d
    assert take("Q") == n
    rec = np.dtype([("d", "<f4"), ("id", "<u8")])
    lists = [[] for _ in range(n_layers)]
    deg = np.zeros((n_layers, n), np.uint64)
    for v in range(n):
        for layer in range(take("Q")):
            ne = take("Q")
            lists[layer].append(np.frombuffer(raw, dtype=rec, count=ne, offset=pos)["id"].astype(np.uint32))
            deg[layer, v] = ne
            pos += 12 * ne
    off = np.zeros((n_layers, n + 1), np.uint64)
    base = 0
    for layer in range(n_layers):
        off[layer, 0] = base
        off[layer, 1:] = base + np.cumsum(deg[layer])
        base += int(deg[layer].sum())
    return sv, n_layers, off, np.concatenate([x for per in lists for x in per])


def part1(rows):
    import torch
    from expann_amd import AntitopoEngine, _lib
    L = _lib.load()
    d, k, ef = 128, 10, 60
    rng = np.random.RandomState(7)
    base = sift_like(rng, rows, d)
    q_all = sift_like(rng, 10000, d, frac=True)
    eng = AntitopoEngine(16, 80, 1, 0, False, dim=d)
    t0 = time.perf_counter()
    eng.store_many_vectors_batched(base, False)
    eng.build()
    with tempfile.TemporaryDirectory() as tmp:
        idx = os.path.join(tmp, "latency.index")
        eng.save_index(idx)
        sv, n_layers, off, nb = read_index_csr(idx)
    eng.close()
    h = C.c_void_p()
    rc = L.expann_graph_create(d, 0, base.ctypes.data, rows, n_layers, sv, off.ctypes.data, nb.ctypes.data, C.byref(h))
    assert rc == 0, L.expann_graph_last_error(None)
    print(f"# graph: {rows} x d{d} SIFT-like rows, batched builder, M = 16, ef_construction = 80, {n_layers} layers, "
          f"built and uploaded in {time.perf_counter() - t0:.1f} s; k = {k}, ef_search = {ef}")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    st = torch.cuda.Stream()
    tq_all = torch.from_numpy(q_all).cuda()
    torch.cuda.synchronize()
    stat = C.c_uint64()

    def get_stat(name):
        assert L.expann_graph_get_stat(h, name, C.byref(stat)) == 0
        return stat.value
    print("# us per search, host to host: median (min) over the calls; kernel ms: median [min .. max]")
    print("mode m     | (a) host buffers      kernel ms (a)            | (b) device + sync     kernel ms (b)            "
          "redo launch us | (c) 16 device, 1 sync | calls a/b/c | same bits")
    for mode in (0, 1):
        for m in (1, 32, 1000, 10000):
            q = np.ascontiguousarray(q_all[:m])
            ids_h, d_h, dc_h = np.zeros((m, k), np.uint64), np.zeros((m, k), np.float32), np.zeros(m, np.uint32)
            ids_d = torch.zeros((16, m, k), dtype=torch.int64, device="cuda")
            d_d = torch.zeros((16, m, k), dtype=torch.float32, device="cuda")
            dc_d = torch.zeros((16, m), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def run_a():
                rc = L.expann_graph_search_mode(h, q.ctypes.data, m, k, ef, mode, ids_h.ctypes.data, d_h.ctypes.data,
                                                dc_h.ctypes.data)
                assert rc == 0, L.expann_graph_last_error(h)

            def enqueue(i):
                rc = L.expann_graph_search_device(h, tq_all.data_ptr(), m, k, ef, mode, ids_d[i].data_ptr(),
                                                  d_d[i].data_ptr(), dc_d[i].data_ptr(), st.cuda_stream)
                assert rc == 0, L.expann_graph_last_error(h)

            def run_b():
                enqueue(0)
                assert L.expann_graph_sync(h) == 0, L.expann_graph_last_error(h)

            def run_c():
                for i in range(16):
                    enqueue(i)
                assert L.expann_graph_sync(h) == 0, L.expann_graph_last_error(h)
            for f in (run_a, run_b, run_c):  # warm-up of every shape
                for _ in range(3):
                    f()
            same = (np.array_equal(ids_d[15].cpu().numpy().view(np.uint64), ids_h)
                    and np.array_equal(d_d[15].cpu().numpy().view(np.uint32), d_h.view(np.uint32))
                    and np.array_equal(dc_d[15].cpu().numpy().view(np.uint32), dc_h))
            ta, tb, tc, ka, kb, redo_us = [], [], [], [], [], []
            redone = 0

            def enough(calls, seconds):
                return calls >= 200 or seconds >= 0.5
            while not (enough(len(ta), sum(ta)) and enough(len(tb), sum(tb)) and enough(16 * len(tc), 16 * sum(tc))):
                for _ in range(8):  # (a), (b) and (c) alternate in short blocks
                    t = time.perf_counter()
                    run_a()
                    ta.append(time.perf_counter() - t)
                    ka.append(L.expann_graph_last_kernel_ms(h))
                for _ in range(8):
                    t = time.perf_counter()
                    run_b()
                    tb.append(time.perf_counter() - t)
                    kb.append(L.expann_graph_last_kernel_ms(h))
                    redo_us.append(get_stat(b"redo_kernel_ns") / 1e3)
                    redone += get_stat(b"redo_queries")
                t = time.perf_counter()
                run_c()
                tc.append((time.perf_counter() - t) / 16)
            assert redone == 0, "a walk overflowed: the redo launch was not empty"

            def us(x):
                return f"{statistics.median(x) * 1e6:9.1f} ({min(x) * 1e6:9.1f})"

            def ms(x):
                return f"{statistics.median(x):7.4f} [{min(x):7.4f} .. {max(x):7.4f}]"
            print(f"{mode}    {m:<5d} | {us(ta)} {ms(ka)} | {us(tb)} {ms(kb)} {statistics.median(redo_us):8.1f}"
                  f"       | {us(tc)} | {len(ta)}/{len(tb)}/{16 * len(tc)} | {same}", flush=True)
    print(f"# device searches enqueued: {get_stat(b'deferred_searches')}, ended in overflow: {get_stat(b'redo_overflows')}")
    L.expann_graph_destroy(h)


def part2(parent_dir, rounds):
    tool = os.path.join(ROOT, "expann_amd", "host", "expann_graph_tool")
    this_dir = os.path.join(ROOT, "expann_amd")
    n, m, d, k, M, efc, ef = 1_000_000, 10_000, 128, 10, 60, 480, 60
    print(f"\n# host-buffer path, kernel ms of the C4 shape ({n} x d{d}, M = {M}, ef_construction = {efc}, {m} queries, "
          f"k = {k}, ef_search = {ef}): expann_graph_tool on one index file, the two builds alternating, one process "
          "per run, three timed searches per mode and run (each after a warm one)")
    with tempfile.TemporaryDirectory() as tmp:
        idx, qf = os.path.join(tmp, "c4.index"), os.path.join(tmp, "c4.queries")
        common = [str(x) for x in ("--m", m, "--d", d, "--k", k, "--M", M, "--ef_construction", efc, "--data", "sift",
                                   "--index", idx, "--queries", qf)]
        subprocess.run([tool, "--n", str(n), "--batched", "1024", "--build-only", "1"] + common, check=True,
                       capture_output=True, text=True)
        series = {("parent", 0): [], ("parent", 1): [], ("this", 0): [], ("this", 1): []}
        for r in range(rounds):
            for name, lib_dir in (("parent", parent_dir), ("this", this_dir)):
                env = dict(os.environ, LD_LIBRARY_PATH=lib_dir + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
                out = subprocess.run([tool, "--n", "0", "--read-index", "1", "--ef", f"{ef},{ef},{ef}"] + common,
                                     check=True, capture_output=True, text=True, env=env)
                for line in out.stdout.strip().splitlines():
                    x = json.loads(line)
                    if x["phase"] == "query":
                        series[(name, x["use_compression"])].append(x["kernel_ms"])
                print(f"round {r} {name:6s}: fp32 {series[(name, 0)][-3:]}  uint8 {series[(name, 1)][-3:]}", flush=True)
    for comp, label in ((0, "fp32"), (1, "uint8")):
        p, t = series[("parent", comp)], series[("this", comp)]
        spread = max(p) - min(p)
        delta = statistics.median(t) - statistics.median(p)
        inside = min(p) <= statistics.median(t) <= max(p)
        print(f"{label}: parent median {statistics.median(p):.4f} ms, spread (max - min) {spread:.4f} ms; this build median "
              f"{statistics.median(t):.4f} ms; difference of the medians {delta:+.4f} ms -> "
              f"{'within' if abs(delta) <= spread else 'OUTSIDE'} the parent's spread"
              f"{'' if inside else ' (but not between the parent runs smallest and largest)'}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--parent-lib", default=None, help="directory with the libexpann_hip.so of the build to compare with")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--skip-latency", action="store_true")
    a = ap.parse_args()
    if not a.skip_latency:
        part1(a.rows)
    if a.parent_lib:
        part2(os.path.abspath(a.parent_lib), a.rounds)
