"""The graph engine over binary16 rows (expann_graph_create_f16), measured on the C4 graph (1 M x d128 SIFT-like rows,
M = 60, ef_construction = 480, batched build; 10 k queries, k = 10, ef_search = 60) on one MI355X.

    python profiles/graph_f16_ab.py --parent-lib /path/to/parent/libexpann_hip.so [--alt-lib LABEL=/path/to/lib.so]
        [--build-times "text"] > profiles/graph_f16_ab.txt

  1. the fp32 walk of an fp32 handle in this build and in the parent build (EXPANN_LIB selects the library; one
     process per run, the two builds alternating): this build's median must lie inside the parent's own min .. max,
     or the element type has leaked into the float instances;
  2. the binary16 handle against the fp32 handle over the same graph and the same values (SIFT-like integers are
     binary16 values): walk kernel ms in modes 0 and 2, distcomps (must be equal), algorithmic row bytes per second
     (mode 0: scored rows x the bytes of a row; mode 2: scored rows x d bytes of the int8 copy plus the k re-scored
     rows; over the kernel time) against the 8 TB/s HBM peak, "vector_bytes"; the same
     at one run-time dim (--any-dim, 1 M x d144 by default); --alt-lib adds another build of this tree (a variant
     under trial, such as twice the rows in flight in the compiled binary16 instances) to the d128 table;
  3. build times, handed in by --build-times (they are measured where the library is compiled).
One process per (library, handle) and round, the handles alternating; medians of the rounds' timed searches with
their min .. max."""
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
HBM_PEAK = 8.0e12


def med(x):
    return f"{statistics.median(x):8.3f} [{min(x):8.3f} .. {max(x):8.3f}]"


def build(tmp, rows, d):
    """the graph through the batched builder (the C ABI: the engine is opened at exactly d); base, queries and the CSR
    form of the index go to one .npz"""
    from expann_amd import _lib
    from graph_device_latency import read_index_csr, sift_like
    L = _lib.load()
    rng = np.random.RandomState(7 + d)
    base = sift_like(rng, rows, d)
    q = sift_like(rng, M_Q, d, frac=True)
    assert np.array_equal(base.astype(np.float16).astype(np.float32), base)
    t0 = time.perf_counter()
    e = C.c_void_p()
    assert L.expann_antitopo_create(d, 0, GRAPH_M, EFC, 1, 0, 0, C.byref(e)) == 0, L.expann_antitopo_last_error(None)
    assert L.expann_antitopo_store_batched(e, base.ctypes.data, rows, 0) == 0, L.expann_antitopo_last_error(e)
    idx = os.path.join(tmp, f"c4_{d}.index")
    assert L.expann_antitopo_save(e, idx.encode()) == 0
    L.expann_antitopo_destroy(e)
    t1 = time.perf_counter()
    sv, n_layers, off, nb = read_index_csr(idx)
    os.remove(idx)
    path = os.path.join(tmp, f"c4_{d}.npz")
    np.savez(path, base=base, q=q, sv=sv, n_layers=n_layers, off=off, nb=nb)
    print(f"# graph: {rows} x d{d} SIFT-like rows, batched builder, M = {GRAPH_M}, ef_construction = {EFC}, {n_layers} "
          f"layers, built in {t1 - t0:.1f} s; {M_Q} queries, k = {K}, ef_search = {EF}", flush=True)
    return path


def worker(path, rows, mode, repeats):
    """one handle (rows: "f32" or "f16"), `repeats` timed device-buffer searches after a warm one"""
    import torch
    from expann_amd import _lib
    L = _lib.load()
    z = np.load(path)
    base, q = np.ascontiguousarray(z["base"]), np.ascontiguousarray(z["q"])
    off, nb = np.ascontiguousarray(z["off"]), np.ascontiguousarray(z["nb"])
    n, d = base.shape
    h = C.c_void_p()
    if rows == "f16":
        halves = base.astype(np.float16)
        rc = L.expann_graph_create_f16(d, 0, halves.ctypes.data, n, int(z["n_layers"]), int(z["sv"]), off.ctypes.data,
                                       nb.ctypes.data, C.byref(h))
    else:
        rc = L.expann_graph_create(d, 0, base.ctypes.data, n, int(z["n_layers"]), int(z["sv"]), off.ctypes.data,
                                   nb.ctypes.data, C.byref(h))
    assert rc == 0, L.expann_graph_last_error(None)
    tq = torch.from_numpy(q).cuda()
    ids = torch.zeros((q.shape[0], K), dtype=torch.int64, device="cuda")
    dists = torch.zeros((q.shape[0], K), dtype=torch.float32, device="cuda")
    dc = torch.zeros((q.shape[0],), dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def run():
        rc = L.expann_graph_search_device(h, tq.data_ptr(), tq.shape[0], K, EF, mode, ids.data_ptr(), dists.data_ptr(),
                                          dc.data_ptr(), st.cuda_stream)
        assert rc == 0, L.expann_graph_last_error(h)
        assert L.expann_graph_sync(h) == 0, L.expann_graph_last_error(h)
        return L.expann_graph_last_kernel_ms(h)
    run()
    ms = [run() for _ in range(repeats)]
    out = {"kernel_ms": ms, "distcomps": int(dc.cpu().numpy().astype(np.int64).sum()),
           "ids_crc": int(ids.cpu().numpy().astype(np.uint64).sum() % (1 << 61)),
           "dist_crc": int(dists.cpu().numpy().view(np.uint32).astype(np.uint64).sum() % (1 << 61))}
    if hasattr(L, "expann_graph_create_f16"):
        vb = C.c_uint64()
        assert L.expann_graph_get_stat(h, b"vector_bytes", C.byref(vb)) == 0
        out["vector_bytes"] = vb.value
    print(json.dumps(out))
    L.expann_graph_destroy(h)


def run_worker(me, path, rows, mode, repeats, lib):
    env = dict(os.environ)
    env.pop("EXPANN_LIB", None)
    if lib:
        env["EXPANN_LIB"] = os.path.abspath(lib)
    out = subprocess.run(me + ["--worker", rows, "--graph", path, "--mode", str(mode), "--repeats", str(repeats)],
                         check=True, capture_output=True, text=True, env=env)
    return json.loads(out.stdout.strip().splitlines()[-1])


def part2(me, path, d, modes, libs, rounds, repeats):
    """libs: [(label, path or None)]; every (label, rows, mode) in every round, in turn"""
    print("build  rows mode | kernel ms                        | distcomps    | vector_bytes | row bytes / s      | of the HBM peak")
    for mode in modes:
        res = {}
        for r in range(rounds):
            for label, lib in libs:
                for rows in ("f32", "f16"):
                    o = run_worker(me, path, rows, mode, repeats, lib)
                    a = res.setdefault((label, rows), dict(o, kernel_ms=[]))
                    a["kernel_ms"] += o["kernel_ms"]
                    assert (a["distcomps"], a["ids_crc"], a["dist_crc"]) == (o["distcomps"], o["ids_crc"], o["dist_crc"])
        first = next(iter(res.values()))
        for (label, rows), a in res.items():
            # the same answers from every handle and build: distcomps, ids and distance bits
            assert (a["distcomps"], a["ids_crc"], a["dist_crc"]) == (first["distcomps"], first["ids_crc"], first["dist_crc"])
            t = statistics.median(a["kernel_ms"]) * 1e-3
            elem = 2 if rows == "f16" else 4
            # bytes the scoring asks for: mode 0 reads a row per scored vertex; the byte modes read its d bytes of the
            # int8 copy, and the rows only for the final re-score of the k results
            bps = (a["distcomps"] * d * elem if mode == 0 else a["distcomps"] * d + M_Q * K * d * elem) / t
            print(f"{label:6s} {rows}  {mode}   | {med(a['kernel_ms'])} | {a['distcomps']:12d} | {a['vector_bytes']:12d} | "
                  f"{bps / 1e12:6.2f} TB/s        | {bps / HBM_PEAK:.2f}", flush=True)
        for label, _ in libs:
            f32, f16 = (statistics.median(res[(label, r)]["kernel_ms"]) for r in ("f32", "f16"))
            print(f"# {label}, mode {mode}: f16 / f32 kernel time = {f16 / f32:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent build's libexpann_hip.so")
    ap.add_argument("--alt-lib", default=None, help="LABEL=path: another build of this tree for the d128 table of part 2")
    ap.add_argument("--build-times", default=None)
    ap.add_argument("--rows", type=int, default=N)
    ap.add_argument("--any-dim", type=int, default=144)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--graph", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a.graph, a.worker, a.mode, a.repeats)
    me = [sys.executable, os.path.abspath(__file__)]
    with tempfile.TemporaryDirectory() as tmp:
        path = build(tmp, a.rows, D)
        if a.parent_lib:
            print(f"\n# 1. fp32 walk of an fp32 handle, kernel ms, one process per run, {a.rounds} rounds of parent then this "
                  f"build, {a.repeats} timed searches each after a warm one")
            series = {"parent": [], "this": []}
            for r in range(a.rounds):
                for name in ("parent", "this"):
                    ms = run_worker(me, path, "f32", 0, a.repeats, a.parent_lib if name == "parent" else None)["kernel_ms"]
                    series[name] += ms
                    print(f"round {r} {name:6s}: {med(ms)}", flush=True)
            p, t = series["parent"], series["this"]
            inside = min(p) <= statistics.median(t) <= max(p)
            print(f"parent: {med(p)}\nthis  : {med(t)}\nthis build's median is {'INSIDE' if inside else 'OUTSIDE'} the "
                  f"parent's min .. max", flush=True)
        libs = [("this", None)]
        if a.alt_lib:
            label, lib = a.alt_lib.split("=", 1)
            libs.append((label, lib))
        rounds = max(2, a.rounds - 2)
        print(f"\n# 2. binary16 handle against fp32 handle, d = {D}: {rounds} rounds, handles (and builds) in turn, "
              f"{a.repeats} timed searches each; median [min .. max]")
        part2(me, path, D, (0, 2), libs, rounds, a.repeats)
        os.remove(path)
        if a.any_dim:
            print(f"\n# 2b. the same at a run-time dim, d = {a.any_dim}, mode 0")
            path = build(tmp, a.rows, a.any_dim)
            part2(me, path, a.any_dim, (0,), [("this", None)], rounds, a.repeats)
    if a.build_times:
        print("\n# 3. build times\n" + a.build_times)


if __name__ == "__main__":
    main()
