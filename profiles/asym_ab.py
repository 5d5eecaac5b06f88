"""Packed-bit rows against int8 queries (expann_search_asym_i8, scan_asym.hpp) on one MI355X.

    python profiles/asym_ab.py [--parent-lib DIR] [--parts recall,throughput,bench] > profiles/asym_ab.txt

  recall      (CPU) Gaussian rows sign-quantised, Gaussian queries scaled to int8: recall@10 of the asymmetric score and
              of the Hamming distance against the exact fp32 inner product over the signs' source rows.
  throughput  1 M rows x 10 000 queries, k = 10: device time between two events on the search's stream around warmed
              steps (a step is the whole search: thresholds, scans, selects); one warm step, then steps until five
              are done or ten seconds have passed (three at least), the median.  The asymmetric search at 256, 1 024,
              1 536 and 3 072 bits; in the same run expann_search with "scan_kernel" 2 (the Hamming matrix-core form)
              on the same rows at 256 and 1 024 bits, and an EXPANN_DTYPE_I8 inner-product index of the +-1 rows at
              256 bits.  The share of the int8 MFMA peak is 2 m n dim operations over the STEP time -- an
              underestimate of the kernel's own share.
              Under EXPANN_LIB the same part times another build's library (how the query re-read was priced against a
              timing-only build that is not in the tree: profiles/asym_ab.txt says so where it quotes it).
  bench       --parent-lib DIR: `bench.py --gpus 1 --steps 60 --warmup 5` on DIR's libexpann_hip.so and on this
              build, alternated rounds; this build's median against the other's min..max."""
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
I8_MFMA_PEAK = 5.0e15  # int8 operations per second (dense, 2.4 GHz), as DESIGN.md 4.8 counts them


def recall():
    print("## ranking quality (CPU): recall@10 against the exact fp32 inner product; 20 000 Gaussian rows, 200 queries")
    for dim in (256, 1024):
        rng = np.random.default_rng(dim)
        src = rng.standard_normal((20_000, dim)).astype(np.float32)
        q = rng.standard_normal((200, dim)).astype(np.float32)
        truth = np.argsort(-(q @ src.T), axis=1, kind="stable")[:, :10]
        signs = np.where(src > 0, 1, -1).astype(np.int32)
        q8 = np.clip(np.rint(q * (127.0 / np.abs(q).max(axis=1, keepdims=True))), -127, 127).astype(np.int32)
        asym = np.argsort(-(q8 @ signs.T), axis=1, kind="stable")[:, :10]
        ham = np.argsort(-(np.where(q > 0, 1, -1).astype(np.int32) @ signs.T), axis=1, kind="stable")[:, :10]
        hit = lambda got: np.mean([len(set(a) & set(b)) / 10.0 for a, b in zip(got, truth)])
        print(f"dim {dim:5d}: asymmetric {hit(asym):.3f}   Hamming {hit(ham):.3f}", flush=True)


def step_ms(search, st):
    import torch
    def one():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        search()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)
    one()
    out, t0 = [], time.perf_counter()
    while len(out) < 3 or (len(out) < 5 and time.perf_counter() - t0 < 10.0):
        out.append(one())
    return statistics.median(out), min(out), max(out)


def measure(kind, dim, rows, queries, k):
    """kind: "asym" (b1 rows, int8 queries), "hamming" (b1 rows, packed queries, scan_kernel 2), "i8ip" (int8 rows and queries)"""
    import torch
    from expann_amd import GpuBruteForceEngine
    m = len(queries)
    t_rows, tq = torch.from_numpy(rows).cuda(), torch.from_numpy(queries).cuda()
    ids = torch.empty(m, k, dtype=torch.int64, device="cuda")
    dd = torch.empty(m, k, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng = GpuBruteForceEngine(dim, "ip", "i8") if kind == "i8ip" else GpuBruteForceEngine(dim, "hamming", "b1")
    eng.set_base_device(t_rows.data_ptr(), len(rows), 0)
    if kind == "hamming":
        eng.set_option("scan_kernel", 2)
    call = eng.search_asym_device if kind == "asym" else eng.search_device
    ms = step_ms(lambda: call(tq.data_ptr(), m, k, ids.data_ptr(), dd.data_ptr(), st.cuda_stream), st)
    nbytes = eng.get_stat("base_bytes")
    eng.close()
    return ms, nbytes  # ms: (median, min, max)


def throughput():
    print("## throughput: 1 M rows, 10 000 queries, k = 10; ms per step (median, min .. max), share of the int8 MFMA peak (from the step time)")
    n, m, k = 1_000_000, 10_000, 10
    for dim in (256, 1024, 1536, 3072):
        rng = np.random.default_rng(dim)
        rows = rng.integers(0, 256, (n, dim // 8), dtype=np.uint8)
        q8 = rng.integers(-128, 128, (m, dim), dtype=np.int8)
        kinds = [("asym", q8, rows)]
        if dim <= 1024:
            kinds.append(("hamming", np.packbits(q8 >= 0, axis=1, bitorder="little"), rows))
        if dim == 256:
            kinds.append(("i8ip", q8, (2 * np.unpackbits(rows, axis=1, bitorder="little").astype(np.int8) - 1)))
        for kind, queries, r in kinds:
            (ms, lo, hi), nb = measure(kind, dim, r, queries, k)
            print(f"dim {dim:5d} {kind:8s}: {ms:10.3f} ms ({lo:.3f} .. {hi:.3f})  {m / ms * 1e3:12.0f} queries/s  "
                  f"{100 * 2.0 * m * n * dim / (ms * 1e-3) / I8_MFMA_PEAK:5.1f} % of the int8 MFMA peak  {nb:12d} bytes of rows",
                  flush=True)


def bench(parent_lib, rounds):
    print(f"## C2 (bench.py --gpus 1 --steps 60 --warmup 5), {rounds} alternated rounds: the JSON lines, then ms_per_step")
    vals = {"parent": [], "this": []}
    for _ in range(rounds):
        for name, lib in (("parent", os.path.join(parent_lib, "libexpann_hip.so")), ("this", None)):
            env = dict(os.environ)
            if lib:
                env["EXPANN_LIB"] = lib
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "5"],
                               env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                print(r.stderr[-2000:])
                sys.exit(r.returncode)
            line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
            vals[name].append(line)
            print(name, json.dumps(line), flush=True)
    key = "ms_per_step"
    p, t = [x[key] for x in vals["parent"]], [x[key] for x in vals["this"]]
    print(f"{key}: parent min {min(p)} max {max(p)}; this build median {statistics.median(t)} "
          f"-> {'inside' if min(p) <= statistics.median(t) <= max(p) else 'OUTSIDE'} the parent's spread")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parts", default="recall,throughput,bench")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    for part in a.parts.split(","):
        if part == "bench":
            if a.parent_lib:
                bench(a.parent_lib, a.rounds)
        else:
            {"recall": recall, "throughput": throughput}[part]()
