"""The two Hamming scans over packed-bit rows (EXPANN_DTYPE_B1, scan_hamming.hpp) on one MI355X.

    python profiles/hamming_ab.py [--parent-lib DIR] [--parts throughput,crossover,context,bench] > profiles/hamming_ab.txt

Every figure is device time between two events on the search's stream, around warmed steps of expann_search_device on
resident queries (a step is the whole search: thresholds, scans, selects).  A measurement takes one warm step, then
steps until five are done or ten seconds have passed (three at least); the median is reported.
  throughput  1 M rows x 256 and x 1024 bits, 10 000 queries, k = 10 and 100: ms per step and queries/s of form 1
              (VALU) and form 2 (int8 matrix cores), with the share of the bound that applies computed from the
              shapes over the STEP time (an underestimate of the kernel's own share: selects and thresholds are in
              the step).  Form 2: 2 m n dim operations over the int8 MFMA peak; form 1: 2 VALU lane-operations (xor,
              popcount-accumulate) per pair and dword over the VALU issue rate.
  crossover   256 bits, k = 10, m in {1, 8, 32, 96, 512, 4096} x n in {16 k, 64 k, 1 M}: both forms, the faster named
  context     the same 256 bits stored one per byte as EXPANN_DTYPE_U8 rows under L2 (byte-dim 256): time and bytes
  bench       --parent-lib DIR: `bench.py --gpus 1 --steps 60 --warmup 5` on DIR's libexpann_hip.so and on this
              build, five alternated rounds; this build's median against the other's min..max."""
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
I8_MFMA_PEAK = 5.0e15            # int8 operations per second (dense, 2.4 GHz), as DESIGN.md 4.8 counts them
VALU_PEAK = 256 * 4 * 16 * 2.4e9  # lane-operations per second: 256 CUs x 4 SIMDs x 16 lanes per clock


def step_ms(eng, tq, m, k, ids, dd, st):
    import torch
    def one():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        eng.search_device(tq.data_ptr(), m, k, ids.data_ptr(), dd.data_ptr(), st.cuda_stream)
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)
    one()
    out, t0 = [], time.perf_counter()
    while len(out) < 3 or (len(out) < 5 and time.perf_counter() - t0 < 10.0):
        out.append(one())
    return statistics.median(out)


def measure(dtype, metric, dim, rows, queries, k, scan_kernel):
    import torch
    from expann_amd import GpuBruteForceEngine
    m = len(queries)
    t_rows, tq = torch.from_numpy(rows).cuda(), torch.from_numpy(queries).cuda()
    ids = torch.empty(m, k, dtype=torch.int64, device="cuda")
    dd = torch.empty(m, k, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng = GpuBruteForceEngine(dim, metric, dtype)
    eng.set_base_device(t_rows.data_ptr(), len(rows), 0)
    eng.set_option("scan_kernel", scan_kernel)
    ms = step_ms(eng, tq, m, k, ids, dd, st)
    nbytes = eng.get_stat("base_bytes")
    eng.close()
    return ms, nbytes


def bits(rng, n, dim):
    return rng.integers(0, 256, (n, dim // 8), dtype=np.uint8)


def throughput():
    print("## throughput: 1 M rows, 10 000 queries; ms per step (median), queries/s, share of the bound (from the step time)")
    n, m = 1_000_000, 10_000
    for dim in (256, 1024):
        rng = np.random.default_rng(dim)
        rows, queries = bits(rng, n, dim), bits(rng, m, dim)
        for k in (10, 100):
            for form in (1, 2):
                ms, _ = measure("b1", "hamming", dim, rows, queries, k, form)
                if form == 2:
                    share, bound = 2.0 * m * n * dim / (ms * 1e-3) / I8_MFMA_PEAK, "int8 MFMA peak"
                else:
                    share, bound = 2.0 * m * n * (dim / 32) / (ms * 1e-3) / VALU_PEAK, "VALU issue rate"
                print(f"dim {dim:5d} k {k:4d} form {form}: {ms:10.3f} ms  {m / ms * 1e3:12.0f} queries/s  "
                      f"{100 * share:5.1f} % of the {bound}", flush=True)


def crossover():
    print("## crossover: 256 bits, k = 10; ms per step of form 1 / form 2")
    dim, k = 256, 10
    rng = np.random.default_rng(5)
    all_rows, all_q = bits(rng, 1_000_000, dim), bits(rng, 4096, dim)
    for n in (16_384, 65_536, 1_000_000):
        for m in (1, 8, 32, 96, 512, 4096):
            t = [measure("b1", "hamming", dim, all_rows[:n], all_q[:m], k, form)[0] for form in (1, 2)]
            print(f"n {n:8d} m {m:5d}: {t[0]:10.3f} / {t[1]:10.3f} ms  -> form {1 if t[0] <= t[1] else 2}", flush=True)


def context():
    print("## context (not a target): the same 256 bits as uint8 0/1 rows, EXPANN_DTYPE_U8 under L2, byte-dim 256")
    n, m, dim, k = 1_000_000, 10_000, 256, 10
    rng = np.random.default_rng(256)
    rows, queries = bits(rng, n, dim), bits(rng, m, dim)
    ms, nb = measure("b1", "hamming", dim, rows, queries, k, 0)
    print(f"b1 auto : {ms:10.3f} ms  {nb:12d} bytes of rows")
    rows8 = np.unpackbits(rows, axis=1, bitorder="little")
    q8 = np.unpackbits(queries, axis=1, bitorder="little")
    import torch
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(dim, "l2", "u8")
    t_rows, tq = torch.from_numpy(rows8).cuda(), torch.from_numpy(q8.astype(np.float32)).cuda()
    ids = torch.empty(m, k, dtype=torch.int64, device="cuda")
    dd = torch.empty(m, k, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.set_base_device(t_rows.data_ptr(), n, 0)
    ms = step_ms(eng, tq, m, k, ids, dd, st)
    print(f"u8 auto : {ms:10.3f} ms  {eng.get_stat('base_bytes'):12d} bytes of rows", flush=True)
    eng.close()


def bench(parent_lib):
    print("## C2 (bench.py --gpus 1 --steps 60 --warmup 5), five alternated rounds: the JSON lines, then ms_per_step")
    vals = {"parent": [], "this": []}
    for _ in range(5):
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
    ap.add_argument("--parts", default="throughput,crossover,context,bench")
    a = ap.parse_args()
    for part in a.parts.split(","):
        if part == "bench":
            if a.parent_lib:
                bench(a.parent_lib)
        else:
            {"throughput": throughput, "crossover": crossover, "context": context}[part]()
