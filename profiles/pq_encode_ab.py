"""Codes and codebooks from fp32 rows (pq_encode.hpp) on one MI355X.

    python profiles/pq_encode_ab.py [--parent-lib DIR] [--parts encode,train,recall,bench] > profiles/pq_encode_ab.txt

  encode  1 M Gaussian rows on the device at (dim, M) = (128, 16), (768, 64), (1 024, 128), "pq8" and "pq4":
          encode_device between two events; one warm call, then `--repeats` calls, the median with min .. max; the
          3 n dim ncent fp32 operations of THE ENCODE RULE over the step time against the packed-fp32 VALU peak without
          FMA (256 CUs x 128 operations per clock x 2.4 GHz = 78.6e12/s), and the row bytes over the step time.
  train   100 000 rows, 20 iterations, the same shapes: host clock around train_pq_codebooks (it ends in a device
          synchronise and includes the upload of the rows) at iters = 20 and iters = 0; encode = encode_device on the
          same rows; update = (t20 - t0) / 20 - encode, i.e. what an iteration takes beside its encode pass.
  recall  the set-up of profiles/pq_ab.py (20 000 Gaussian rows, 200 queries, dim 128, inner product, recall@10), the
          codebooks by expann_pq_train (20 iterations) and the codes by expann_pq_encode; informational.
  bench   --parent-lib DIR: pq_ab.py's alternated bench.py rounds, this build against DIR's."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pq_ab import SHAPES, bench, rule_scores  # noqa: E402  (profiles/ is the script's directory)

PEAK_OPS = 256 * 128 * 2.4e9  # packed fp32 add / mul per second, no FMA
README_RECALL = {16: 0.26, 32: 0.55, 64: 0.84}


def timed_encode(eng, tx, tc, n, repeats):
    import torch
    st = torch.cuda.Stream()
    ms = []
    for r in range(repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        eng.encode_device(tx.data_ptr(), n, tc.data_ptr(), st.cuda_stream)
        e1.record(st)
        e1.synchronize()
        if r:  # (call 0 warms)
            ms.append(e0.elapsed_time(e1))
    return ms


def encode(repeats):
    import torch
    from expann_amd import GpuBruteForceEngine
    n = 1_000_000
    print("## encode_device, 1 M rows; ms per call (median, min .. max)")
    for dim, M in SHAPES:
        rng = np.random.default_rng(dim)
        tx = torch.randn(n, dim, device="cuda", dtype=torch.float32)
        for dtype, ncent in (("pq8", 256), ("pq4", 16)):
            cb = rng.standard_normal((M, ncent, dim // M)).astype(np.float32)
            eng = GpuBruteForceEngine(dim, "l2", dtype, codebooks=cb)
            tc = torch.empty(n, M if ncent == 256 else M // 2, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ms = timed_encode(eng, tx, tc, n, repeats)
            eng.close()
            med = statistics.median(ms)
            ops = 3.0 * n * dim * ncent
            print(f"dim {dim:5d} M {M:3d} {dtype}: {med:9.3f} ms ({min(ms):.3f} .. {max(ms):.3f})  {ops / (med * 1e-3):.3g} fp32 op/s = "
                  f"{100 * ops / (med * 1e-3) / PEAK_OPS:.1f} % of the packed-fp32 VALU peak; rows at {n * dim * 4 / (med * 1e-3) / 1e9:.0f} GB/s",
                  flush=True)
        del tx


def train(repeats):
    import torch
    from expann_amd import GpuBruteForceEngine, train_pq_codebooks
    n, iters = 100_000, 20
    print("## train_pq_codebooks, 100 000 rows, 20 iterations; ms (median of the repeats)")
    for dim, M in SHAPES:
        rows = np.random.default_rng(dim + 1).standard_normal((n, dim)).astype(np.float32)
        tx = torch.from_numpy(rows).cuda()
        for bits, dtype, ncent in ((8, "pq8", 256), (4, "pq4", 16)):
            t = {0: [], iters: []}
            for r in range(repeats + 1):
                for it in t:
                    t0 = time.perf_counter()
                    cb = train_pq_codebooks(rows, M, bits, it)
                    if r:
                        t[it].append(1e3 * (time.perf_counter() - t0))
            eng = GpuBruteForceEngine(dim, "l2", dtype, codebooks=cb)
            tc = torch.empty(n, M if ncent == 256 else M // 2, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            enc = statistics.median(timed_encode(eng, tx, tc, n, repeats))
            eng.close()
            t20, t00 = statistics.median(t[iters]), statistics.median(t[0])
            print(f"dim {dim:5d} M {M:3d} {dtype}: whole call {t20:9.2f} ms, upload + init + download {t00:8.2f} ms; per iteration "
                  f"{(t20 - t00) / iters:8.3f} ms = encode {enc:8.3f} + update {(t20 - t00) / iters - enc:8.3f}", flush=True)


def recall():
    from expann_amd import GpuBruteForceEngine, train_pq_codebooks
    print("## recall@10 of THE PQ RULE (inner product) against the exact fp32 inner product; 20 000 Gaussian rows, 200 queries, dim 128; "
          "codebooks by expann_pq_train (20 iterations), codes by expann_pq_encode; beside it the README's figure for NumPy Lloyd codebooks")
    n, m, dim = 20_000, 200, 128
    rng = np.random.default_rng(0)
    rows, queries = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((m, dim)).astype(np.float32)
    exact = np.argsort(-(queries @ rows.T), axis=1, kind="stable")[:, :10]
    for M in (16, 32, 64):
        cb = train_pq_codebooks(rows, M, 8, 20)
        eng = GpuBruteForceEngine(dim, "ip", "pq8", codebooks=cb)
        codes = eng.encode(rows)
        eng.close()
        got = np.argsort(rule_scores(cb, codes, queries, True), axis=1, kind="stable")[:, :10]
        r = np.mean([len(set(g) & set(e)) / 10 for g, e in zip(got, exact)])
        print(f"M {M:3d} ({M} bytes per row): recall@10 {r:.3f}  (README: {README_RECALL[M]:.2f})", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parts", default="encode,train,recall,bench")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    parts = a.parts.split(",")
    if "encode" in parts:
        encode(a.repeats)
    if "train" in parts:
        train(a.repeats)
    if "recall" in parts:
        recall()
    if "bench" in parts and a.parent_lib:
        bench(a.parent_lib, a.rounds)
