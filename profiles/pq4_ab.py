"""4-bit product-quantised rows (EXPANN_DTYPE_PQ4, scan_pq4.hpp) on one MI355X, and their ranking on
the CPU.

    python profiles/pq4_ab.py [--parent-lib DIR] [--parts recall,throughput,bench] > profiles/pq4_ab.txt

  recall      CPU only: 20 000 Gaussian rows, 200 queries, dim 128; codebooks of 16 centroids from 8 Lloyd iterations
              per sub-quantiser in NumPy; recall@10 (inner product) against the exact fp32 inner product at 16 / 32 / 64
              bytes per row, of THE PQ4 RULE and of the same codes scored with unquantised fp32 tables -- the loss of
              step 4 apart from the loss of the 4-bit codebooks.
  throughput  1 M rows, L2, k = 10, with 10 000 queries and with 1: a "pq4" index, a "pq8" index of equal bytes per
              row and an "i4" index of dim 16 M (the same MFMA work: K = 16 M) in one process, alternated; device time
              between two events around a step (the whole search: tables, thresholds, scans, selects); one warm step
              each, then `--repeats` alternated steps, the median with min .. max; the share of the int8 MFMA peak by
              the STEP time with K = 16 M (an end-to-end figure, not a kernel's share).
  bench       --parent-lib DIR: `bench.py --gpus 1 --steps 60 --warmup 5` on DIR's libexpann_hip.so and on this
              build, alternated rounds; this build's median against the other's min..max."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
I8_MFMA_PEAK = 5.0e15  # int8 operations per second (dense, 2.4 GHz), as DESIGN.md 4.8 counts them
SHAPES = ((128, 32, 16), (768, 128, 64), (1024, 256, 128))  # dim, M of "pq4", M of "pq8": equal bytes per row


def tables_ip(cb, queries):
    M, _, dsub = cb.shape
    q = queries.reshape(len(queries), M, 1, dsub)
    T = np.zeros((len(queries), M, cb.shape[1]), np.float32)
    for j in range(dsub):
        T = T + q[..., j] * cb[None, :, :, j]
    return np.float32(0) - T


def gather(T, codes):
    S = np.zeros((T.shape[0], len(codes)), T.dtype)
    for i in range(T.shape[1]):
        S = S + T[:, i, codes[:, i]]
    return S


def rule_scores(T):
    """steps 2-4 of THE PQ4 RULE: the byte tables (the bias and the step do not change a query's ranking)"""
    F = np.float32
    lo = T.min(axis=2)
    span = (T.max(axis=2) - lo).max(axis=1)
    r = (F(255) / span).astype(F)
    return np.minimum(F(255), np.rint((T - lo[:, :, None]) * r[:, None, None])).astype(np.int64)


def recall():
    print("## CPU: recall@10 (inner product) against the exact fp32 inner product; 20 000 Gaussian rows, 200 queries, dim 128; "
          "16 centroids per sub-quantiser from 8 Lloyd iterations.  (profiles/pq_ab.txt, 256 centroids: 0.26 / 0.55 / 0.84 at "
          "16 / 32 / 64 bytes per row)")
    n, m, dim = 20_000, 200, 128
    rng = np.random.default_rng(0)
    rows, queries = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((m, dim)).astype(np.float32)
    exact = np.argsort(-(queries @ rows.T), axis=1, kind="stable")[:, :10]
    for M in (32, 64, 128):
        dsub = dim // M
        cb = np.empty((M, 16, dsub), np.float32)
        codes = np.empty((n, M), np.uint8)
        for i in range(M):
            x = rows[:, i * dsub:(i + 1) * dsub]
            c = x[rng.choice(n, 16, replace=False)].copy()
            for it in range(9):
                a = ((x * x).sum(1)[:, None] - 2 * x @ c.T + (c * c).sum(1)[None]).argmin(1)
                if it == 8:
                    break
                for j in range(16):
                    if (a == j).any():
                        c[j] = x[a == j].mean(0)
            cb[i], codes[:, i] = c, a
        T = tables_ip(cb, queries)
        out = []
        for S in (gather(rule_scores(T), codes), gather(T, codes)):
            got = np.argsort(S, axis=1, kind="stable")[:, :10]
            out.append(np.mean([len(set(g) & set(e)) / 10 for g, e in zip(got, exact)]))
        print(f"M {M:3d} ({M // 2} bytes per row): recall@10 {out[0]:.3f} by THE PQ4 RULE, {out[1]:.3f} with unquantised fp32 tables", flush=True)


def throughput(repeats):
    import torch
    from expann_amd import GpuBruteForceEngine
    print("## 1 M rows, L2, k = 10; ms per step (median, min .. max) of alternated steps")
    n, k = 1_000_000, 10
    st = torch.cuda.Stream()
    for dim, M4, M8 in SHAPES:
        rng = np.random.default_rng(dim)
        cb4 = rng.standard_normal((M4, 16, dim // M4)).astype(np.float32)
        cb8 = rng.standard_normal((M8, 256, dim // M8)).astype(np.float32)
        rows = {"pq4": torch.from_numpy(rng.integers(0, 256, (n, M4 // 2), dtype=np.uint8)).cuda(),
                "pq8": torch.from_numpy(rng.integers(0, 256, (n, M8), dtype=np.uint8)).cuda(),
                "i4": torch.from_numpy(rng.integers(0, 256, (n, 8 * M4), dtype=np.uint8)).cuda()}
        engines = {"pq4": GpuBruteForceEngine(dim, "l2", "pq4", codebooks=cb4), "pq8": GpuBruteForceEngine(dim, "l2", "pq8", codebooks=cb8),
                   "i4": GpuBruteForceEngine(16 * M4, "l2", "i4")}
        for kind in engines:
            engines[kind].set_base_device(rows[kind].data_ptr(), n, 0)
        for m in (10_000, 1):
            q = torch.from_numpy(rng.standard_normal((m, dim)).astype(np.float32)).cuda()
            tq = {"pq4": q, "pq8": q, "i4": torch.from_numpy(rng.integers(-128, 128, (m, 16 * M4), dtype=np.int8)).cuda()}
            out = {kind: (torch.empty(m, k, dtype=torch.int64, device="cuda"), torch.empty(m, k, dtype=torch.float32, device="cuda"))
                   for kind in engines}
            torch.cuda.synchronize()

            def step(kind):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                engines[kind].search_device(tq[kind].data_ptr(), m, k, out[kind][0].data_ptr(), out[kind][1].data_ptr(), st.cuda_stream)
                e1.record(st)
                e1.synchronize()
                return e0.elapsed_time(e1)
            ms = {kind: [] for kind in engines}
            for r in range(repeats + 1):
                for kind in engines:
                    t = step(kind)
                    if r:  # (round 0 warms all three)
                        ms[kind].append(t)
            for kind, M in (("pq4", M4), ("pq8", M8), ("i4", M4)):
                med = statistics.median(ms[kind])
                share = "" if kind == "pq8" else f"  {100 * 2.0 * m * n * 16 * M4 / (med * 1e-3) / I8_MFMA_PEAK:5.1f} % of the int8 MFMA peak by the step time (K = {16 * M4})"
                prof = engines[kind].get_profile()
                print(f"dim {dim:5d} m {m:6d} {kind:>3} M {M:3d}: {med:10.3f} ms ({min(ms[kind]):.3f} .. {max(ms[kind]):.3f})  "
                      f"{engines[kind].get_stat('base_bytes'):12d} bytes of rows  {prof['scan_kernel']}, {prof['levels']} levels{share}", flush=True)
            print(f"dim {dim:5d} m {m:6d}: pq4 / pq8 step time {statistics.median(ms['pq4']) / statistics.median(ms['pq8']):.3f}; "
                  f"pq4 / i4 {statistics.median(ms['pq4']) / statistics.median(ms['i4']):.3f}", flush=True)
        for e in engines.values():
            e.close()
        del rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parts", default="recall,throughput,bench")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    parts = a.parts.split(",")
    if "recall" in parts:
        recall()
    if "throughput" in parts:
        throughput(a.repeats)
    if "bench" in parts and a.parent_lib:
        from pq_ab import bench  # (the same alternation as the PQ8 record's)
        bench(a.parent_lib, a.rounds)
