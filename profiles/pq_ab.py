"""Product-quantised rows (EXPANN_DTYPE_PQ8, scan_pq.hpp) on one MI355X, and their ranking on the CPU.

    python profiles/pq_ab.py [--parent-lib DIR] [--parts recall,bound,throughput,bench] > profiles/pq_ab.txt

  recall      CPU only: 20 000 Gaussian rows, 200 queries, dim 128; codebooks from a few Lloyd iterations per
              sub-quantiser in NumPy; recall@10 of THE PQ RULE (inner product) against the exact fp32 inner product.
  bound       CPU only: the LDS-gather bound -- CUs x table floats per clock x clock -- and the bank-conflict factor
              of random codes on 64 banks at each TQ, from a Monte-Carlo MODEL of the access (stated with it).
  throughput  1 M rows, L2, k = 10, at (dim, M) = (128, 16), (768, 64), (1 024, 128), with 10 000 queries and with 1:
              a "pq8" index and an "i8" index over the decoded rows (scaled to +-127 and rounded) in one process,
              alternated; device time between two events around a step (the whole search: thresholds, scans,
              selects); one warm step each, then `--repeats` alternated steps, the median with min .. max; the row
              bytes of both; table lookups per second against the bound; the prologue's share BY THE ARITHMETIC of
              bf_plan.hpp (prologue = 384 dsub rows' worth of VALU work against the rows of a workgroup), not measured.
  bench       --parent-lib DIR: `bench.py --gpus 1 --steps 60 --warmup 5` on DIR's libexpann_hip.so and on this
              build, alternated rounds; this build's median against the other's min..max."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CUS, CLOCK, FLOATS_PER_CLK = 256, 2.4e9, 64  # LDS: 64 banks x 4 bytes per clock per CU
SHAPES = ((128, 16), (768, 64), (1024, 128))


def tile_class(M):
    return max(t for t in (1, 2, 4, 8) if t == 1 or t * M * 1024 <= 128 * 1024)


def conflict_factor(tq, trials=4000, seed=0):
    """MODEL: a ds_read of w bytes per lane is served in passes of 256 / w lanes (b128: 16, b64: 32, b32: 64); a pass
    takes as many clocks as the busiest bank has distinct addresses.  Entry c of a sub-quantiser sits at byte
    c * 4 * TQ; at TQ = 8 an entry is two b128 reads, each of which can fall on half of the sixteen 16-byte columns."""
    rng = np.random.default_rng(seed)
    width = min(4 * tq, 16)
    lanes, cols = 256 // width, 256 // width
    total = 0
    for _ in range(trials):
        entry = np.unique(rng.integers(0, 256, lanes))  # (equal addresses are one broadcast)
        col = (entry * 4 * tq // width) % cols
        total += np.bincount(col, minlength=cols).max()
    return total / trials


def bound():
    print("## LDS-gather bound: table floats per second = CUs x 64 floats per clock x clock = "
          f"{CUS} x {FLOATS_PER_CLK} x {CLOCK / 1e9} GHz = {CUS * FLOATS_PER_CLK * CLOCK:.3g} (row, code, query) lookups/s, divided by "
          "the conflict factor below (a model of random codes on 64 banks, not a measurement)")
    f = {tq: conflict_factor(tq) for tq in (1, 2, 4, 8)}
    for tq in f:
        print(f"TQ {tq}: passes of {256 // min(4 * tq, 16)} lanes, conflict factor {f[tq]:.2f} -> {CUS * FLOATS_PER_CLK * CLOCK / f[tq]:.3g} lookups/s")
    return f


def rule_scores(cb, codes, queries, ip):
    M, _, dsub = cb.shape
    q = queries.reshape(len(queries), M, 1, dsub)
    T = np.zeros((len(queries), M, 256), np.float32)
    for j in range(dsub):
        T = T + q[..., j] * cb[None, :, :, j] if ip else T + (q[..., j] - cb[None, :, :, j]) * (q[..., j] - cb[None, :, :, j])
    S = T[:, 0, codes[:, 0]]
    for i in range(1, M):
        S = S + T[:, i, codes[:, i]]
    return np.float32(0) - S if ip else S


def recall():
    print("## CPU: recall@10 of THE PQ RULE (inner product) against the exact fp32 inner product; 20 000 Gaussian rows, 200 "
          "queries, dim 128; codebooks from 8 Lloyd iterations per sub-quantiser (README: sign bits 0.21 asymmetric, 0.09 Hamming)")
    n, m, dim = 20_000, 200, 128
    rng = np.random.default_rng(0)
    rows, queries = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((m, dim)).astype(np.float32)
    exact = np.argsort(-(queries @ rows.T), axis=1, kind="stable")[:, :10]
    for M in (16, 32, 64):
        dsub = dim // M
        cb = np.empty((M, 256, dsub), np.float32)
        codes = np.empty((n, M), np.uint8)
        for i in range(M):
            x = rows[:, i * dsub:(i + 1) * dsub]
            c = x[rng.choice(n, 256, replace=False)].copy()
            for it in range(9):
                a = ((x * x).sum(1)[:, None] - 2 * x @ c.T + (c * c).sum(1)[None]).argmin(1)
                if it == 8:
                    break
                for j in range(256):
                    if (a == j).any():
                        c[j] = x[a == j].mean(0)
            cb[i], codes[:, i] = c, a
        got = np.argsort(rule_scores(cb, codes, queries, True), axis=1, kind="stable")[:, :10]
        r = np.mean([len(set(g) & set(e)) / 10 for g, e in zip(got, exact)])
        print(f"M {M:3d} ({M} bytes per row, {dim * 4 // M} x smaller than fp32): recall@10 {r:.3f}", flush=True)


def throughput(repeats, factor):
    import torch
    from expann_amd import GpuBruteForceEngine
    print("## 1 M rows, L2, k = 10; ms per step (median, min .. max) of alternated steps")
    n, k = 1_000_000, 10
    st = torch.cuda.Stream()
    for dim, M in SHAPES:
        dsub = dim // M
        rng = np.random.default_rng(dim)
        cb = rng.standard_normal((M, 256, dsub)).astype(np.float32)
        codes = torch.from_numpy(rng.integers(0, 256, (n, M), dtype=np.uint8)).cuda()
        cb_t = torch.from_numpy(cb).cuda()
        scale = 127.0 / float(np.abs(cb).max())
        dec = torch.empty(n, dim, dtype=torch.int8, device="cuda")
        for i in range(M):  # the decoded rows, scaled to +-127 and rounded
            dec[:, i * dsub:(i + 1) * dsub] = torch.round(cb_t[i][codes[:, i].long()] * scale).to(torch.int8)
        engines = {"pq8": GpuBruteForceEngine(dim, "l2", "pq8", codebooks=cb), "i8": GpuBruteForceEngine(dim, "l2", "i8")}
        engines["pq8"].set_base_device(codes.data_ptr(), n, 0)
        engines["i8"].set_base_device(dec.data_ptr(), n, 0)
        for m in (10_000, 1):
            q = rng.standard_normal((m, dim)).astype(np.float32)
            tq = {"pq8": torch.from_numpy(q).cuda(),
                  "i8": torch.from_numpy(np.clip(np.round(q * scale), -127, 127).astype(np.int8)).cuda()}
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
                    if r:  # (round 0 warms both)
                        ms[kind].append(t)
            for kind in engines:
                print(f"dim {dim:5d} M {M:3d} m {m:6d} {kind:>3}: {statistics.median(ms[kind]):10.3f} ms ({min(ms[kind]):.3f} .. "
                      f"{max(ms[kind]):.3f})  {engines[kind].get_stat('base_bytes'):12d} bytes of rows", flush=True)
            prof = engines["pq8"].get_profile()
            tile = int(prof["query_tile"])
            med = statistics.median(ms["pq8"])
            # the arithmetic of plan_pq_chunks for the full scan: 256 CUs x the workgroups whose tables fit 160 KB
            slots = CUS * max(1, min(8, 160 * 1024 // (tile * M * 1024)))
            qtiles = -(-m // tile)
            chunks = min(max(n // (3840 * dsub), -(-slots // qtiles)), max(1, n // 16 // 16))
            rows_wg = n / chunks
            print(f"dim {dim:5d} M {M:3d} m {m:6d}: {prof['scan_kernel']}, {prof['levels']} levels; {m * n * M / (med * 1e-3):.3g} lookups/s "
                  f"by the step time = {100 * m * n * M / (med * 1e-3) / (CUS * FLOATS_PER_CLK * CLOCK / factor[tile]):.1f} % of the bound at conflict "
                  f"factor {factor[tile]:.2f} ({100 * (qtiles * tile) * n * M / (med * 1e-3) / (CUS * FLOATS_PER_CLK * CLOCK / factor[tile]):.1f} % "
                  f"counting the tile's empty slots); prologue share by the arithmetic: {384 * dsub} / ({384 * dsub} + "
                  f"{rows_wg:.0f} rows per workgroup) = {100 * 384 * dsub / (384 * dsub + rows_wg):.1f} %", flush=True)
        for e in engines.values():
            e.close()
        del codes, dec


def bench(parent_lib, rounds):
    print(f"## C2 (bench.py --gpus 1 --steps 60 --warmup 5), {rounds} alternated rounds: ms_per_step")
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
            vals[name].append(line["ms_per_step"])
            print(name, line["ms_per_step"], line["roofline"]["kernel"], flush=True)
    p, t = vals["parent"], vals["this"]
    print(f"ms_per_step: parent min {min(p)} max {max(p)}; this build median {statistics.median(t)} "
          f"-> {'inside' if min(p) <= statistics.median(t) <= max(p) else 'OUTSIDE'} the parent's spread")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parts", default="recall,bound,throughput,bench")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    parts = a.parts.split(",")
    factor = bound() if ("bound" in parts or "throughput" in parts) else None
    if "recall" in parts:
        recall()
    if "throughput" in parts:
        throughput(a.repeats, factor)
    if "bench" in parts and a.parent_lib:
        bench(a.parent_lib, a.rounds)
