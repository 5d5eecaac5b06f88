#!/usr/bin/env python3
"""profiles/i8_any_dim_table.py -- 8-bit brute force at 1 M rows x 10 k queries, k = 10: ms per step, queries/s
and the share of the int8 MFMA peak, with the planner's own choice and under scan_kernel = 1 (the exact
v_dot4 scan), for uint8 L2 and int8 IP at each dim given.

  python profiles/i8_any_dim_table.py [--tag NAME] [--rows N] [--queries M] [--no-exact] DIM [DIM ...]

EXPANN_LIB selects the library (A/B against another build: run the same command once per library, alternating).
Rows and queries are made on the device from a seed (full-range uint8 / int8), searches go through
expann_search_device; a step is timed by the host clock around a search that ends in a device synchronise, after
warm-up steps of the same shape.  One JSON line per (dim, score, mode) on stdout."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from expann_amd import GpuBruteForceEngine, _lib  # noqa: E402

MFMA_I8_PEAK_TOPS = 5033.0   # (bench.py's constant: int8 MFMA = 2x the dense bf16 rate)


def timed(eng, q, m, k, ids, dd, warmup, min_steps, max_steps, min_seconds):
    for _ in range(warmup):
        eng.search_device(q.data_ptr(), m, k, ids.data_ptr(), dd.data_ptr(), 0)
    torch.cuda.synchronize()
    times = []
    t_all = time.perf_counter()
    while len(times) < max_steps and (len(times) < min_steps or time.perf_counter() - t_all < min_seconds):
        t0 = time.perf_counter()
        eng.search_device(q.data_ptr(), m, k, ids.data_ptr(), dd.data_ptr(), 0)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    times.sort()
    return times[len(times) // 2] * 1e3, times[0] * 1e3, len(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dims", type=int, nargs="+")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--no-exact", action="store_true", help="skip the scan_kernel = 1 runs")
    a = ap.parse_args()
    n, m, k = a.rows, a.queries, a.k
    for d in a.dims:
        for dtype, metric in (("u8", "l2"), ("i8", "ip")):
            g = torch.Generator(device="cuda")
            g.manual_seed(d)
            if dtype == "u8":
                base = torch.randint(0, 256, (n, d), dtype=torch.uint8, device="cuda", generator=g)
                q = torch.randint(0, 256, (m, d), device="cuda", generator=g).to(torch.float32)
            else:
                base = torch.randint(-128, 128, (n, d), dtype=torch.int8, device="cuda", generator=g)
                q = torch.randint(-128, 128, (m, d), dtype=torch.int8, device="cuda", generator=g)
            ids = torch.empty(m, k, dtype=torch.int64, device="cuda")
            dd = torch.empty(m, k, dtype=torch.float32, device="cuda")
            try:
                eng = GpuBruteForceEngine(d, metric, dtype)
            except _lib.ExpannError as e:
                print(json.dumps({"tag": a.tag, "d": d, "score": dtype + "_" + metric, "error": str(e)}), flush=True)
                continue
            eng.set_base_device(base.data_ptr(), n, 0)
            torch.cuda.synchronize()
            keep = None
            for mode in ([0] if a.no_exact else [0, 1]):
                eng.set_option("scan_kernel", mode)
                med, best, steps = timed(eng, q, m, k, ids, dd, warmup=5 if mode == 0 else 1,
                                         min_steps=10 if mode == 0 else 2, max_steps=60, min_seconds=1.5)
                eng.set_profiling(True)                 # one more step, profiled: which kernel ran, how long the scan took
                eng.search_device(q.data_ptr(), m, k, ids.data_ptr(), dd.data_ptr(), 0)
                torch.cuda.synchronize()
                prof = eng.get_profile()
                eng.set_profiling(False)
                same = None
                if keep is None:
                    keep = (ids.clone(), dd.clone())
                else:                                   # the two modes return the same bits
                    same = bool(torch.equal(keep[0], ids) and torch.equal(keep[1].view(torch.int32), dd.view(torch.int32)))
                tops = 2.0 * n * d * m / (med * 1e-3) / 1e12
                print(json.dumps({"tag": a.tag, "d": d, "score": dtype + "_" + metric, "scan_kernel_option": mode,
                                  "kernel": prof["scan_kernel"], "ms_per_step": round(med, 3), "ms_best": round(best, 3),
                                  "steps": steps, "queries_per_s": round(m / (med * 1e-3)),
                                  "tops_end_to_end": round(tops, 1),
                                  "frac_i8_mfma_peak": round(tops / MFMA_I8_PEAK_TOPS, 4),
                                  "scan_ms_profiled": round(prof["scan_ms"], 3), "retries": prof["retries"],
                                  "candidates_per_query": round(prof["candidates"] / m, 1),
                                  "same_bits_as_auto": same}), flush=True)
            eng.close()
            del base, q


if __name__ == "__main__":
    main()
