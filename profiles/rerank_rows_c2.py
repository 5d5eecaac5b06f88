"""Rows the selects re-score exactly per query at the C2 shape (1 M x d128 iid fp32 rows, 10 000 queries, k = 10, L2,
the planner's own choices), with "rerank_rounds" 2 and 1: one untimed search each under "rerank_stats".  The rows and
queries are bench.py's (same generator seeds)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from expann_amd import GpuBruteForceEngine  # noqa: E402

n, d, m, k = 1_000_000, 128, 10_000, 10
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(1234)
base = torch.randn(n, d, device=dev, dtype=torch.float32, generator=g).cpu().numpy()
g.manual_seed(4321)
queries = torch.randn(m, d, device=dev, dtype=torch.float32, generator=g).cpu().numpy()
res = {}
for rounds in (2, 1):
    eng = GpuBruteForceEngine(d, "l2")
    eng.store_many_vectors(base)
    eng.build()
    eng.set_option("rerank_rounds", rounds)
    eng.set_option("rerank_stats", 1)
    eng.set_profiling(True)
    ids, dists = eng.query_k_batch(queries, k)
    prof = eng.get_profile()
    rows = eng.get_stat("rerank_rows")
    print(f"rerank_rounds {rounds}: {prof['scan_kernel']}, spec_rank {eng.get_stat('spec_rank')}, redo_queries "
          f"{eng.get_stat('redo_queries')}, {prof['candidates'] / m:.1f} candidates per query, "
          f"{rows / m:.1f} rows re-scored per query ({rows} in all), retries {prof['retries']}")
    res[rounds] = (ids, dists, rows)
    eng.close()
assert np.array_equal(res[1][0], res[2][0]) and np.array_equal(res[1][1].view(np.uint32), res[2][1].view(np.uint32))
print(f"same ids and distance bits; rows re-scored, two rounds / one: {res[2][2] / max(1, res[1][2]):.3f}")
