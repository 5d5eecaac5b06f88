"""The sampled pass of the C2 shape (1 M x d128 iid fp32 rows, 10 000 queries, k = 10, L2, the planner's own choices) on
int8 and on fp16 ("i8_sample" 1 and 0): one untimed search each -- candidates per query, queries the redo pass served,
the keys of their redo lists -- and the two results compared bit for bit.  The rows and queries are bench.py's (same
generator seeds)."""
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
for i8_sample in (1, 0):
    eng = GpuBruteForceEngine(d, "l2")
    eng.store_many_vectors(base)
    eng.build()
    eng.set_option("i8_sample", i8_sample)
    eng.set_profiling(True)
    ids, dists = eng.query_k_batch(queries, k)
    prof = eng.get_profile()
    print(f"i8_sample {i8_sample}: {prof['scan_kernel']}, stat i8_sample {eng.get_stat('i8_sample')}, spec_rank "
          f"{eng.get_stat('spec_rank')}, {prof['candidates'] / m:.1f} candidates per query, redo_queries "
          f"{eng.get_stat('redo_queries')}, redo_candidates {eng.get_stat('redo_candidates')}, retries {prof['retries']}")
    res[i8_sample] = (ids, dists)
    eng.close()
assert np.array_equal(res[1][0], res[0][0]) and np.array_equal(res[1][1].view(np.uint32), res[0][1].view(np.uint32))
print("same ids and distance bits")
