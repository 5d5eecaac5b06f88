#!/usr/bin/env python3
"""profiles/i8_sample_model.py -- numpy model (CPU, no device) of the thresholds a speculating int8-filter search takes
from its sampled pass (scan_gemm_i8f.hpp, "Sampled pass on int8").  iid N(0, 1) rows, N = 266 240,
d = 128, 2 048 queries, k = 10, j = 4; the sample is the library's: 64-row tiles at stride 16, classes (chunk, row mod
32).  For thresholds from (a) the exact scores of the sampled rows (what the fp16 pass gives up to its small slack),
(b) the int8 interval's centre  N_q + N_b - 2 s^2 q~.b~  (cb = rint(N_b / 2s^2), as the kernel sees it) and (c) the
int8 upper bound row by row, it prints the share of queries whose k-th best row lies above tau_s (they go to the redo
pass) and the rows with L <= tau_s per query (the candidate lists).  Last line: the PROVEN tau from the k-th largest
class maximum of (b) plus the largest half width of the rows the pass sees -- valid for every query?  and the lists it would give.
Output: profiles/i8_sample_model.txt."""
import numpy as np

N, D, M, K, J = 266_240, 128, 2048, 10, 4
rng = np.random.RandomState(20261)
base = rng.standard_normal((N, D)).astype(np.float32)
queries = rng.standard_normal((M, D)).astype(np.float32)

# the header's terms, fp64
b64, q64 = base.astype(np.float64), queries.astype(np.float64)
rms = float(np.sqrt(np.mean(b64 ** 2)))
s = float(np.float32(min(float(np.abs(base).max()), 5.5 * rms)) / np.float32(127.0))
lam = 1.4 * s / (np.sqrt(12.0) * rms)
eps = (D / 8.0 + 16.0) * 2.0 ** -24
c = 1.0 + 1.0 / lam
two_s2 = 2.0 * s * s
bq = np.clip(np.rint(base * np.float32(1.0 / s)), -127, 127)
qq = np.clip(np.rint(queries * np.float32(1.0 / s)), -127, 127)
n_b, v_b = (b64 ** 2).sum(1), ((b64 - s * bq) ** 2).sum(1)
n_q, v_q = (q64 ** 2).sum(1), ((q64 - s * qq) ** 2).sum(1)
m_q = np.minimum(2.0 * np.sqrt(n_b.max()) * np.sqrt(v_q), v_q / lam)
a_b, w_b = n_b * (1 - lam - eps) - c * v_b, 2 * (lam + eps) * n_b + 2 * c * v_b
a_q, w_q = n_q * (1 - lam - eps) - m_q - v_q, 2 * (lam + eps) * n_q + 2 * m_q + 2 * v_q
cb = np.rint(n_b / two_s2)
# rows the int8 pass leaves out (cb = kI8fCbNone): wider than twice a row of rms norm with unclipped components
w_cap = 2.0 * (2 * (lam + eps) * D * rms * rms + 2 * c * D * s * s / 12.0)
seen = w_b <= w_cap
bqf, qqf = bq.astype(np.float32), qq.astype(np.float32)   # (|q~.b~| < 2^21: exact in fp32)


def blocks(step=16384):
    for r0 in range(0, N, step):
        yield r0, min(N, r0 + step)


def exact(r0, r1):   # [M][rows] scores
    return n_q[:, None] + n_b[None, r0:r1] - 2.0 * (queries @ base[r0:r1].T).astype(np.float64)


def lower(r0, r1):   # [M][rows] L
    return a_q[:, None] + a_b[None, r0:r1] - two_s2 * (qqf @ bqf[r0:r1].T).astype(np.float64)


# the k-th smallest exact score of the whole index per query
best = np.full((M, K), np.inf)
for r0, r1 in blocks():
    best = np.partition(np.concatenate([best, exact(r0, r1)], 1), K - 1, 1)[:, :K]
s_k = best.max(1)

nt = N // 64
t_sel = nt // 16
rows_of_tile = lambda t: np.arange(64) + (t * (nt // t_sel)) * 64


def class_minima(chunks, score):   # score(rows) -> [M][len(rows)]; -> [M][chunks * 32] class minima
    tpb = -(-t_sel // chunks)
    chunks = -(-t_sel // tpb)
    out = np.full((M, chunks, 32), np.inf)
    for t in range(t_sel):
        r = rows_of_tile(t)
        v = score(r).reshape(M, 2, 32).min(1)
        out[:, t // tpb] = np.minimum(out[:, t // tpb], v)
    return out.reshape(M, -1)


sc_exact = lambda r: n_q[:, None] + n_b[None, r] - 2.0 * (queries @ base[r].T).astype(np.float64)
g_of = lambda r: (qqf @ bqf[r].T).astype(np.float64) - np.where(seen[r], cb[r], 2.0 ** 30)[None, :]
sc_centre = lambda r: n_q[:, None] - two_s2 * g_of(r)
sc_upper = lambda r: (a_q + w_q)[:, None] + (a_b + w_b)[None, r] - two_s2 * (qqf @ bqf[r].T).astype(np.float64)

cases = [("exact scores of the sample", 384, sc_exact), ("int8 centre", 384, sc_centre), ("int8 centre", 608, sc_centre),
         ("int8 upper bound, row by row", 608, sc_upper)]
taus = []
for name, classes, fn in cases:
    taus.append(np.sort(class_minima(classes // 32, fn), 1)[:, J - 1])
# the proven tau of the int8 pass: the k-th class maximum of g (608 classes) and the largest half width of the rows the pass sees
g_k = -np.sort(-(-(class_minima(19, lambda r: -g_of(r)))), 1)[:, K - 1]   # k-th largest g
tau_proven = a_q + w_q + two_s2 * (0.5 - g_k) + 0.5 * w_b[seen].max()
taus.append(tau_proven)
counts = np.zeros((len(taus), M), np.int64)
for r0, r1 in blocks():
    low = lower(r0, r1)
    for i, t in enumerate(taus):
        counts[i] += (low <= t[:, None]).sum(1)

lines = [f"N {N} d {D} queries {M} k {K} j {J}: s {s:.5f} lambda {lam:.5f}, mean interval width W_q + W_b "
         f"{w_q.mean() + w_b.mean():.2f}, sd of (centre - exact) over the sample "
         f"{np.std(sc_centre(rows_of_tile(7)) - sc_exact(rows_of_tile(7))):.3f}",
         "thresholds from | classes | queries failing | rows with L <= tau_s per query, mean / max"]
for i, (name, classes, _) in enumerate(cases):
    lines.append(f"{name} | {classes} | {100.0 * (s_k > taus[i]).mean():.2f} % | {counts[i].mean():.1f} / {counts[i].max()}")
lines.append(f"rows left out of the int8 pass (W_b > {w_cap:.2f}): {int((~seen).sum())}; W_b mean {w_b.mean():.2f}, max {w_b.max():.2f}, max of the rows seen {w_b[seen].max():.2f}")
lines.append(f"proven tau from the k-th class maximum of g (608 classes) + w_b max / 2: valid for "
             f"{int((tau_proven >= s_k).sum())} of {M} queries; rows with L <= tau per query {counts[-1].mean():.1f} / {counts[-1].max()}")
print("\n".join(lines))
