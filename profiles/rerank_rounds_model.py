"""CPU model (numpy) of the int8 filter's candidate lists and of what the select re-scores, from the formulas in the
header of expann_amd/csrc/scan_gemm_i8f.hpp in real numbers -- no floors, no fp32 / fp16 rounding terms, the fp16
sampled pass replaced by exact scores.  1 M x 128 iid N(0, 1) rows, 256 queries, k = 10, s = 5.5 rms / 127,
lambda = 1.4 s / (sqrt(12) rms), tau_s = the 4th best S among every 16th row (the C2 step's speculative rank).
Prints the list length, the rows the single cut keeps (kappa <= kth(kappa + w_b) + w_q) and the rows three
two-round variants re-score (first round, T = its k-th exact score, then the rows with tau + 2 s^2 kappa <= T)."""
import numpy as np

N, D, M, K, J, FRAC = 1_000_000, 128, 256, 10, 4, 16
rng = np.random.RandomState(0)
base = rng.standard_normal((N, D)).astype(np.float32)
queries = rng.standard_normal((M, D)).astype(np.float32)

rms = float(np.sqrt(np.mean(base.astype(np.float64) ** 2)))
s = min(float(np.abs(base).max()), 5.5 * rms) / 127.0
lam = 1.4 * s / (np.sqrt(12.0) * rms)
eps = (D / 8.0 + 16.0) * 2.0 ** -24
c = 1.0 + 1.0 / lam


def quant(x):
    return np.clip(np.rint(x / s), -127, 127).astype(np.float32)


bq, qq = quant(base), quant(queries)
n_b = (base.astype(np.float64) ** 2).sum(1)
v_b = ((base - s * bq).astype(np.float64) ** 2).sum(1)
n_q = (queries.astype(np.float64) ** 2).sum(1)
v_q = ((queries - s * qq).astype(np.float64) ** 2).sum(1)
big_b = np.sqrt(n_b.max())
m_q = np.minimum(2.0 * big_b * np.sqrt(v_q), v_q / lam)
a_b = n_b * (1.0 - lam - eps) - c * v_b
w_b = (2.0 * (lam + eps) * n_b + 2.0 * c * v_b) / (2.0 * s * s)
a_q = n_q * (1.0 - lam - eps) - m_q - v_q
w_q = (2.0 * (lam + eps) * n_q + 2.0 * m_q + 2.0 * v_q) / (2.0 * s * s) + 4.0

out = {name: [] for name in ("list", "cut", "two_kappa", "two_upper", "two_k")}
for i in range(M):
    S = n_q[i] + n_b - 2.0 * (base @ queries[i]).astype(np.float64)
    L = a_q[i] + a_b - 2.0 * s * s * (bq @ qq[i]).astype(np.float64)
    tau = np.sort(S[::FRAC])[J - 1]
    cand = np.nonzero(L <= tau)[0]
    kappa = (L[cand] - tau) / (2.0 * s * s)
    upper = kappa + w_b[cand]
    out["list"].append(len(cand))
    if len(cand) <= K:
        for name in ("cut", "two_kappa", "two_upper", "two_k"):
            out[name].append(len(cand))
        continue
    out["cut"].append(int((kappa <= np.sort(upper)[K - 1] + w_q[i]).sum()))
    for name, order, r1 in (("two_kappa", kappa, 16), ("two_upper", upper, 16), ("two_k", kappa, K)):
        first = np.argsort(order, kind="stable")[:r1]
        T = np.sort(S[cand[first]])[K - 1]
        rest = np.ones(len(cand), bool)
        rest[first] = False
        out[name].append(len(first) + int((rest & (tau + 2.0 * s * s * kappa <= T)).sum()))
print(f"rms {rms:.4f}  s {s:.5f}  lambda {lam:.5f}  c {c:.1f}")
for name, what in (("list", "list length per query"), ("cut", "rows kept by the single cut"),
                   ("two_kappa", "two rounds, first round the 16 smallest kappa"),
                   ("two_upper", "two rounds, first round the 16 smallest upper bounds"),
                   ("two_k", "two rounds, first round of only k = 10 rows")):
    v = np.array(out[name])
    print(f"{what:55s} mean {v.mean():7.1f}  p99 {np.percentile(v, 99):7.1f}")
