"""Host model (float64 numpy, no GPU) of the int8 filter's analysis -- the header comment of
expann_amd/csrc/scan_gemm_i8f.hpp restated formula by formula -- and the adversarial data built on it
(tests/test_i8f_model.py on the CPU, tests/test_gpu_i8_filter_adversarial.py on the GPU).

Names follow the header: one scale s per index, x~ = clamp(rint(x / s)), e = x - s x~, N = |x|^2, V = |e|^2,
P = s^2 q~.b~, and for every pair   L <= S <= L + W_q + W_b   with S the reference-order fp32 score."""
import numpy as np

U24 = 2.0 ** -24
BP_MIN, BP_MAX = -(1 << 29) - (1 << 22), (1 << 29) - (1 << 22)
THP_LIM = 1 << 29
CB_MAX = 1 << 29
CLIP_RMS = 5.5          # s = min(max |x|, 5.5 rms) / 127
TRIM_ENERGY = 1.0 / 16  # ... rms of the components within the clip when those hold less than this of the energy


def f32_down(x):
    """float64 -> float32 rounded toward -inf"""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def f32_up(x):
    """float64 -> float32 rounded toward +inf"""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def index_scale(base):
    """(s, rms) as the header's "Quantisation" paragraph states them: s = min(max |x|, 5.5 rms) / 127 in fp32"""
    x = np.asarray(base, dtype=np.float64)
    sumsq = float((x * x).sum())
    rms = np.sqrt(sumsq / x.size)
    maxabs = float(np.abs(x).max())
    clip = np.float32(min(maxabs, CLIP_RMS * rms))
    if maxabs > clip:
        inside = np.abs(x) <= float(clip)
        sumsq_in = float((x[inside] ** 2).sum())
        if inside.any() and sumsq_in < TRIM_ENERGY * sumsq:
            rms = np.sqrt(sumsq_in / int(inside.sum()))
            clip = np.float32(min(maxabs, CLIP_RMS * rms))
    return float(clip / np.float32(127.0)), float(np.float32(rms))


class I8fModel:
    """the per-index constants and the per-row / per-query / per-pair terms of the analysis"""

    def __init__(self, base, s=None, rms=None):
        base = np.asarray(base, dtype=np.float32)
        self.d = d = base.shape[1]
        if s is None:
            s, rms = index_scale(base)
        self.s, self.rms = float(s), float(rms)
        self.two_s2 = 2.0 * self.s * self.s
        self.lam = 1.4 * self.s / (np.sqrt(12.0) * self.rms) if self.rms > 0 else 0.01
        self.c = 1.0 + 1.0 / self.lam
        self.eps = (d / 8.0 + 16.0) * U24
        self.eta = (d + 16.0) * 2.0 ** -149
        self.lo = 1.0 - self.lam - self.eps
        self.wn = 2.0 * (self.lam + self.eps)
        # B >= max_b |b|: from the largest fp32 reference-order ||b||^2, 2^-16 above its rounding
        nb = (base.astype(np.float64) ** 2).sum(1)
        self.B = float(np.sqrt(nb.max() * (1.0 + 2.0 ** -16)) * (1.0 + 2.0 ** -40))
        self.w_cap = 2.0 * (self.wn * d * self.rms ** 2 + 2.0 * self.c * d * self.s ** 2 / 12.0) / self.two_s2
        self.rows = self._side(base, query=False)

    def quant(self, x):
        return np.clip(np.rint(np.asarray(x, dtype=np.float64) / self.s), -127, 127)

    def _side(self, x, query):
        x = np.asarray(x, dtype=np.float64)
        t = self.quant(x)
        e = x - self.s * t
        N, V = (x * x).sum(1), (e * e).sum(1)
        n_lo, n_up, v_up = N * (1.0 - 2.0 ** -40), N * (1.0 + 2.0 ** -40), V * (1.0 + 2.0 ** -40)
        out = {"t": t, "N": N, "V": V}
        if query:
            m2b = 2.0 * self.B * np.sqrt(v_up) * (1.0 + 2.0 ** -40)
            mvl = v_up / self.lam
            out["M_branch_B"] = m2b < mvl                      # M_q takes its 2 B |e_q| branch
            M = np.minimum(m2b, mvl) * (1.0 + 2.0 ** -40)
            out["M"] = M
            out["A"] = n_lo * self.lo - M - v_up
            out["W"] = self.wn * n_up + 2.0 * M + 2.0 * v_up + 2.0 * self.eta
            # the stored query terms: A_q - eta rounded down, W_q rounded up (fp32)
            out["aq"] = f32_down((out["A"] - self.eta) * (1.0 - 2.0 ** -40))
            out["wq"] = f32_up(out["W"] * (1.0 + 2.0 ** -40))
        else:
            out["A"] = n_lo * self.lo - self.c * v_up
            out["W"] = self.wn * n_up + 2.0 * self.c * v_up
            xb = out["A"] / self.two_s2
            xl = xb - (np.abs(xb) * 2.0 ** -30 + 2.0 ** -10)
            ok = (xl >= BP_MIN) & (xl <= BP_MAX)
            out["bp"] = np.where(ok, np.floor(xl), np.where(xl > 0, BP_MAX, BP_MIN)).astype(np.int64)
            out["clamped"] = ~ok
            w = f32_up(out["W"] / self.two_s2 * (1.0 + 2.0 ** -40)).astype(np.float64)
            out["w"] = np.where(ok, w, np.inf)                  # row_w
            xc = np.rint(N / self.two_s2)
            out["seen"] = ok & (xc <= CB_MAX) & (out["w"] <= self.w_cap)   # rows the int8 sampled pass can see
            out["cb"] = xc
        return out

    def queries(self, q):
        return self._side(np.asarray(q, dtype=np.float32), query=True)

    def pairs(self, Q, rows=None):
        """P, L, width and centre of the interval [L, L + W_q + W_b] of every (query, row) pair; rows: an index
        array or None for all"""
        R = self.rows
        sel = slice(None) if rows is None else rows
        dot = Q["t"] @ R["t"][sel].T                            # q~.b~: exact integers below 2^21
        P = self.s * self.s * dot
        L = Q["A"][:, None] + R["A"][sel][None, :] - 2.0 * P - self.eta
        width = Q["W"][:, None] + R["W"][sel][None, :]
        return {"dot": dot, "P": P, "L": L, "width": width, "centre": L + 0.5 * width}

    def wb_max(self):
        seen = self.rows["seen"]
        return float(self.rows["w"][seen].max()) if seen.any() else 0.0

    # ---- "Integer test" / "Keys and pruning" ----------------------------------------------------------------
    def thp(self, Q, tau):
        xq = (Q["aq"].astype(np.float64) - np.asarray(tau, dtype=np.float64)) / self.two_s2
        xl = xq - (np.abs(xq) * 2.0 ** -30 + 2.0 ** -10)
        ok = (xl >= -THP_LIM) & (xl <= THP_LIM)
        return np.where(ok, -np.floor(xl), np.where(xl > 0, -THP_LIM, THP_LIM)), ok

    def kappa(self, Q, tau, rows=None):
        """kappa = bp - thp - q~.b~ of every pair for the fp32 thresholds tau[q] (-inf: a clamped bp)"""
        sel = slice(None) if rows is None else rows
        thp, _ = self.thp(Q, tau)
        dot = Q["t"] @ self.rows["t"][sel].T
        kap = self.rows["bp"][sel][None, :].astype(np.float64) - thp[:, None] - dot
        return np.where(self.rows["clamped"][sel][None, :], -np.inf, kap)

    def w_q(self, Q, tau):
        """the select's query width: W_q / 2s^2 + 4 + ulp(aq) / 2s^2 (+inf when thp is clamped)"""
        _, ok = self.thp(Q, tau)
        ulp = np.abs(Q["aq"].astype(np.float64)) * 2.0 ** -23 + 2.0 ** -149
        return np.where(ok, (Q["wq"].astype(np.float64) + ulp) / self.two_s2 * (1.0 + 2.0 ** -40) + 4.0, np.inf)

    def cut_two_rounds(self, T, tau):
        """x = (T - tau_q) / 2s^2 with its rounding margin: a candidate with kappa > x is dropped"""
        x = (np.asarray(T, dtype=np.float64) - np.asarray(tau, dtype=np.float64)) / self.two_s2
        return f32_up(x + np.abs(x) * 2.0 ** -40 + 2.0 ** -10).astype(np.float64)

    # ---- "Sampled pass on int8" -----------------------------------------------------------------------------
    def g(self, Q, rows=None):
        sel = slice(None) if rows is None else rows
        return Q["t"] @ self.rows["t"][sel].T - self.rows["cb"][sel][None, :]

    def proven_tau(self, Q, g_k, wb_max=None):
        """S <= aq + ulp(aq) + W_q + 2s^2 (1/2 + 2^-9 - g_k + wb_max / 2), rounded up to fp32"""
        wb_max = self.wb_max() if wb_max is None else wb_max
        aq = Q["aq"].astype(np.float64)
        ulp = np.abs(aq) * 2.0 ** -23 + 2.0 ** -149
        # (a factor 1 + 2^-40 on every positive term covers the fp64 roundings)
        terms = [aq, ulp, Q["wq"].astype(np.float64), self.two_s2 * (0.5 + 2.0 ** -9 + 0.5 * wb_max),
                 -self.two_s2 * np.asarray(g_k, dtype=np.float64)]
        return f32_up(sum(np.where(t > 0, t * (1.0 + 2.0 ** -40), t) for t in terms))


def all_scores(oracle, base, queries):
    """S of every pair: the oracle's reference-order fp32 L2 score ([m][n] float32)"""
    n = base.shape[0]
    ids = np.arange(n, dtype=np.uint64)
    out = np.empty((queries.shape[0], n), dtype=np.float32)
    for i in range(queries.shape[0]):
        kept, sc = oracle.filter_by_score(base, queries[i], ids, np.float32(np.inf), oracle.METRIC_L2_F32)
        assert len(kept) == n
        out[i] = sc
    return out


# ---- the constructions -------------------------------------------------------------------------------------
# Every index: N(0, 1) x 32 s far rows clamped to 126 s, one planted component of 127 s exactly, so that
# max |x| = 127 * 2^e <= 5.5 rms and the index takes s = 2^e exactly (no clip, no trim).
D, K = 128, 10
E = -5                     # s = 2^-5: far rows of rms ~1
DELTA = 2.0 ** -8          # distance from the rounding midpoint, in cells
N_DROP = 32768 + 40        # just above the form's minimum of 2 * 256 * 64 rows, off the 64-row tile
N_SAMPLE = 262_144 + 4_096  # the smallest index the int8 sampled pass serves


def sampled_tile_stride(n):
    """rows from one sampled 64-row tile to the next (sampled_pass_f16, expann_hip.hip; both the fp16 and the int8
    pass): of nt tiles the pass reads t_sel = max(256, nt / 16) (sample_frac_for: 16 at k = 10, an index this small),
    one every nt / t_sel, when 2 t_sel <= nt.  A class is (chunk of consecutive sampled tiles, row mod 32)."""
    nt = (n + 63) // 64
    t_sel = max(256, nt // 16)
    assert 2 * t_sel <= nt
    return 64 * (nt // t_sel)




def _far_rows(rng, n, s):
    base = rng.standard_normal((n, D)) * (32.0 * s)
    base = np.clip(base, -126.0 * s, 126.0 * s).astype(np.float32)
    return base


def _t_for_lambda(base, s):
    """t with |e| / |q| = (1/2) / (t + 1/2) nearest the index's lambda (AM-GM tight)"""
    rms = np.sqrt((base.astype(np.float64) ** 2).mean())
    lam = 1.4 * s / (np.sqrt(12.0) * rms)
    return int(round(0.5 / lam - 0.5))


def _midpoint_queries(rng, m, s, t, side):
    """|q_i| = s (t + 1/2 + side * DELTA): side -1 rounds to t (error parallel to q), +1 to t + 1 (anti-parallel)"""
    sgn = rng.choice([-1.0, 1.0], size=(m, D))
    v = sgn * s * (t + 0.5 + side * DELTA)
    q = v.astype(np.float32)
    if np.log2(s) == np.floor(np.log2(s)):      # (a power of two: exactly representable; else 2^-24 beside, << DELTA)
        assert np.array_equal(q.astype(np.float64), v)
    return q


def _move(rng, b, q, comps, cells, s, outward=None):
    """move components of b by whole cells: the quantisation error stays what it was"""
    for c in comps:
        sign = np.sign(q[c]) if outward else (rng.choice([-1.0, 1.0]) if outward is None else -np.sign(q[c]))
        b[c] = np.float32(float(b[c]) + sign * cells * s)


def _plant(base, q_seed, s, t, m, decoys, flips):
    """queries on the grid of s and their family / decoy rows, written into base (see build_drop)"""
    rng = np.random.RandomState(q_seed)
    q = _midpoint_queries(rng, m, s, t, -1)
    fam = np.zeros((m, K), dtype=np.int64)
    dec = np.zeros((m, decoys), dtype=np.int64)
    stride = sampled_tile_stride(base.shape[0])              # family rows in sampled tiles, decoys in skipped ones
    assert stride >= 128 and stride * m <= base.shape[0] and K <= 32 and decoys <= 64
    for i in range(m):
        for j in range(K):
            row = stride * i + j
            b = q[i].copy()
            _move(rng, b, q[i], rng.choice(D, j + 1, replace=False), 1, s)
            base[row] = b
            fam[i, j] = row
        for r in range(decoys):
            row = stride * i + 64 + r
            b = q[i].copy()
            comps = rng.choice(D, flips + K + 1, replace=False)
            for c in comps[:flips]:
                b[c] = np.float32(np.sign(q[i, c]) * s * (t + 0.5 + DELTA))
            _move(rng, b, q[i], comps[flips:], 1, s)
            base[row] = b
            dec[i, r] = row
    return q, fam, dec


def build_drop(seed=1, n=N_DROP, m=96, decoys=0, flips=3):
    """(a) drop direction, and with decoys > 0 (b) cut direction.  Returns base, queries, fam [m][K], dec [m][decoys].

    Query i: every |q_i| = s (t + 1/2 - DELTA), random signs: e_q = sign(q_i) s (1/2 - DELTA) in every component.
    Family row j of query i (row stride i + j, stride 128: a tile the fp16 sampled pass reads, K residues mod 32 of one chunk):
    the query with j + 1 components moved by one cell -- the same error vector, score (j + 1) s^2.
    Decoy r (row stride i + 64 + r: a tile the sampled pass skips): the query with `flips` components pushed across
    the rounding midpoint (their error flips sign: the centre drops by ~2 (2t + 1) s^2 each) and K + 1 components
    moved by one cell: score (K + 1) s^2 + flips (2 DELTA s)^2, above every family row's."""
    rng = np.random.RandomState(seed)
    s = 2.0 ** E
    base = _far_rows(rng, n, s)
    base[n - 1, 0] = np.float32(127.0 * s)
    q, fam, dec = _plant(base, seed + 1000, s, _t_for_lambda(base, s), m, decoys, flips)
    return base, q, fam, dec


def build_sample(seed=2, n=N_SAMPLE, m=72, near=5, mids=6, t=32, cells=35, comps=10):
    """(c) proven tau of the int8 sampled pass.  Returns base, queries, near_rows [m][near], mid_rows [m][mids].

    Query i: every |q_i| = s (t + 1/2 + DELTA): rounds to t + 1, e_q = -sign(q_i) s (1/2 - DELTA), anti-parallel
    to q.  All planted rows keep that error vector, so q.e_b = -|q| |e_b| and e_q.b ~ -|e_q| |b|: their exact
    score is their centre PLUS nearly the half-width -- they look nearer than they are.
    near rows (1024 i + j): the query with j + 1 components moved by one cell; fewer than K of them.
    mid rows (1024 i + near + r): `comps` components moved outward by `cells` cells and r by one cell: scores
    ~comps cells^2 s^2, far enough that their LOWER bound exceeds the nearest row's centre (tau_s of spec_rank 1):
    the speculative list holds the near rows alone, fewer than K, and the redo pass filters with the proven tau
    made from g_K -- a mid row's.  t is below the AM-GM optimum so that the mid rows' row_w stays under w_cap."""
    rng = np.random.RandomState(seed)
    s = 2.0 ** E
    base = _far_rows(rng, n, s)
    q = _midpoint_queries(rng, m, s, t, +1)
    nr = np.zeros((m, near), dtype=np.int64)
    mr = np.zeros((m, mids), dtype=np.int64)
    stride = sampled_tile_stride(n)
    assert stride * m <= n and near < K <= near + mids <= 32
    for i in range(m):
        for j in range(near):
            row = stride * i + j
            b = q[i].copy()
            _move(rng, b, q[i], rng.choice(D, j + 1, replace=False), 1, s)
            base[row] = b
            nr[i, j] = row
        for r in range(mids):
            row = stride * i + near + r
            b = q[i].copy()
            cc = rng.choice(D, comps + r, replace=False)
            _move(rng, b, q[i], cc[:comps], cells, s, outward=True)
            _move(rng, b, q[i], cc[comps:], 1, s, outward=True)
            base[row] = b
            mr[i, r] = row
    base[n - 1, 0] = np.float32(127.0 * s)
    return base, q, nr, mr


def build_edge(kind, seed=3, n=N_DROP, m=96):
    """(d) edges of the integer range, the (a) construction on an index whose scale is set by the clip.
    "clip": query 0 and its first family row get a component of 6.5 x 32 s, beyond the clip of 5.5 rms, and M_q of
    that query takes its 2 B |e_q| branch.  "clamp": one far row gets a component of 1500 x 32 s: c V_b drives its
    bp to the lower clamp limit -- key -inf, a candidate of every query.  Either way max |x| > 5.5 rms, so
    s = 5.5 rms / 127 is no power of two and depends on the planted rows: they are planted on the grid of the s the
    index has WITH them (a fixed point, reached in three rounds to far below DELTA cells)."""
    rng = np.random.RandomState(seed)
    base = _far_rows(rng, n, 2.0 ** E)
    if kind == "clamp":
        base[20000, 7] = np.float32(1500.0)
    s = 2.0 ** E
    for _ in range(4):
        q, fam, _ = _plant(base, seed + 1000, s, _t_for_lambda(base, s), m, 0, 0)
        if kind == "clip":
            q[0, 5] = base[fam[0, 0], 5] = np.float32(6.5)
        s = index_scale(base)[0]
    return base, q, fam


def build_iid(seed=4, n=N_DROP, m=96):
    rng = np.random.RandomState(seed)
    return rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((m, D)).astype(np.float32)


# ---- what the constructions claim, asserted on the model ---------------------------------------------------
def assert_cut_orderings(mod, Qi, S_i, fam_i, dec_i):
    """(b), one query: every decoy's kappa is below every family row's -- the first re-rank round (the K rounded up to
    16 smallest keys) holds decoys alone -- while every decoy's exact score is above the K-th family score; and the
    cut the analysis derives from the decoys' K-th score keeps every family row"""
    sk = np.sort(S_i[fam_i])[K - 1]
    tau = np.float32(sk)                                       # the tightest threshold a sound sampled pass can give
    kf, kd = mod.kappa(Qi, tau, fam_i)[0], mod.kappa(Qi, tau, dec_i)[0]
    assert len(dec_i) >= 16 and kd.max() < kf.min(), (kd.max(), kf.min())
    assert S_i[dec_i].min() > sk, (S_i[dec_i].min(), sk)
    T = np.sort(S_i[dec_i])[K - 1]
    assert (kf <= mod.cut_two_rounds(T, tau)).all()
    kth = np.sort(kd + mod.rows["w"][dec_i])[K - 1]           # one round: kappa <= kth(kappa + w_b) + w_q
    assert (kf <= kth + mod.w_q(Qi, tau)[0]).all()


def sample_bites(mod, Q, near, mid, ref):
    """(c): per query, how much of the proven tau's room over the centre of the K-th largest class maximum the true
    K-th score consumes; asserts what the construction claims on the way"""
    assert mod.rows["seen"][near].all() and mod.rows["seen"][mid].all()       # row_w <= w_cap: they are class maxima
    assert mod.wb_max() == mod.rows["w"][mid].max()                         # ... and wb_max is theirs, not a far row's
    m = near.shape[0]
    bites = np.empty(m)
    for i in range(m):
        Qi = {name: v[i:i + 1] for name, v in Q.items()}
        rows = np.concatenate([near[i], mid[i]])
        assert set(ref[0][i].tolist()) <= set(rows.tolist())                # the planted rows are the answer
        sk = float(ref[1][i, -1])
        pr = mod.pairs(Qi, rows)
        g = mod.g(Qi, rows)[0]
        order = np.argsort(-g, kind="stable")
        tau_s = pr["centre"][0][order[0]]                                   # spec_rank 1: the best maximum's centre
        assert (pr["L"][0] <= tau_s).sum() < K                              # the speculative list fails short of K rows
        tau = float(mod.proven_tau(Qi, g[order[K - 1]])[0])
        assert tau >= sk, (tau, sk)
        ck = pr["centre"][0][order[K - 1]]
        bites[i] = (sk - ck) / (tau - ck)
    return bites
