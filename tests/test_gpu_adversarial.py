"""Adversarial soundness of the conservative fp16 filter (scan_gemm_f16.hpp / scan_gemm_f16kx.hpp).

The filter may only DROP a row when its reference-order score is certainly above the threshold;
its slack  eps_d (|q|^2 + |b|^2) + abs (|q| + |b|)  is 12.5 % (d <= 256) above the worst case of
the fp16 input rounding, and that worst case needs (1) every component of q and of b rounded in
the SAME direction by the full half-ulp, (2) |q_i| = |b_i| in every component (q ~ b: the
expanded form cancels catastrophically) and (3) a threshold with no room of its own.  Random data
never comes near it (errors grow like sqrt(d), not d).  These tests construct it:

  * every component is  +-2^e (1 + j 2^-10 + 2^-11 -+ 2^-23), j small: one fp32 ulp beside the
    midpoint of two fp16 neighbours, so fp16 rounding moves ALL of them down (or all up) by
    ~2^-11 relative;
  * the true neighbours of a query are the query itself with a few components doubled (same
    mantissa, same rounding direction, score = sum of those q_i^2 << |q|^2 + |b|^2);
  * they sit in rows that every threshold sample contains, so with the threshold ladder
    (sample_pass = 0) tau is EXACTLY the k-th neighbour's reference-order score: that row has to
    pass `estimate <= tau` with nothing but the slack between them.

`bite` (host arithmetic, float64) is the fraction of the slack the construction really consumes;
the asserts on it keep the test honest.  Ids and distance bits must equal the oracle's.

The slack formula is implemented once per geometry; the second half of the file takes the same construction to
the ones the first three dims do not reach: scan_gemm_f16x<64>, the d = 256 instance of scan_gemm_w8,
scan_gemm_f16kx<768> / <832>, the run-time-dim form, the few-query direct path, binary16 rows, the masked row
terms under a row filter and the ip_rescale query scaling.  A threshold made by a sampled pass comes from the same
fp16 estimate as the scan's and carries the slack itself, so the family row always passes it: what bites is the
threshold ladder, whose level 0 scores its rows exactly (sample_pass = 0, and every small index below)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, M, K = 65536, 40, 10


def _adv(rng, shape, direction):
    """fp32 values one ulp beside an fp16 rounding midpoint; direction -1: fp16 rounds toward zero,
    +1: away from zero, 0: half / half."""
    e = rng.randint(-3, 1, size=shape)
    j = rng.randint(0, 6, size=shape)
    sgn = rng.choice([-1.0, 1.0], size=shape)
    if direction == 0:
        dirs = rng.choice([-1.0, 1.0], size=shape)
    else:
        dirs = np.full(shape, float(direction))
    mant = 1.0 + j * 2.0 ** -10 + 2.0 ** -11 + dirs * 2.0 ** -23
    v = (sgn * mant * 2.0 ** e).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), sgn * mant * 2.0 ** e)      # exactly representable
    return v


def _sample_stride(n):
    """rows between the starts of the 16-row groups every threshold sample holds: level 0 of plan_levels (expann_hip.hip)
    scans s0 = max(64, 4 K / 16) groups, each n_groups / s0 groups after the one before"""
    n_groups = (n + 15) // 16
    s0 = max(64, (4 * K + 15) // 16)
    assert n_groups > s0
    return 16 * (n_groups // s0)


def _build(d, direction, seed, n=N, m=M, step=1):
    """family row jn of query t sits at row stride t + step jn (step 8: every eighth row, for the row filter's case)"""
    rng = np.random.RandomState(seed)
    q = _adv(rng, (m, d), direction)
    qn = float(np.sqrt((q[0].astype(np.float64) ** 2).sum()))
    base = (rng.standard_normal((n, d)) * qn / np.sqrt(d)).astype(np.float32)    # far rows, same norm
    stride = _sample_stride(n)
    assert m <= 64 and stride * m < n and step * K <= 16 * 8
    fam = np.zeros((m, K), dtype=np.int64)
    for t in range(m):
        order = np.argsort(np.abs(q[t]), kind="stable")      # smallest components first
        for jn in range(K):
            row = stride * t + step * jn                      # inside every threshold sample
            b = q[t].copy()
            b[order[:jn + 1]] *= 2.0                          # same mantissa, same rounding direction
            base[row] = b
            fam[t, jn] = row
    base[stride * m] = q[0]                                   # an exact duplicate of a query (score 0)
    return base, q, fam


def _bite(base, q, fam, d):
    """largest fraction of the L2 slack consumed by a family row (float64 on the exact values); eps is
    gemm_f16_filter_eps(d) of scan_gemm_f16.hpp, the real d for the run-time-dim form too"""
    from math import sqrt
    eps = 1.125 * 2.0 ** -10 if d <= 256 else 2.0 ** -10 + (4.0 + 4.25 * d + 256.0) * 2.0 ** -24
    maxabs = max(np.abs(base).max(), 1e-30)
    s = 2.0 ** np.floor(np.log2(32768.0 / maxabs))
    worst = 0.0
    for t in range(q.shape[0]):
        qt = q[t].astype(np.float64)
        q16 = (q[t] * np.float32(s)).astype(np.float16).astype(np.float64)
        for row in fam[t]:
            b = base[row].astype(np.float64)
            b16 = (base[row] * np.float32(s)).astype(np.float16).astype(np.float64)
            nq, nb = (qt ** 2).sum(), (b ** 2).sum()
            true = ((qt - b) ** 2).sum()
            raw = (nq + nb - 2.0 * (q16 * b16).sum() / s ** 2) - true
            slack = eps * (nq + nb) + 2.0 ** -24 / s * sqrt(d) * (sqrt(nq) + sqrt(nb))
            worst = max(worst, raw / slack)
    return worst


@pytest.mark.parametrize("d", [128, 512, 960])
@pytest.mark.parametrize("direction", [-1, 1, 0])
def test_same_signed_rounding_with_cancellation_and_exact_thresholds(oracle, d, direction):
    from expann_amd import GpuBruteForceEngine
    base, q, fam = _build(d, direction, 1000 + d + direction)
    if direction == -1:
        bite = _bite(base, q, fam, d)
        # theory: 1 / 1.125 = 0.889 (d <= 256), 0.87 at d = 512, 0.79 at d = 960, reached up to the
        # j-dependent mantissas and the far rows' share of the scale
        assert bite > (0.80 if d <= 512 else 0.72), bite
    for metric, om in (("l2", oracle.METRIC_L2_F32), ("ip", oracle.METRIC_IP_F32)):
        ref = oracle.brute_force(base, q, K, om, n_threads=16)
        if metric == "l2":   # the construction is what it claims: the family rows ARE the answer
            assert np.array_equal(np.sort(ref[0][1:], axis=1), np.sort(fam[1:].astype(np.uint64), axis=1))
        for opts in ({}, {"sample_pass": 0, "scan_kernel": 4}, {"scan_kernel": 4, "sample_frac": 4}):
            eng = GpuBruteForceEngine(d, metric)
            eng.store_many_vectors(base)
            eng.build()
            for name, val in opts.items():
                eng.set_option(name, val)
            eng.set_profiling(True)
            ids, dists = eng.query_k_batch(q, K)
            prof = eng.get_profile()
            eng.close()
            assert prof["scan_kernel"].startswith("scan_gemm_f16"), prof["scan_kernel"]   # the filter under test ran
            assert np.array_equal(ids, ref[0]), (metric, opts)
            assert np.array_equal(dists.view(np.uint32), ref[1].view(np.uint32)), (metric, opts)


def test_bf16_split_filter_same_signed_rounding(oracle):
    """the 3-term bf16 split (scan_kernel = 3): components one ulp beside a bf16 rounding midpoint in
    the hi part, same construction otherwise"""
    from expann_amd import GpuBruteForceEngine
    d = 128
    rng = np.random.RandomState(4242)
    e = rng.randint(-3, 1, size=(M, d))
    sgn = rng.choice([-1.0, 1.0], size=(M, d))
    # hi = bf16(x) keeps 8 bits: midpoint at 2^-8; lo = bf16(x - hi) keeps 8 more: put the value one
    # fp32 ulp below a midpoint of the SECOND split as well
    mant = 1.0 + 2.0 ** -8 - 2.0 ** -16 - 2.0 ** -23
    q = (sgn * mant * 2.0 ** e).astype(np.float32)
    qn = float(np.sqrt((q[0].astype(np.float64) ** 2).sum()))
    base = (rng.standard_normal((N, d)) * qn / np.sqrt(d)).astype(np.float32)
    for t in range(M):
        order = np.argsort(np.abs(q[t]), kind="stable")
        for jn in range(K):
            b = q[t].copy()
            b[order[:jn + 1]] *= 2.0
            base[1024 * t + jn] = b
    ref = oracle.brute_force(base, q, K, oracle.METRIC_L2_F32, n_threads=16)
    eng = GpuBruteForceEngine(d, "l2")
    eng.store_many_vectors(base)
    eng.build()
    eng.set_option("scan_kernel", 3)
    ids, dists = eng.query_k_batch(q, K)
    eng.close()
    assert np.array_equal(ids, ref[0]) and np.array_equal(dists.view(np.uint32), ref[1].view(np.uint32))


# ---- the same construction on every other implementation of the slack ----------------------------------------
# Small indexes (8 192 rows, + 16 where a case is off the tile): below 2 * 256 * 64 rows no sampled pass runs, so
# every option set takes its thresholds from the ladder, whose level 0 holds the family rows -- tau is exactly the
# k-th score.  BITE: the value _bite measured on the host (direction -1) for each case; asserted with 0.05 of
# room.  Theory is (2^-10 / eps_d) x 0.997: 0.886 up to d = 256, 0.82 at 768, 0.81 at 832, 0.78 at 1040
# and 0.48 at 4096 -- there more than half of eps_d is kept for the d roundings of the fp32 accumulation, which no
# choice of inputs steers: the d = 4096 case runs the construction through the run-time-dim form's longest rows
# and is exact, but a halved eps would not fail it.  Binary16 rows: the rows carry no rounding of their own (they ARE
# fp16 values), only the queries do: half of the above.
SMALL = 8192
OPTS3 = ({}, {"sample_pass": 0, "scan_kernel": 4}, {"scan_kernel": 4, "sample_frac": 4})
BITE = {("f32", 64): 0.8862, ("f32", 256): 0.8860, ("f32", 768): 0.8203, ("f32", 832): 0.8092,
        ("f32", 80): 0.8864, ("f32", 1040): 0.7753, ("f32", 4096): 0.4796,
        ("few", 128): 0.8858, ("few", 512): 0.8676, ("f16", 128): 0.4432, ("f16", 832): 0.4047, ("filter", 128): 0.8860,
        ("filter", 768): 0.8203, ("ip", 128): 0.8862}


def _search(base, q, metric, opts, dtype="f32", allow=None):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(base.shape[1], metric, dtype=dtype)
    eng.store_many_vectors(base)
    eng.build()
    if allow is not None:
        eng.set_row_filter(allow)
    for name, val in opts.items():
        eng.set_option(name, val)
    eng.set_profiling(True)
    ids, dists = eng.query_k_batch(q, K)
    prof = eng.get_profile()
    eng.close()
    return ids, dists, prof


def _same(ids, dists, ref, what):
    assert np.array_equal(ids, ref[0]), what
    assert np.array_equal(dists.view(np.uint32), ref[1].view(np.uint32)), what


def _check_bite(key, base, q, fam, d, direction):
    if direction == -1:
        bite = _bite(base, q, fam, d)
        print(f"bite {key}: {bite:.4f}")
        assert bite > BITE[key] - 0.05, (key, bite)


def _both_metrics(oracle, base, q, fam, kernel, opt_sets=OPTS3):
    for metric, om in (("l2", oracle.METRIC_L2_F32), ("ip", oracle.METRIC_IP_F32)):
        ref = oracle.brute_force(base, q, K, om, n_threads=16)
        if metric == "l2":
            assert np.array_equal(np.sort(ref[0][1:], axis=1), np.sort(fam[1:].astype(np.uint64), axis=1))
        for opts in opt_sets:
            ids, dists, prof = _search(base, q, metric, opts)
            assert prof["scan_kernel"] == kernel, (prof["scan_kernel"], metric, opts)
            _same(ids, dists, ref, (metric, opts))


@pytest.mark.parametrize("d,n,kernel", [(64, SMALL, "scan_gemm_f16x<64, false>"), (256, SMALL + 16, "scan_gemm_f16y<256, false>"),
                                        (768, SMALL, "scan_gemm_f16kx<768, false>"), (832, SMALL, "scan_gemm_f16kx<832, false>")])
@pytest.mark.parametrize("direction", [-1, 1, 0])
def test_compiled_dims_without_a_case_of_their_own(oracle, d, n, kernel, direction):
    """scan_gemm_f16x<64>, the d = 256 instance of scan_gemm_w8 and scan_gemm_f16kx<768> / <832>"""
    base, q, fam = _build(d, direction, 2000 + d + direction, n=n)
    _check_bite(("f32", d), base, q, fam, d, direction)
    _both_metrics(oracle, base, q, fam, kernel)


@pytest.mark.parametrize("d,n", [(80, SMALL + 16), (1040, SMALL), (4096, SMALL)])
@pytest.mark.parametrize("direction", [-1, 1])
def test_run_time_dim_form(oracle, d, n, direction):
    """scan_gemm_kl<F16Elem>: rows padded to 32-element k-steps (d = 80 -> 96), eps of the real d up to 4096"""
    base, q, fam = _build(d, direction, 3000 + d + direction, n=n)
    _check_bite(("f32", d), base, q, fam, d, direction)
    _both_metrics(oracle, base, q, fam, "scan_gemm_f16kl")


# (d, m) -> the few-query kernel: scan_direct_f16<D, TQ> serves m <= TQ queries in one pass; d = 512 has TQ 1 and 2
# only (kDirectF16), and the planner gives four queries at d = 512 to the exact fp32 scan: no fp16 slack is involved
# there, the case stays for the exactness and names what ran
FEW = {(128, 1): "scan_direct_f16<128, 2>", (128, 2): "scan_direct_f16<128, 2>", (128, 4): "scan_direct_f16<128, 4>",
       (512, 1): "scan_direct_f16<512, 1>", (512, 2): "scan_direct_f16<512, 2>", (512, 4): "scan_filter_f32<512,4,"}


@pytest.mark.parametrize("d", [128, 512])
@pytest.mark.parametrize("sampled", [True, False])
def test_few_queries(oracle, d, sampled):
    """m = 1, 2, 4: scan_direct_f16 on the last level.  sampled: 32 768 + 16 rows, the smallest index the fused
    sample_direct_f16_kernel serves -- it reads every second 16-row step, the family rows' among them, K of one
    workgroup's 16 classes; else sample_pass = 0 on the small index (the ladder)"""
    n = 32768 + 16 if sampled else SMALL
    base, q, fam = _build(d, -1, 4000 + d + sampled, n=n, m=4)
    _check_bite(("few", d), base, q, fam, d, -1)
    for metric, om in (("l2", oracle.METRIC_L2_F32), ("ip", oracle.METRIC_IP_F32)):
        ref = oracle.brute_force(base, q, K, om, n_threads=16)
        for m in (1, 2, 4):
            ids, dists, prof = _search(base, q[:m], metric, {} if sampled else {"sample_pass": 0})
            assert prof["scan_kernel"].startswith(FEW[(d, m)]), (prof["scan_kernel"], d, m)
            _same(ids, dists, (ref[0][:m], ref[1][:m]), (metric, d, m, sampled))


@pytest.mark.parametrize("d,kernel", [(128, "scan_gemm_f16x<128, false>"), (832, "scan_gemm_f16kx<832, false>")])
def test_binary16_rows(oracle, d, kernel):
    """EXPANN_DTYPE_F16: the rows are the adversarial values rounded to binary16, the queries adversarial fp32; the
    oracle scores the upcast rows"""
    base, q, fam = _build(d, -1, 5000 + d, n=SMALL)
    base16 = base.astype(np.float16)
    up = base16.astype(np.float32)
    _check_bite(("f16", d), up, q, fam, d, -1)
    for metric, om in (("l2", oracle.METRIC_L2_F32), ("ip", oracle.METRIC_IP_F32)):
        ref = oracle.brute_force(up, q, K, om, n_threads=16)
        for opts in OPTS3:
            ids, dists, prof = _search(base16, q, metric, opts, dtype="f16")
            assert prof["scan_kernel"] == kernel, (prof["scan_kernel"], metric, opts)
            _same(ids, dists, ref, (metric, opts))


@pytest.mark.parametrize("d,kernel", [(128, "scan_gemm_f16x<128, false>"), (768, "scan_gemm_f16kx<768, false>")])
def test_masked_row_terms_under_a_row_filter(oracle, d, kernel):
    """rows 0 - 3 of every 8 allowed: the family rows (every eighth row) and half of the far rows.  Level 0 of the
    filtered ladder walks every fourth entry of the filter's list -- the rows that are multiples of 8 -- and scores
    them exactly, so tau is the k-th family score; the full scan then filters with the masked row terms"""
    base, q, fam = _build(d, -1, 6000 + d, n=SMALL, step=8)
    _check_bite(("filter", d), base, q, fam, d, -1)
    allow = (np.arange(SMALL) % 8) < 4
    assert allow[fam].all() and allow.sum() > 2048          # (more allowed rows than a list holds: no list-only search)
    rows = np.flatnonzero(allow)
    for metric, om in (("l2", oracle.METRIC_L2_F32), ("ip", oracle.METRIC_IP_F32)):
        rids, rd = oracle.brute_force(base[rows], q, K, om, n_threads=16)
        ref = (rows[rids.astype(np.int64)].astype(np.uint64), rd)
        for opts in OPTS3:
            ids, dists, prof = _search(base, q, metric, opts, allow=allow)
            assert prof["scan_kernel"] == kernel, (prof["scan_kernel"], metric, opts)
            _same(ids, dists, ref, (metric, opts))


@pytest.mark.parametrize("rescale", [1, 0])
def test_ip_rescale(oracle, rescale):
    """metric ip with the queries scaled to the rows' largest norm before the fp16 rounding ("ip_rescale" 1) and
    as they come (0)"""
    d = 128
    base, q, fam = _build(d, -1, 7000, n=SMALL)
    _check_bite(("ip", d), base, q, fam, d, -1)
    ref = oracle.brute_force(base, q, K, oracle.METRIC_IP_F32, n_threads=16)
    for opts in OPTS3:
        ids, dists, prof = _search(base, q, "ip", dict(opts, ip_rescale=rescale))
        assert prof["scan_kernel"] == "scan_gemm_f16x<128, false>", (prof["scan_kernel"], opts)
        _same(ids, dists, ref, opts)
