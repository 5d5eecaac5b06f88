"""fp32 brute force at any dim that is a multiple of 16 up to 4096 (the dims without kernels of their own:
scan_filter_f32_any, score_ids_f32_any, the run-time-dim fp16 filter scan_gemm_f16kl): ids and fp32 distance
bits equal to the oracle's on every path -- exact scan, sampled pass + fp16 filter, fallbacks and retries."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = np.uint64(2 ** 64 - 1)
DIMS = [16, 48, 96, 384, 400, 1024, 1536, 2048, 3072, 4096]


def _gauss(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32)


def _engine(base, metric="l2"):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(base.shape[1], metric)
    eng.store_many_vectors(base)
    eng.build()
    return eng


def _om(oracle, metric):
    return oracle.METRIC_L2_F32 if metric == "l2" else oracle.METRIC_IP_F32


def _same(ids, dists, rids, rd):
    assert np.array_equal(ids, rids)
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32))


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", DIMS)
def test_small_index_exact_scan(oracle, d, metric):
    n, m, k = 3000, 9, 10
    base, queries = _gauss(d, n, d), _gauss(d + 1, m, d)
    eng = _engine(base, metric)
    ids, dists = eng.query_k_batch(queries, k)
    eng.close()
    _same(ids, dists, *oracle.brute_force(base, queries, k, _om(oracle, metric), n_threads=16))


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", DIMS)
def test_gemm_size(oracle, d, metric):
    n, m = 65_536, 97
    base, queries = _gauss(10 * d, n, d), _gauss(10 * d + 1, m, d)
    rids, rd = oracle.brute_force(base, queries, 100, _om(oracle, metric), n_threads=16)
    eng = _engine(base, metric)
    eng.set_profiling(True)
    for k in (1, 10, 100):
        ids, dists = eng.query_k_batch(queries, k)
        prof = eng.get_profile()
        _same(ids, dists, rids[:, :k], rd[:, :k])
        if d >= 64:
            assert prof["scan_kernel"].startswith("scan_gemm_f16"), prof["scan_kernel"]
            assert prof["retries"] == 0, (k, prof)
    eng.close()


def test_ties_duplicates_and_padding(oracle):
    d = 400
    base = _gauss(7, 5000, d)
    base[100:140] = base[3]                       # repeated rows
    queries = _gauss(8, 6, d)
    queries[0] = base[3]                          # a query equal to a base row (and to its copies)
    queries[1] = base[4999]
    eng = _engine(base)
    for k in (1, 50):
        _same(*eng.query_k_batch(queries, k), *oracle.brute_force(base, queries, k, oracle.METRIC_L2_F32, n_threads=16))
    eng.close()
    small = base[:20].copy()                      # k > n: UINT64_MAX / +inf padding
    eng = _engine(small)
    ids, dists = eng.query_k_batch(queries, 32)
    eng.close()
    assert (ids[:, 20:] == PAD).all() and np.isinf(dists[:, 20:]).all()
    _same(ids[:, :20], dists[:, :20], *oracle.brute_force(small, queries, 20, oracle.METRIC_L2_F32, n_threads=16))


def test_gemm_ties_and_duplicates(oracle):
    d = 1536
    base = _gauss(11, 70_000, d)
    base[5000:5300] = base[17]
    queries = _gauss(12, 100, d)
    queries[0] = base[17]
    eng = _engine(base)
    ids, dists = eng.query_k_batch(queries, 10)
    eng.close()
    _same(ids, dists, *oracle.brute_force(base, queries, 10, oracle.METRIC_L2_F32, n_threads=16))


def test_ip_norms_over_two_decades(oracle):
    """the seed-619 shape: query and row norms spread over two decades, k = 100"""
    rng = np.random.default_rng(619)
    n, d, m, k = 70_000, 1536, 130, 100
    base = (rng.standard_normal((n, d), dtype=np.float32) * 10.0 ** rng.uniform(-1, 1, (n, 1))).astype(np.float32)
    queries = (rng.standard_normal((m, d), dtype=np.float32) * 10.0 ** rng.uniform(-1, 1, (m, 1))).astype(np.float32)
    eng = _engine(base, "ip")
    _same(*eng.query_k_batch(queries, k), *oracle.brute_force(base, queries, k, oracle.METRIC_IP_F32, n_threads=16))
    eng.close()


def test_queries_outside_the_fp16_range_fall_back(oracle):
    n, d, m, k = 70_000, 1536, 100, 10
    base, queries = _gauss(21, n, d), _gauss(22, m, d)
    queries[5, 7] = 1.0e9                         # scaled by the index's power of two: far outside fp16
    eng = _engine(base)
    eng.set_profiling(True)
    ids, dists = eng.query_k_batch(queries, k)
    prof = eng.get_profile()
    eng.close()
    assert prof["scan_kernel"].startswith("scan_filter_f32"), prof
    _same(ids, dists, *oracle.brute_force(base, queries, k, oracle.METRIC_L2_F32, n_threads=16))


def test_forced_overflow_retry(oracle):
    n, d, m, k = 100_000, 2048, 130, 64          # (lists of 128 keys: the full scan's ~6 k candidates overflow)
    base, queries = _gauss(31, n, d), _gauss(32, m, d)
    eng = _engine(base)
    eng.set_option("cand_capacity", 64)
    eng.set_profiling(True)
    ids, dists = eng.query_k_batch(queries, k)
    assert eng.get_profile()["retries"] >= 1
    eng.close()
    _same(ids, dists, *oracle.brute_force(base, queries, k, oracle.METRIC_L2_F32, n_threads=16))


def test_async_search_and_sync(oracle):
    torch = pytest.importorskip("torch")
    n, d, m, k = 70_000, 1536, 200, 10
    base, q1, q2 = _gauss(41, n, d), _gauss(42, m, d), _gauss(43, m, d)
    eng = _engine(base)
    eng.set_option("async_search", 1)
    tq = [torch.from_numpy(q).cuda() for q in (q1, q2)]
    out = [(torch.empty(m, k, dtype=torch.int64, device="cuda"), torch.empty(m, k, dtype=torch.float32, device="cuda"))
           for _ in range(2)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    for q, (i, dd) in zip(tq, out):
        eng.search_device(q.data_ptr(), m, k, i.data_ptr(), dd.data_ptr(), st.cuda_stream)
    eng.sync()
    torch.cuda.synchronize()
    eng.close()
    for q, (i, dd) in zip((q1, q2), out):
        _same(i.cpu().numpy().view(np.uint64), dd.cpu().numpy(),
              *oracle.brute_force(base, q, k, oracle.METRIC_L2_F32, n_threads=16))


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", [400, 3072])
def test_score_ids(oracle, d, metric):
    base = _gauss(d + 5, 3000, d)
    query = _gauss(d + 6, 1, d)[0]
    ids = np.random.default_rng(d).integers(0, 3000, 700).astype(np.uint64)
    om = _om(oracle, metric)
    all_ids, all_sc = oracle.filter_by_score(base, query, ids, float("inf"), om)
    cutoff = float(np.median(all_sc))
    eng = _engine(base, metric)
    for c in (float("inf"), cutoff):
        kept, sc = eng.score_ids(query, ids, c)
        rk, rs = oracle.filter_by_score(base, query, ids, c, om)
        assert np.array_equal(kept, rk)
        assert np.array_equal(sc.view(np.uint32), rs.view(np.uint32))
    eng.close()


def test_rows_past_2_to_the_32_elements(oracle):
    """n * d > 2^32 (1.05 M x 4096): 64-bit row and query offsets in every kernel"""
    torch = pytest.importorskip("torch")
    n, d, m, k = 1_050_000, 4096, 16, 10
    g = torch.Generator(device="cuda")
    g.manual_seed(4096)
    base = torch.randn(n, d, device="cuda", generator=g)
    queries = base[torch.tensor([3, 1_049_999, 700_000, 1_048_577])].clone() + 0.01
    queries = torch.cat([queries, torch.randn(m - 4, d, device="cuda", generator=g)])
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(d, "l2")
    eng.set_base_device(base.data_ptr(), n, 0)
    eng.set_profiling(True)
    ids = torch.empty(m, k, dtype=torch.int64, device="cuda")
    dd = torch.empty(m, k, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.search_device(queries.data_ptr(), m, k, ids.data_ptr(), dd.data_ptr(), 0)
    torch.cuda.synchronize()
    prof = eng.get_profile()
    eng.close()
    qh = queries.cpu().numpy()
    bh = base.cpu().numpy()
    del base
    rids, rd = oracle.brute_force(bh, qh, k, oracle.METRIC_L2_F32, n_threads=16)
    assert prof["scan_kernel"].startswith("scan_gemm_f16kl"), prof
    _same(ids.cpu().numpy().view(np.uint64), dd.cpu().numpy(), rids, rd)
    assert rids[1, 0] == 1_049_999 and rids[3, 0] == 1_048_577


@pytest.mark.parametrize("d,name", [(128, "scan_gemm_f16x<128, false>"), (768, "scan_gemm_f16kx<768, false>")])
def test_compiled_dims_keep_their_kernels(oracle, d, name):
    n, m, k = 70_000, 140, 10
    base, queries = _gauss(d + 50, n, d), _gauss(d + 51, m, d)
    eng = _engine(base)
    eng.set_profiling(True)
    ids, dists = eng.query_k_batch(queries, k)
    assert eng.get_profile()["scan_kernel"] == name
    eng.close()
    _same(ids, dists, *oracle.brute_force(base, queries, k, oracle.METRIC_L2_F32, n_threads=16))


@pytest.mark.parametrize("seed", range(int(os.environ.get("EXPANN_ANY_DIM_FUZZ_N", "24"))))
def test_random_any_dim(oracle, seed):
    rng = np.random.default_rng(7000 + seed)
    d = 16 * int(rng.integers(1, 257))
    n = int(rng.choice([700, 5000, 20000, 70001]))
    m = int(rng.choice([1, 3, 8, 23, 97, 300]))
    k = int(rng.choice([1, 5, 10, 17, 64, 100]))
    metric = str(rng.choice(["l2", "l2", "ip"]))
    kind = str(rng.choice(["gauss", "clustered", "scaled", "dups"]))
    base = rng.standard_normal((n, d), dtype=np.float32)
    queries = rng.standard_normal((m, d), dtype=np.float32)
    if kind == "clustered":
        c = int(rng.integers(8, 200))
        centres = rng.standard_normal((c, d), dtype=np.float32)
        base = (centres[rng.integers(0, c, n)] + 0.2 * base).astype(np.float32)
        queries = (centres[rng.integers(0, c, m)] + 0.2 * queries).astype(np.float32)
    elif kind == "scaled":
        base = (base * 10.0 ** rng.uniform(-1, 1, (n, 1))).astype(np.float32)
        queries = (queries * 10.0 ** rng.uniform(-1, 1, (m, 1))).astype(np.float32)
    elif kind == "dups":
        base[rng.integers(0, n, n // 3)] = base[int(rng.integers(0, n))]
        queries[0] = base[0]
    eng = _engine(base, metric)
    ids, dists = eng.query_k_batch(queries, k)
    eng.close()
    _same(ids, dists, *oracle.brute_force(base, queries, k, _om(oracle, metric), n_threads=16))
