"""Brute force over 8-bit rows at any dim that is a multiple of 64 up to 4096 (the dims without kernels of
their own: scan_filter_i8_any, score_ids_i8_any, the run-time-dim int8 matrix-core filter scan_gemm_i8kl).
Integer scores are exact in any summation order, so ids and fp32 distance bits equal the oracle's on every
path -- exact scan, sampled pass + int8 filter, retries, the sharded handle."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = np.uint64(2 ** 64 - 1)
DIMS = [192, 320, 512, 1024, 1536, 2048, 3072, 4096]
# (dtype, engine metric, oracle metric)
SCORES = [("u8", "l2", "METRIC_L2_U8"), ("i8", "l2", "METRIC_L2_I8"),
          ("i8", "l2_i8_refcompat", "METRIC_L2_I8_REFCOMPAT"), ("i8", "ip", "METRIC_IP_I8")]
GEMM_SCORES = [s for s in SCORES if s[1] != "l2_i8_refcompat"]   # (the bilinear forms: what the matrix cores take)


def _rows(rng, n, d, dtype, lo=None, hi=None):
    """uint8 rows: full-range integers; int8 rows: the full int8 range"""
    if dtype == "u8":
        return rng.integers(0 if lo is None else lo, 256 if hi is None else hi, (n, d), dtype=np.uint8)
    return rng.integers(-128 if lo is None else lo, 128 if hi is None else hi, (n, d), dtype=np.int8)


def _queries(rng, m, d, dtype, lo=None, hi=None):
    """uint8 rows take fp32 queries holding integers in [0, 255]; int8 rows take int8 queries"""
    q = _rows(rng, m, d, dtype, lo, hi)
    return q.astype(np.float32) if dtype == "u8" else q


def _engine(base, metric, dtype):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(base.shape[1], metric, dtype)
    eng.store_many_vectors(base)
    eng.build()
    return eng


def _same(ids, dists, rids, rd):
    assert np.array_equal(ids, rids)
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32))


@pytest.mark.parametrize("dtype,metric,ometric", SCORES)
@pytest.mark.parametrize("d", DIMS)
def test_small_index_exact_scan(oracle, d, dtype, metric, ometric):
    n, m, k = 3000, 9, 10
    rng = np.random.default_rng(d)
    base, queries = _rows(rng, n, d, dtype), _queries(rng, m, d, dtype)
    eng = _engine(base, metric, dtype)
    eng.set_profiling(True)
    ids, dists = eng.query_k_batch(queries, k)
    prof = eng.get_profile()
    eng.close()
    assert prof["scan_kernel"].startswith("scan_filter_i8_any"), prof
    _same(ids, dists, *oracle.brute_force(base, queries, k, getattr(oracle, ometric), n_threads=16))


@pytest.mark.parametrize("dtype,metric,ometric", GEMM_SCORES)
@pytest.mark.parametrize("d", DIMS)
def test_gemm_size(oracle, d, dtype, metric, ometric):
    n, m = 65_536, 97
    rng = np.random.default_rng(10 * d)
    base, queries = _rows(rng, n, d, dtype), _queries(rng, m, d, dtype)
    rids, rd = oracle.brute_force(base, queries, 100, getattr(oracle, ometric), n_threads=16)
    eng = _engine(base, metric, dtype)
    eng.set_profiling(True)
    for k in (1, 10, 100):
        ids, dists = eng.query_k_batch(queries, k)
        prof = eng.get_profile()
        _same(ids, dists, rids[:, :k], rd[:, :k])
        assert prof["scan_kernel"].startswith("scan_gemm_i8kl"), prof["scan_kernel"]
        assert prof["retries"] == 0, (k, prof)
    eng.close()


@pytest.mark.parametrize("dtype,metric,ometric", GEMM_SCORES)
def test_d896_runs_on_the_1024_byte_slots(oracle, dtype, metric, ometric):
    """d = 896 is mapped onto the 1024-byte-slot instances of scan_gemm_i8x (as d = 832 / 960), the exact scan
    stays the run-time-dim one"""
    n, m, d = 65_536, 97, 896
    rng = np.random.default_rng(896)
    base, queries = _rows(rng, n, d, dtype), _queries(rng, m, d, dtype)
    rids, rd = oracle.brute_force(base, queries, 100, getattr(oracle, ometric), n_threads=16)
    eng = _engine(base, metric, dtype)
    eng.set_profiling(True)
    for k in (1, 10, 100):
        _same(*eng.query_k_batch(queries, k), rids[:, :k], rd[:, :k])
        prof = eng.get_profile()
        assert prof["scan_kernel"].startswith("scan_gemm_i8x<1024"), prof["scan_kernel"]
        assert prof["retries"] == 0, (k, prof)
    eng.set_option("scan_kernel", 1)
    _same(*eng.query_k_batch(queries[:9], 10), rids[:9, :10], rd[:9, :10])
    assert eng.get_profile()["scan_kernel"].startswith("scan_filter_i8_any"), eng.get_profile()
    eng.close()


def _tie_case(oracle):
    """d = 4096, uint8, full-range rows: every distance is ~4.5e7 > 2^25, where fp32 holds multiples of 4 only.
    The last rows of the index are copies of the 40 nearest rows of each of 8 queries with ONE byte moved by 1
    towards or away from the query: integer scores that differ by 1 .. 3 from the original's and collapse onto
    the same float, so the id has to break the tie."""
    n, d, m, k, nq, near = 70_000, 4096, 100, 100, 8, 40
    rng = np.random.default_rng(40960)
    base = _rows(rng, n, d, "u8")
    queries = _queries(rng, m, d, "u8")
    nids, _ = oracle.brute_force(base[:n - nq * near], queries[:nq], near, oracle.METRIC_L2_U8, n_threads=16)
    for j in range(nq):
        for i, r in enumerate(nids[j].astype(np.int64)):
            row = base[r].copy()
            diff = np.abs(row.astype(np.int32) - queries[j].astype(np.int32))
            c = int(np.argmin(diff + 1000 * ((row == 0) | (row == 255))))   # the byte nearest the query's (not at the range's end)
            row[c] = row[c] + 1 if i % 2 == 0 else row[c] - 1
            base[n - nq * near + j * near + i] = row
    return base, queries, k


def test_scores_above_2_to_the_24(oracle):
    base, queries, k = _tie_case(oracle)
    rids, rd = oracle.brute_force(base, queries, k, oracle.METRIC_L2_U8, n_threads=16)
    assert rd.min() > 2.0 ** 24
    ties = int(((rd[:, 1:] == rd[:, :-1]) & (rids[:, 1:] != rids[:, :-1])).sum())
    assert ties >= 20, ties                                   # (the condition on the data, from the oracle's output)
    eng = _engine(base, "l2", "u8")
    eng.set_profiling(True)
    _same(*eng.query_k_batch(queries, k), rids, rd)           # auto: the int8 matrix-core filter
    assert eng.get_profile()["scan_kernel"].startswith("scan_gemm_i8kl"), eng.get_profile()
    eng.set_option("scan_kernel", 1)                          # the exact scan
    _same(*eng.query_k_batch(queries, k), rids, rd)
    assert eng.get_profile()["scan_kernel"].startswith("scan_filter_i8_any"), eng.get_profile()
    eng.close()


@pytest.mark.parametrize("dtype,metric,ometric", [SCORES[0], SCORES[3]])
def test_duplicates_query_equal_to_a_row_and_padding(oracle, dtype, metric, ometric):
    d = 320
    rng = np.random.default_rng(7)
    base = _rows(rng, 5000, d, dtype)
    base[100:140] = base[3]                       # repeated rows
    queries = _queries(rng, 6, d, dtype)
    queries[0] = base[3]                          # a query equal to a base row (and to its copies)
    queries[1] = base[4999]
    om = getattr(oracle, ometric)
    eng = _engine(base, metric, dtype)
    for k in (1, 50):
        _same(*eng.query_k_batch(queries, k), *oracle.brute_force(base, queries, k, om, n_threads=16))
    eng.close()
    small = base[:20].copy()                      # k > n: UINT64_MAX / +inf padding
    eng = _engine(small, metric, dtype)
    ids, dists = eng.query_k_batch(queries, 32)
    eng.close()
    assert (ids[:, 20:] == PAD).all() and np.isinf(dists[:, 20:]).all()
    _same(ids[:, :20], dists[:, :20], *oracle.brute_force(small, queries, 20, om, n_threads=16))


def test_gemm_duplicates(oracle):
    d = 1536
    rng = np.random.default_rng(11)
    base = _rows(rng, 70_000, d, "i8")
    base[5000:5300] = base[17]
    queries = _queries(rng, 100, d, "i8")
    queries[0] = base[17]
    eng = _engine(base, "l2", "i8")
    ids, dists = eng.query_k_batch(queries, 10)
    eng.close()
    _same(ids, dists, *oracle.brute_force(base, queries, 10, oracle.METRIC_L2_I8, n_threads=16))


def test_forced_overflow_retry(oracle):
    n, d, m, k = 100_000, 2048, 130, 64          # (lists of 128 keys: the full scan's candidates overflow them)
    rng = np.random.default_rng(31)
    base, queries = _rows(rng, n, d, "u8"), _queries(rng, m, d, "u8")
    eng = _engine(base, "l2", "u8")
    eng.set_option("cand_capacity", 64)
    eng.set_profiling(True)
    ids, dists = eng.query_k_batch(queries, k)
    assert eng.get_profile()["retries"] >= 1
    eng.close()
    _same(ids, dists, *oracle.brute_force(base, queries, k, oracle.METRIC_L2_U8, n_threads=16))


def test_async_search_and_sync(oracle):
    torch = pytest.importorskip("torch")
    n, d, m, k = 70_000, 1536, 200, 10
    rng = np.random.default_rng(41)
    base, q1, q2 = _rows(rng, n, d, "i8"), _queries(rng, m, d, "i8"), _queries(rng, m, d, "i8")
    eng = _engine(base, "ip", "i8")
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
              *oracle.brute_force(base, q, k, oracle.METRIC_IP_I8, n_threads=16))


@pytest.mark.parametrize("dtype,metric,ometric", [SCORES[0], SCORES[3]])
@pytest.mark.parametrize("d", [320, 3072])
def test_score_ids(oracle, d, dtype, metric, ometric):
    rng = np.random.default_rng(d + 5)
    base = _rows(rng, 3000, d, dtype)
    query = _queries(rng, 1, d, dtype)[0]
    ids = rng.integers(0, 3000, 700).astype(np.uint64)
    om = getattr(oracle, ometric)
    all_ids, all_sc = oracle.filter_by_score(base, query, ids, float("inf"), om)
    cutoff = float(np.median(all_sc))
    eng = _engine(base, metric, dtype)
    for c in (float("inf"), cutoff):
        kept, sc = eng.score_ids(query, ids, c)
        rk, rs = oracle.filter_by_score(base, query, ids, c, om)
        assert np.array_equal(kept, rk)
        assert np.array_equal(sc.view(np.uint32), rs.view(np.uint32))
    eng.close()


def test_rows_past_2_to_the_32_bytes(oracle):
    """n * d > 2^32 (1.05 M x 4096 uint8): 64-bit row offsets in every kernel"""
    torch = pytest.importorskip("torch")
    n, d, m, k = 1_050_000, 4096, 16, 10
    g = torch.Generator(device="cuda")
    g.manual_seed(4096)
    base = torch.randint(0, 256, (n, d), dtype=torch.uint8, device="cuda", generator=g)
    queries = base[torch.tensor([3, 1_049_999, 700_000, 1_048_577], device="cuda")].to(torch.float32)
    queries[:, 5] = torch.where(queries[:, 5] < 128, queries[:, 5] + 1, queries[:, 5] - 1)   # next to, not on, the row
    queries = torch.cat([queries, torch.randint(0, 256, (m - 4, d), device="cuda", generator=g).to(torch.float32)])
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(d, "l2", "u8")
    eng.set_base_device(base.data_ptr(), n, 0)
    ids = torch.empty(m, k, dtype=torch.int64, device="cuda")
    dd = torch.empty(m, k, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.search_device(queries.data_ptr(), m, k, ids.data_ptr(), dd.data_ptr(), 0)
    torch.cuda.synchronize()
    eng.close()
    qh = queries.cpu().numpy()
    bh = base.cpu().numpy()
    del base
    rids, rd = oracle.brute_force(bh, qh, k, oracle.METRIC_L2_U8, n_threads=16)
    _same(ids.cpu().numpy().view(np.uint64), dd.cpu().numpy(), rids, rd)
    assert rids[1, 0] == 1_049_999 and rids[3, 0] == 1_048_577


@pytest.mark.parametrize("dtype,metric,ometric,d,n,m,k,name", [
    ("u8", "l2", "METRIC_L2_U8", 128, 70001, 300, 17, "scan_gemm_i8w<128,U8L2>"),
    ("i8", "ip", "METRIC_IP_I8", 128, 65536, 97, 100, "scan_gemm_i8w<128,I8IP>"),
    ("i8", "l2", "METRIC_L2_I8", 768, 70001, 300, 17, "scan_gemm_i8x<768,I8L2>"),
    ("i8", "ip", "METRIC_IP_I8", 768, 65536, 97, 100, "scan_gemm_i8x<768,I8IP>"),
])
def test_compiled_dims_keep_their_kernels(oracle, dtype, metric, ometric, d, n, m, k, name):
    rng = np.random.default_rng(n + d + m)
    base, queries = _rows(rng, n, d, dtype), _queries(rng, m, d, dtype)
    eng = _engine(base, metric, dtype)
    eng.set_profiling(True)
    ids, dists = eng.query_k_batch(queries, k)
    assert eng.get_profile()["scan_kernel"] == name
    eng.close()
    _same(ids, dists, *oracle.brute_force(base, queries, k, getattr(oracle, ometric), n_threads=16))


def test_three_shards_on_one_device_d1536_int8_ip(oracle):
    from expann_amd import GpuBruteForceEngine, ShardedBruteForceEngine
    rng = np.random.default_rng(1536)
    n, d, m, k = 70_000, 1536, 100, 10
    base, queries = _rows(rng, n, d, "i8"), _queries(rng, m, d, "i8")
    sh = ShardedBruteForceEngine(d, "ip", "i8", devices=[0, 0, 0])
    sh.store_many_vectors(base)
    sh.build()
    ids, dists = sh.query_k_batch(queries, k)
    sh.close()
    one = _engine(base, "ip", "i8")
    pids, pd = one.query_k_batch(queries, k)
    one.close()
    rids, rd = oracle.brute_force(base, queries, k, oracle.METRIC_IP_I8, n_threads=16)
    _same(ids, dists, rids, rd)
    _same(pids, pd, rids, rd)


@pytest.mark.parametrize("seed", range(int(os.environ.get("EXPANN_I8_ANY_DIM_FUZZ_N", "24"))))
def test_random_i8_any_dim(oracle, seed):
    rng = np.random.default_rng(8000 + seed)
    d = 64 * int(rng.integers(1, 65))
    n = int(rng.choice([700, 5000, 20000, 70001]))
    m = int(rng.choice([1, 3, 8, 23, 97, 300]))
    k = int(rng.choice([1, 5, 10, 17, 64, 100]))
    dtype, metric, ometric = SCORES[int(rng.integers(0, len(SCORES)))]
    kind = str(rng.choice(["uniform", "clustered", "lowrange", "dups"]))
    base, queries = _rows(rng, n, d, dtype), _queries(rng, m, d, dtype)
    if kind == "clustered":
        c = int(rng.integers(8, 200))
        lo, hi = (0, 255) if dtype == "u8" else (-128, 127)
        centres = _rows(rng, c, d, dtype).astype(np.int32)

        def near(count):
            x = centres[rng.integers(0, c, count)] + rng.integers(-12, 13, (count, d))
            return np.clip(x, lo, hi).astype(base.dtype)
        base, queries = near(n), near(m).astype(queries.dtype)
    elif kind == "lowrange":                      # few distinct values: many exact ties, the id decides
        lo, hi = (0, 4) if dtype == "u8" else (-2, 2)
        base, queries = _rows(rng, n, d, dtype, lo, hi), _queries(rng, m, d, dtype, lo, hi)
    elif kind == "dups":
        base[rng.integers(0, n, n // 3)] = base[int(rng.integers(0, n))]
        queries[0] = base[0]
    eng = _engine(base, metric, dtype)
    ids, dists = eng.query_k_batch(queries, k)
    eng.close()
    _same(ids, dists, *oracle.brute_force(base, queries, k, getattr(oracle, ometric), n_threads=16))
