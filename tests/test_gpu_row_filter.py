"""Row filter of the brute-force engine: while a bitmap over the rows is set, a search returns what
an index holding only the allowed rows, in the same order, would return with its ids mapped back -- ids equal and
distances equal as uint32 bit patterns to the oracle's answer over base[allowed]."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = np.uint64(2 ** 64 - 1)
N, D, M = 65_573, 128, 300


@pytest.fixture(scope="module")
def gpu():
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_device_count() >= 1, "these tests need a HIP device"
    return L


def _engine(base, metric="l2", **opts):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(base.shape[1], metric)
    eng.store_many_vectors(base)
    eng.build()
    for name, val in opts.items():
        eng.set_option(name, val)
    eng.set_profiling(True)
    return eng


def _expected(oracle, base, queries, k, allow, ip=False, id_offset=0):
    """the oracle over the allowed rows only, ids mapped back (PAD stays PAD)"""
    idx = np.flatnonzero(allow)
    m = queries.shape[0]
    if idx.size == 0:
        return np.full((m, k), PAD, np.uint64), np.full((m, k), np.inf, np.float32)
    rids, rd = oracle.brute_force(np.ascontiguousarray(base[idx]), queries, k,
                                  oracle.METRIC_IP_F32 if ip else oracle.METRIC_L2_F32, n_threads=8)
    out = np.full(rids.shape, PAD, np.uint64)
    ok = rids != PAD
    out[ok] = idx[rids[ok].astype(np.int64)].astype(np.uint64) + np.uint64(id_offset)
    return out, rd


def _same(got, want, what=""):
    ids, dists = got
    rids, rd = want
    assert np.array_equal(ids, rids), what
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32)), what


def _random_filter(n, density, seed):
    return np.random.RandomState(seed).rand(n) < density


def _exactly(n, count, seed):
    allow = np.zeros(n, bool)
    allow[np.random.RandomState(seed).choice(n, count, replace=False)] = True
    return allow


@pytest.fixture(scope="module")
def big():
    """the d = 128 index most cases share: rows, queries and one engine whose filter the cases change"""
    rng = np.random.RandomState(4081)
    base = rng.standard_normal((N, D)).astype(np.float32)
    queries = rng.standard_normal((M, D)).astype(np.float32)
    return base, queries


@pytest.fixture(scope="module")
def big_eng(gpu, big):
    eng = _engine(big[0])
    yield eng
    eng.close()


# 1. direct scan ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(3000, 128), (1000, 48)])
def test_small_index_direct_scan(gpu, oracle, n, d):
    rng = np.random.RandomState(n + d)
    base = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((7, d)).astype(np.float32)
    allow = _random_filter(n, 0.5, 1)
    eng = _engine(base)
    eng.set_row_filter(allow)
    assert eng.get_stat("filter_active") == 1 and eng.get_stat("filter_rows") == int(allow.sum())
    _same(eng.query_k_batch(queries, 10), _expected(oracle, base, queries, 10, allow))
    # the bitmap instance of the same kernels (a list capacity below the allowed rows: the threshold ladder)
    eng.set_option("cand_capacity", 256)
    _same(eng.query_k_batch(queries, 10), _expected(oracle, base, queries, 10, allow), "ladder")
    eng.close()


@pytest.mark.parametrize("density", [0.5, 0.05])
def test_direct_ladder_on_a_large_index(big, oracle, density):
    """scan_kernel = 1: the threshold ladder of the exact scan, planned on the allowed rows -- level 0 from an even
    sample of the filter's list (more than 16 384 allowed rows: the list holds every other one), the later levels
    on the bitmap"""
    base, queries = big
    allow = _random_filter(N, density, 21)
    eng = _engine(base, scan_kernel=1)
    eng.set_row_filter(allow)
    got = eng.query_k_batch(queries[:20], 10)
    prof = eng.get_profile()
    _same(got, _expected(oracle, base, queries[:20], 10, allow))
    assert prof["scan_kernel"].startswith("scan_filter_f32") and prof["retries"] == 0, prof
    eng.close()


# 2. matrix-core form at d = 128 ----------------------------------------------------------------
def test_all_ones_equals_the_unfiltered_oracle(big, big_eng, oracle):
    base, queries = big
    big_eng.set_row_filter(np.ones(N, bool))
    assert big_eng.get_stat("filter_rows") == N
    _same(big_eng.query_k_batch(queries, 10), oracle.brute_force(base, queries, 10, oracle.METRIC_L2_F32, n_threads=8))


@pytest.mark.parametrize("density", [0.5, 0.05])
def test_random_filter_runs_the_fp16_form_without_retry(big, big_eng, oracle, density):
    base, queries = big
    allow = _random_filter(N, density, 7)
    big_eng.set_row_filter(allow)
    big_eng.get_profile()
    got = big_eng.query_k_batch(queries, 10)
    prof = big_eng.get_profile()
    _same(got, _expected(oracle, base, queries, 10, allow))
    assert prof["scan_kernel"].startswith("scan_gemm_f16"), prof
    assert prof["retries"] == 0, prof


def test_first_half_disallowed(big, big_eng, oracle):
    base, queries = big
    allow = np.arange(N) >= N // 2
    big_eng.set_row_filter(allow)
    _same(big_eng.query_k_batch(queries, 10), _expected(oracle, base, queries, 10, allow))


def test_only_every_32nd_row(big, oracle):
    """31 of every 32 classes of the sampled pass (chunk, row mod 32) stay empty"""
    base, queries = big
    n = 65_568
    allow = np.arange(n) % 32 == 0
    assert allow.sum() == 2049
    eng = _engine(base[:n])
    eng.set_row_filter(allow)
    got = eng.query_k_batch(queries, 10)
    prof = eng.get_profile()
    _same(got, _expected(oracle, base[:n], queries, 10, allow))
    assert prof["retries"] == 0, prof
    eng.close()


# 3. the other fp16 geometries ---------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 256, 768, 192])
def test_other_fp16_geometries(gpu, oracle, d):
    rng = np.random.RandomState(d)
    n, m = 40_000, 130
    base = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((m, d)).astype(np.float32)
    allow = _random_filter(n, 0.5, d)
    eng = _engine(base, scan_kernel=4)
    eng.set_row_filter(allow)
    got = eng.query_k_batch(queries, 10)
    prof = eng.get_profile()
    _same(got, _expected(oracle, base, queries, 10, allow))
    assert prof["scan_kernel"].startswith("scan_gemm_f16"), prof
    eng.close()


# 4. inner product ---------------------------------------------------------------------------
def test_inner_product(gpu, oracle):
    rng = np.random.RandomState(41)
    n, d, m = 40_000, 128, 130
    base = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((m, d)).astype(np.float32)
    allow = _random_filter(n, 0.3, 4)
    eng = _engine(base, "ip")
    eng.set_row_filter(allow)
    _same(eng.query_k_batch(queries, 10), _expected(oracle, base, queries, 10, allow, ip=True))
    eng.close()


# 5. list path and its boundary ------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 9, 10, 100, 2048, 2049])
def test_very_selective_filters(big, big_eng, oracle, count):
    base, queries = big
    allow = _exactly(N, count, count)
    big_eng.set_row_filter(allow)
    assert big_eng.get_stat("filter_rows") == count
    ids, dists = big_eng.query_k_batch(queries, 10)
    _same((ids, dists), _expected(oracle, base, queries, 10, allow))
    short = min(count, 10)
    assert (ids[:, short:] == PAD).all() and np.isinf(dists[:, short:]).all()
    assert (ids[:, :short] != PAD).all()


# 6. a handful of queries ------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3])
def test_a_handful_of_queries(big, big_eng, oracle, m):
    base, queries = big
    allow = _random_filter(N, 0.5, 7)
    big_eng.set_row_filter(allow)
    _same(big_eng.query_k_batch(queries[:m], 10), _expected(oracle, base, queries[:m], 10, allow))


# 7. k = 100 -------------------------------------------------------------------------------------
def test_k_100(big, big_eng, oracle):
    base, queries = big
    allow = _random_filter(N, 0.2, 100)
    big_eng.set_row_filter(allow)
    _same(big_eng.query_k_batch(queries[:130], 100), _expected(oracle, base, queries[:130], 100, allow))


# 7b. k = 1000 ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def k1000(gpu):
    """70 001 rows of d = 128, 100 queries and one engine for the k = 1000 cases"""
    rng = np.random.RandomState(1000)
    base = rng.standard_normal((70_001, D)).astype(np.float32)
    queries = rng.standard_normal((100, D)).astype(np.float32)
    eng = _engine(base)
    yield base, queries, eng
    eng.close()


def _k1000_case(oracle, k1000, allow, m):
    base, queries, eng = k1000
    eng.set_row_filter(allow)
    assert eng.get_stat("filter_rows") == int(allow.sum())
    eng.get_profile()
    got = eng.query_k_batch(queries[:m], 1000)
    prof = eng.get_profile()
    _same(got, _expected(oracle, base, queries[:m], 1000, allow), prof)
    return got, prof


def test_k_1000_list_regime(oracle, k1000):
    """10 000 allowed rows fit the filter's list (16 384) and are the whole search -- five times the list length
    any k <= 32 ever selects from"""
    _k1000_case(oracle, k1000, _exactly(70_001, 10_000, 1), 100)


@pytest.mark.parametrize("m", [100, 3])
def test_k_1000_ladder_regime(oracle, k1000, m):
    """half the rows allowed: the threshold ladder, planned on the allowed rows"""
    _k1000_case(oracle, k1000, _random_filter(70_001, 0.5, 2), m)


def test_k_1000_padding(oracle, k1000):
    (ids, dists), _ = _k1000_case(oracle, k1000, _exactly(70_001, 600, 3), 100)
    assert (ids[:, :600] != PAD).all() and (ids[:, 600:] == PAD).all() and np.isposinf(dists[:, 600:]).all()


# 8. massive ties ---------------------------------------------------------------------------------
def test_massive_ties(gpu, oracle):
    rng = np.random.RandomState(8)
    n, d = 20_000, 64
    base = np.tile(rng.standard_normal((8, d)).astype(np.float32), (n // 8, 1))
    queries = rng.standard_normal((20, d)).astype(np.float32)
    allow = _random_filter(n, 0.5, 8)
    want = _expected(oracle, base, queries, 10, allow)
    eng = _engine(base)
    eng.set_row_filter(allow)
    _same(eng.query_k_batch(queries, 10), want)
    # the lowest allowed ids of the nearest vector win
    near = want[0][0]
    assert np.array_equal(near, np.sort(near)) and allow[near.astype(np.int64)].all()
    eng.close()


def test_ties_beyond_every_list_capacity(gpu, oracle):
    """20 000 allowed copies of one vector overflow the matrix-core form's lists at every capacity (they cannot
    break ties by row); the retry ends in the exact direct kernel, which reads the filter's bitmap"""
    rng = np.random.RandomState(88)
    n, d, m = 40_000, 64, 130
    base = np.repeat(rng.standard_normal((1, d)).astype(np.float32), n, 0)
    queries = rng.standard_normal((m, d)).astype(np.float32)
    allow = np.zeros(n, bool)
    allow[rng.choice(n, 20_000, replace=False)] = True
    eng = _engine(base)
    eng.set_row_filter(allow)
    got = eng.query_k_batch(queries, 10)
    prof = eng.get_profile()
    _same(got, _expected(oracle, base, queries, 10, allow))
    assert np.array_equal(got[0][0], np.flatnonzero(allow)[:10].astype(np.uint64))
    assert prof["scan_kernel"].startswith("scan_filter_f32"), prof
    eng.close()


# 9. what must be bypassed ------------------------------------------------------------------------
def test_uint8_shortcut_is_bypassed(gpu, oracle):
    rng = np.random.RandomState(9)
    base = rng.randint(0, 256, size=(N, D)).astype(np.float32)
    queries = rng.randint(0, 256, size=(130, D)).astype(np.float32)
    allow = _random_filter(N, 0.5, 9)
    eng = _engine(base)
    eng.set_row_filter(allow)
    _same(eng.query_k_batch(queries, 10), _expected(oracle, base, queries, 10, allow))
    eng.close()


@pytest.mark.parametrize("option,value", [("i8_filter", 2), ("spec_rank", 3)])
def test_int8_filter_and_speculation_are_bypassed(big, oracle, option, value):
    base, queries = big
    allow = _random_filter(N, 0.5, 7)
    eng = _engine(base, **{option: value})
    eng.set_row_filter(allow)
    _same(eng.query_k_batch(queries[:130], 10), _expected(oracle, base, queries[:130], 10, allow))
    assert eng.get_stat("spec_rank") == 10
    eng.close()


# 10. lifecycle -----------------------------------------------------------------------------------
def test_set_change_clear(big, oracle):
    base, queries = big
    a, b = _random_filter(N, 0.5, 1), _random_filter(N, 0.1, 2)
    eng = _engine(base)
    eng.set_row_filter(a)
    _same(eng.query_k_batch(queries, 10), _expected(oracle, base, queries, 10, a), "A")
    eng.set_row_filter(b)
    _same(eng.query_k_batch(queries, 10), _expected(oracle, base, queries, 10, b), "B")
    eng.set_row_filter(None)
    assert eng.get_stat("filter_active") == 0 and eng.get_stat("filter_rows") == N
    _same(eng.query_k_batch(queries, 10), oracle.brute_force(base, queries, 10, oracle.METRIC_L2_F32, n_threads=8),
          "cleared")
    eng.close()


def test_id_offset_and_a_new_base_clears_the_filter(big, oracle):
    import torch
    from expann_amd import GpuBruteForceEngine
    base, queries = big
    n = 40_000
    tb = torch.from_numpy(base[:n]).to("cuda:0")
    torch.cuda.synchronize()
    eng = GpuBruteForceEngine(D, "l2")
    eng.set_base_device(tb.data_ptr(), n, 1000)
    allow = _random_filter(n, 0.5, 3)
    eng.set_row_filter(allow)
    ids, dists = eng.query_k_batch(queries, 10)
    _same((ids, dists), _expected(oracle, base[:n], queries, 10, allow, id_offset=1000))
    assert ids.min() >= 1000
    eng.set_base_device(tb.data_ptr(), n, 1000)
    assert eng.get_stat("filter_active") == 0
    rids, rd = oracle.brute_force(base[:n], queries, 10, oracle.METRIC_L2_F32, n_threads=8)
    _same(eng.query_k_batch(queries, 10), (rids + np.uint64(1000), rd))
    eng.close()


# 11. device buffers, deferred ------------------------------------------------------------------------
def test_deferred_searches_keep_the_filter_they_were_enqueued_under(big, oracle):
    import torch
    from expann_amd import GpuBruteForceEngine, pack_row_filter
    base, queries = big
    dev = torch.device("cuda", 0)
    tb = torch.from_numpy(base).to(dev)
    tq = torch.from_numpy(queries).to(dev)
    a, b = _random_filter(N, 0.5, 11), _random_filter(N, 0.3, 12)
    tbits = torch.from_numpy(pack_row_filter(b).view(np.int32)).to(dev)
    outs = [(torch.empty(M, 10, dtype=torch.int64, device=dev), torch.empty(M, 10, dtype=torch.float32, device=dev))
            for _ in range(2)]
    torch.cuda.synchronize()
    eng = GpuBruteForceEngine(D, "l2")
    eng.set_base_device(tb.data_ptr(), N, 0)
    eng.set_row_filter(a)
    eng.set_option("async_search", 1)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        eng.search_device(tq.data_ptr(), M, 10, outs[0][0].data_ptr(), outs[0][1].data_ptr(), s.cuda_stream)
        eng.set_row_filter_device(tbits.data_ptr(), tbits.numel(), s.cuda_stream)
        assert eng.get_stat("filter_rows") == int(b.sum())
        eng.search_device(tq.data_ptr(), M, 10, outs[1][0].data_ptr(), outs[1][1].data_ptr(), s.cuda_stream)
    eng.sync()
    for (ids, dd), allow, what in zip(outs, (a, b), "AB"):
        _same((ids.cpu().numpy().astype(np.uint64), dd.cpu().numpy()), _expected(oracle, base, queries, 10, allow), what)
    eng.close()


# 12. errors -------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_usable(gpu, oracle):
    from expann_amd import GpuBruteForceEngine, _lib, pack_row_filter
    rng = np.random.RandomState(12)
    n, d = 5000, 128
    # a uint8 index
    b8 = rng.randint(0, 256, size=(n, d)).astype(np.uint8)
    q8 = rng.randint(0, 256, size=(9, d)).astype(np.float32)
    e8 = GpuBruteForceEngine(d, "l2", "u8")
    e8.store_many_vectors(b8)
    e8.build()
    with pytest.raises(_lib.ExpannError) as ei:
        e8.set_row_filter(np.ones(n, bool))
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    _same(e8.query_k_batch(q8, 10), oracle.brute_force(b8, q8, 10, oracle.METRIC_L2_U8, n_threads=4))
    e8.close()
    # before build(), then too few words
    base = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((9, d)).astype(np.float32)
    eng = GpuBruteForceEngine(d, "l2")
    eng.store_many_vectors(base)
    with pytest.raises(_lib.ExpannError) as ei:
        eng.set_row_filter(np.ones(n, bool))
    assert ei.value.code == _lib.ERR_NOT_BUILT
    eng.build()
    words = pack_row_filter(np.ones(n, bool))
    assert gpu.expann_set_row_filter(eng._h, words.ctypes.data, words.size - 1) == _lib.ERR_INVALID_ARG
    assert gpu.expann_set_row_filter(eng._h, None, words.size) == _lib.ERR_INVALID_ARG
    assert eng.get_stat("filter_active") == 0
    _same(eng.query_k_batch(queries, 10), oracle.brute_force(base, queries, 10, oracle.METRIC_L2_F32, n_threads=4))
    eng.close()


# 13. a seeded sweep -------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(int(os.environ.get("EXPANN_FUZZ_FILTER_N", "24"))))
def test_sweep(gpu, oracle, seed):
    rng = np.random.RandomState(9000 + seed)
    n = int(rng.randint(1, 80_001))
    d = int(rng.choice([64, 128, 192, 256]))
    m = int(rng.randint(1, 301))
    k = int(rng.randint(1, 101))
    ip = bool(rng.randint(2))
    density = float(rng.choice([0.001, 0.01, 0.1, 0.5, 0.9, 1]))
    base = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((m, d)).astype(np.float32)
    allow = rng.rand(n) < density
    what = f"seed {seed}: n {n} d {d} m {m} k {k} ip {ip} density {density} allowed {int(allow.sum())}"
    eng = _engine(base, "ip" if ip else "l2")
    eng.set_row_filter(allow)
    assert eng.get_stat("filter_rows") == int(allow.sum()), what
    _same(eng.query_k_batch(queries, k), _expected(oracle, base, queries, k, allow, ip=ip), what)
    eng.close()
