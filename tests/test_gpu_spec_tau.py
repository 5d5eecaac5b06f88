"""Speculative thresholds: the full scan filters with the j-th largest class maximum of the sampled
pass instead of the k-th, the select checks every query's result against that threshold, and the failing queries
are searched again on the device with the proven one.  Whatever j is, ids and distance bits are the oracle's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D = 262_144 + 4_096, 128   # (the sampled pass reads 1/16 of the rows from 262 144 rows on)


@pytest.fixture(scope="module")
def gpu():
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_device_count() >= 1, "these tests need a HIP device"
    return L


@pytest.fixture(scope="module")
def iid():
    rng = np.random.RandomState(20260)
    return rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((4096, D)).astype(np.float32)


@pytest.fixture(scope="module")
def iid_ref(oracle, iid):
    base, queries = iid
    return oracle.brute_force(base, queries, 10, oracle.METRIC_L2_F32, n_threads=16)


def _engine(base, metric="l2", **opts):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(base.shape[1], metric)
    eng.store_many_vectors(base)
    eng.build()
    for name, val in opts.items():
        eng.set_option(name, val)
    eng.set_profiling(True)
    return eng


def _same(ids, dists, rids, rd, what=""):
    assert np.array_equal(ids, rids), what
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32)), what


def _stats(eng):
    return {s: eng.get_stat(s) for s in ("redo_queries", "redo_overflows", "spec_rank")}


@pytest.mark.parametrize("i8_filter", [2, 0])
@pytest.mark.parametrize("rank", ["default", "auto rank forced"])
def test_iid_rows_few_queries_need_the_redo_pass(gpu, iid, iid_ref, i8_filter, rank):
    """iid rows, 4 096 queries, k = 10: exact, no retry, and at most 2 % of the batch served by the redo pass (the
    binomial tail puts j = 4 at 0.15 %, the CPU model of 1 024 queries at 0.29 %) -- with the planner's own choice
    (it speculates on the int8 filter and keeps the fp16 form at k = 10 on proven thresholds) and with the auto
    rank forced on"""
    base, queries = iid
    m, k = 4096, 10
    j = gpu.expann_spec_rank_auto(k, 16)
    assert j < k
    eng = _engine(base, i8_filter=i8_filter, spec_rank=0 if rank == "default" else j)
    ids, dists = eng.query_k_batch(queries[:m], k)
    prof, st = eng.get_profile(), _stats(eng)
    eng.close()
    print(f"i8_filter {i8_filter}, {rank}: candidates per query {prof['candidates'] / m:.1f}, {st}")
    _same(ids, dists, iid_ref[0][:m], iid_ref[1][:m], (prof, st))
    assert prof["retries"] == 0 and st["redo_overflows"] == 0, (prof, st)
    assert st["redo_queries"] <= 0.02 * m, st
    if rank != "default" or i8_filter == 2:
        assert st["spec_rank"] == j, st


@pytest.mark.parametrize("i8_filter", [2, 0])
def test_rank_two_fails_tens_of_queries_and_the_redo_pass_serves_them(gpu, iid, iid_ref, i8_filter):
    base, queries = iid
    m, k = 300, 10
    eng = _engine(base, i8_filter=i8_filter, spec_rank=2)
    ids, dists = eng.query_k_batch(queries[:m], k)
    prof, st = eng.get_profile(), _stats(eng)
    eng.close()
    print(f"i8_filter {i8_filter}, j = 2: {st}")
    _same(ids, dists, iid_ref[0][:m], iid_ref[1][:m], (prof, st))
    assert prof["retries"] == 0 and st["spec_rank"] == 2, (prof, st)
    assert 0 < st["redo_queries"] <= 256, st   # (P(Bin(9, 1/16) >= 2) = 10.5 %: ~30 of 300, one query tile of slots)


def test_rank_one_overflows_the_redo_pass(gpu, iid, iid_ref):
    """j = 1: the best sampled row beats the 10th best of the index for 1 - (15/16)^9 = 44 % of the queries, far more
    than the redo pass's 256 slots for 4 096 queries.  The waiting form repeats the search with proven thresholds;
    the deferred form reports at expann_sync and the repeat with async_search = 0 is exact."""
    import torch
    base, queries = iid
    m, k = 4096, 10
    eng = _engine(base, spec_rank=1)
    ids, dists = eng.query_k_batch(queries[:m], k)
    prof, st = eng.get_profile(), _stats(eng)
    _same(ids, dists, iid_ref[0][:m], iid_ref[1][:m], (prof, st))
    assert prof["retries"] >= 1 and st["redo_overflows"] >= 1, (prof, st)
    assert st["spec_rank"] == k, st   # (the attempt that produced the results ran on proven thresholds)
    dev = torch.device("cuda", 0)
    tq = torch.from_numpy(queries[:m]).to(dev)
    tid = torch.empty(m, k, dtype=torch.int64, device=dev)
    td = torch.empty(m, k, dtype=torch.float32, device=dev)
    s = torch.cuda.Stream(device=dev)
    eng.set_option("async_search", 1)
    eng.search_device(tq.data_ptr(), m, k, tid.data_ptr(), td.data_ptr(), s.cuda_stream)
    with pytest.raises(RuntimeError):
        eng.sync()
    eng.set_option("async_search", 0)
    eng.search_device(tq.data_ptr(), m, k, tid.data_ptr(), td.data_ptr(), s.cuda_stream)
    s.synchronize()
    _same(tid.cpu().numpy().astype(np.uint64), td.cpu().numpy(), iid_ref[0][:m], iid_ref[1][:m])
    eng.close()


@pytest.mark.parametrize("i8_filter", [2, 0])
@pytest.mark.parametrize("k,rank", [(5, 2), (10, 4), (10, 2), (16, 3)])
def test_ties_across_the_threshold(gpu, oracle, i8_filter, k, rank):
    """every row has an identical twin, so the scores come in equal pairs -- at odd k the k-th and (k+1)-th score
    are equal -- and one row is there 40 times (a block of identical rows longer than k) with queries beside it:
    exact, the id order of the ties included"""
    rng = np.random.RandomState(31 + k)
    half = rng.standard_normal((140_000, D)).astype(np.float32)
    block = np.repeat(rng.standard_normal((1, D)).astype(np.float32), 40, 0)
    base = np.concatenate([half, block, half], 0)
    queries = rng.standard_normal((600, D)).astype(np.float32)
    queries[:20] = block[0] + np.float32(0.02) * rng.standard_normal((20, D)).astype(np.float32)
    queries[20:40] = half[:20] + np.float32(0.05) * rng.standard_normal((20, D)).astype(np.float32)
    eng = _engine(base, i8_filter=i8_filter, spec_rank=rank)
    ids, dists = eng.query_k_batch(queries, k)
    prof, st = eng.get_profile(), _stats(eng)
    eng.close()
    rids, rd = oracle.brute_force(base, queries, k, oracle.METRIC_L2_F32, n_threads=16)
    _same(ids, dists, rids, rd, (prof, st))
    assert st["spec_rank"] == rank, st


@pytest.mark.parametrize("i8_filter", [2, 0])
def test_fewer_than_k_rows_under_the_speculative_threshold(gpu, oracle, i8_filter):
    """k = 100 on 40 000 rows with j = 3: the third best of the 41 % sample admits a handful of rows, every query
    fails the check for want of k rows, and the redo pass (one tile of slots for 200 queries) serves them all; the
    batch is not a multiple of the query tile"""
    rng = np.random.RandomState(5)
    base = rng.standard_normal((40_000, D)).astype(np.float32)
    queries = rng.standard_normal((200, D)).astype(np.float32)
    eng = _engine(base, i8_filter=i8_filter, spec_rank=3)
    ids, dists = eng.query_k_batch(queries, 100)
    prof, st = eng.get_profile(), _stats(eng)
    eng.close()
    rids, rd = oracle.brute_force(base, queries, 100, oracle.METRIC_L2_F32, n_threads=16)
    _same(ids, dists, rids, rd, (prof, st))
    assert prof["retries"] == 0 and st["redo_queries"] > 100, (prof, st)


@pytest.mark.parametrize("n,m,k", [(50, 70, 64), (33_000, 257, 10), (70_001, 513, 10), (65_600, 1025, 1)])
def test_small_indexes_odd_batches_and_k_beyond_n(gpu, oracle, n, m, k):
    rng = np.random.RandomState(n + m)
    base = rng.standard_normal((n, D)).astype(np.float32)
    queries = rng.standard_normal((m, D)).astype(np.float32)
    eng = _engine(base, spec_rank=2)
    ids, dists = eng.query_k_batch(queries, k)
    prof, st = eng.get_profile(), _stats(eng)
    eng.close()
    rids, rd = oracle.brute_force(base, queries, k, oracle.METRIC_L2_F32, n_threads=16)
    _same(ids, dists, rids, rd, (prof, st))


def test_inner_product_and_dim_64(gpu, oracle):
    """the check compares in true units: inner product (the filter sees c_q q, ip_rescale) and d = 64"""
    rng = np.random.RandomState(64)
    for d, metric, om in ((128, "ip", "METRIC_IP_F32"), (64, "l2", "METRIC_L2_F32")):
        base = rng.standard_normal((N, d)).astype(np.float32)
        queries = rng.standard_normal((400, d)).astype(np.float32)
        if metric == "ip":   # (L2 queries of another magnitude than the rows leave the fp16 filter's range: another path)
            queries *= rng.uniform(0.01, 30.0, (400, 1)).astype(np.float32)
        eng = _engine(base, metric, spec_rank=2)
        ids, dists = eng.query_k_batch(queries, 10)
        prof, st = eng.get_profile(), _stats(eng)
        eng.close()
        rids, rd = oracle.brute_force(base, queries, 10, getattr(oracle, om), n_threads=16)
        _same(ids, dists, rids, rd, (d, metric, prof, st))
        assert prof["retries"] == 0 and st["redo_queries"] > 0, (d, metric, prof, st)


# candidates of the parent build (proven thresholds only) for the first 2 048 queries of the iid fixture, k = 10
PARENT_CANDIDATES = {2: 918418, 0: 362235}


@pytest.mark.parametrize("i8_filter", [2, 0])
def test_rank_k_is_the_parent_scan(gpu, iid, iid_ref, i8_filter):
    """spec_rank >= k: proven thresholds, the same lists as before speculation existed -- the candidate count of the
    parent build on these seeded inputs, exactly"""
    base, queries = iid
    m, k = 2048, 10
    eng = _engine(base, i8_filter=i8_filter, spec_rank=k)
    ids, dists = eng.query_k_batch(queries[:m], k)
    prof, st = eng.get_profile(), _stats(eng)
    eng.close()
    print(f"i8_filter {i8_filter}, j = k: candidates {prof['candidates']}")
    _same(ids, dists, iid_ref[0][:m], iid_ref[1][:m], (prof, st))
    assert prof["candidates"] == PARENT_CANDIDATES[i8_filter], prof
    assert st == {"redo_queries": 0, "redo_overflows": 0, "spec_rank": k}, st


def test_interleaved_deferred_searches_keep_their_own_redo_lists(gpu, iid, oracle):
    """several deferred searches of different batches back to back on one stream with j = 2: each has failing
    queries, each search's redo pass writes its own rows"""
    import torch
    base, queries = iid
    k = 10
    rng = np.random.RandomState(9)
    qs = [queries[0:300], queries[300:400], rng.standard_normal((700, D)).astype(np.float32), queries[1000:1257],
          queries[0:300]]
    dev = torch.device("cuda", 0)
    tb = torch.from_numpy(base).to(dev)
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(D, "l2")
    eng.set_base_device(tb.data_ptr(), base.shape[0], 0)
    eng.set_option("spec_rank", 2)
    eng.set_option("async_search", 1)
    s = torch.cuda.Stream(device=dev)
    outs = []
    with torch.cuda.stream(s):
        for q in qs:
            tq = torch.from_numpy(q).to(dev)
            ids = torch.empty(q.shape[0], k, dtype=torch.int64, device=dev)
            dd = torch.empty(q.shape[0], k, dtype=torch.float32, device=dev)
            eng.search_device(tq.data_ptr(), q.shape[0], k, ids.data_ptr(), dd.data_ptr(), s.cuda_stream)
            outs.append((tq, ids, dd))
    eng.sync()
    st = _stats(eng)
    for q, (_, ids, dd) in zip(qs, outs):
        rids, rd = oracle.brute_force(base, q, k, oracle.METRIC_L2_F32, n_threads=16)
        _same(ids.cpu().numpy().astype(np.uint64), dd.cpu().numpy(), rids, rd)
    assert st["redo_queries"] >= 5 and st["redo_overflows"] == 0, st   # (~10 % of 1 657 queries)
    eng.close()
