"""The sampled pass of a speculating int8-filter search on the int8 matrix cores (option "i8_sample", DESIGN.md 4.4i /
4.6; scan_gemm_i8f.hpp, "Sampled pass on int8"): tau_s is the centre of the j-th class maximum's int8 interval -- an
estimate the select checks -- and the proven tau of the redo pass comes from the same maxima.  Ids and distance bits
are the oracle's whichever pass gave the thresholds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, K = 262_144 + 4_096, 128, 10   # (the smallest index the 1/16 sample serves)
I8F = "scan_gemm_i8w<128,F32L2>"


@pytest.fixture(scope="module")
def gpu():
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_device_count() >= 1, "these tests need a HIP device"
    return L


@pytest.fixture(scope="module")
def iid():
    rng = np.random.RandomState(20261)
    return rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((4096, D)).astype(np.float32)


@pytest.fixture(scope="module")
def iid_ref(oracle, iid):
    base, queries = iid
    return oracle.brute_force(base, queries, K, oracle.METRIC_L2_F32, n_threads=16)


def _engine(base, **opts):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(base.shape[1], "l2")
    eng.store_many_vectors(base)
    eng.build()
    eng.set_option("i8_filter", 2)
    for name, val in opts.items():
        eng.set_option(name, val)
    eng.set_profiling(True)
    return eng


def _same(ids, dists, rids, rd, what=""):
    assert np.array_equal(ids, rids), what
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32)), what


def _stats(eng):
    return {s: eng.get_stat(s) for s in ("redo_queries", "redo_candidates", "redo_overflows", "spec_rank", "i8_sample")}


def _run(base, queries, k, **opts):
    eng = _engine(base, **opts)
    ids, dists = eng.query_k_batch(queries, k)
    prof, st = eng.get_profile(), _stats(eng)
    eng.close()
    return ids, dists, prof, st


def test_auto_speculation(gpu, iid, iid_ref):
    """4 096 queries (the smallest batch that speculates on auto), i8_sample 1 and 0: both exact with no retry and no
    redo overflow, at most 2 % of the batch in the redo pass (the numpy model, profiles/i8_sample_model.py: 0.39 %),
    and the int8 pass's lists at most 1.5 x the fp16 pass's (the model: 1.00; thresholds from the int8 UPPER bound,
    which this pass must not be, give 2.6)"""
    base, queries = iid
    m = 4096
    j = gpu.expann_spec_rank_auto(K, 16)
    cand = {}
    for i8_sample in (1, 0):
        ids, dists, prof, st = _run(base, queries, K, i8_sample=i8_sample)
        cand[i8_sample] = prof["candidates"] / m
        print(f"i8_sample {i8_sample}: candidates per query {cand[i8_sample]:.1f}, {st}")
        _same(ids, dists, iid_ref[0], iid_ref[1], (i8_sample, prof, st))
        assert prof["scan_kernel"] == I8F and prof["retries"] == 0 and st["redo_overflows"] == 0, (prof, st)
        assert st["i8_sample"] == i8_sample and st["spec_rank"] == j, st
        assert st["redo_queries"] <= 0.02 * m, st
    print(f"candidates per query: int8 pass {cand[1]:.1f}, fp16 pass {cand[0]:.1f} ({cand[1] / cand[0]:.3f})")
    assert cand[1] <= 1.5 * cand[0], cand


def test_fewer_than_k_rows_fall_to_the_proven_tau_of_the_int8_pass(gpu, oracle, iid):
    """j = 1 on 300 queries, 100 of them next to five near copies of themselves planted at random rows: where the
    sample holds a copy the list holds the five copies and nothing else -- fewer than k rows, no bound from the failed
    list, and the redo pass filters with the proven tau the int8 pass made from its k-th class maximum"""
    base, queries = iid
    rng = np.random.RandomState(3)
    base = base.copy()
    q = queries[:300].copy()
    rows = rng.choice(N, 500, replace=False).reshape(100, 5)
    for i in range(100):
        base[rows[i]] = q[i] + np.float32(0.01) * rng.standard_normal((5, D)).astype(np.float32)
    rids, rd = oracle.brute_force(base, q, K, oracle.METRIC_L2_F32, n_threads=16)
    ids, dists, prof, st = _run(base, q, K, i8_sample=2, spec_rank=1)
    print(f"fewer than k rows: retries {prof['retries']}, {st}")
    _same(ids, dists, rids, rd, (prof, st))
    assert prof["retries"] == 0 and st["redo_overflows"] == 0, (prof, st)
    assert st["i8_sample"] == 1 and st["spec_rank"] == 1 and st["redo_queries"] >= 20, st   # (~28 planted + ~90 iid)


def test_ties_among_class_maxima_and_across_tau_s(gpu, oracle):
    """every row has an identical twin (equal class maxima, scores in equal pairs across tau_s) and one row is there
    40 times with queries beside it: exact, the id order of the ties included"""
    rng = np.random.RandomState(31 + K)
    half = rng.standard_normal((140_000, D)).astype(np.float32)
    block = np.repeat(rng.standard_normal((1, D)).astype(np.float32), 40, 0)
    base = np.concatenate([half, block, half], 0)
    queries = rng.standard_normal((600, D)).astype(np.float32)
    queries[:20] = block[0] + np.float32(0.02) * rng.standard_normal((20, D)).astype(np.float32)
    queries[20:40] = half[:20] + np.float32(0.05) * rng.standard_normal((20, D)).astype(np.float32)
    rids, rd = oracle.brute_force(base, queries, K, oracle.METRIC_L2_F32, n_threads=16)
    ids, dists, prof, st = _run(base, queries, K, i8_sample=2, spec_rank=2)
    print(f"ties: retries {prof['retries']}, {st}")
    _same(ids, dists, rids, rd, (prof, st))
    assert st["i8_sample"] == 1 and st["spec_rank"] == 2, st


def test_clamped_rows_and_clipped_queries(gpu, oracle, iid):
    """eight rows scaled by 1e4 (bp clamped: no interval, no centre term -- never a class maximum), a query equal to
    one of them and a query scaled by 100 (clipped) among 254 ordinary ones: exact, a retry allowed (as
    tests/test_gpu_i8_filter.py allows for queries far beyond the clip).  256 ordinary queries on the same rows: exact
    with no retry.  (Eight such rows lift the index's rms from 1 to ~54; the scale comes from the rms of the
    components within the clip when those hold less than 1/16 of the energy -- DESIGN.md 4.4i, "Known limit" -- so the
    ordinary rows keep s ~ 0.043.)"""
    base, queries = iid
    base = base.copy()
    big = np.array([11, 4_097, 65_536, 100_003, 123_457, 200_000, 262_143, N - 1])
    base[big] *= np.float32(1e4)
    q = queries[:256].copy()
    q[100] = base[big[4]]
    q[200] *= np.float32(100.0)
    plain = queries[256:512]
    for name, batch, retry_ok in (("clamped row's twin and a clipped query", q, True), ("ordinary queries", plain, False)):
        rids, rd = oracle.brute_force(base, batch, K, oracle.METRIC_L2_F32, n_threads=16)
        ids, dists, prof, st = _run(base, batch, K, i8_sample=2, spec_rank=4)
        print(f"{name}: retries {prof['retries']}, {prof['scan_kernel']}, candidates per query "
              f"{prof['candidates'] / len(batch):.1f}, {st}")
        _same(ids, dists, rids, rd, (name, prof, st))
        if not retry_ok:
            assert prof["retries"] == 0 and st["i8_sample"] == 1, (name, prof, st)


def test_deferred_search_on_device_buffers(gpu, iid, iid_ref):
    """async_search = 1 and expann_sync, auto: the int8 pass, exact"""
    import torch
    base, queries = iid
    m = 4096
    dev = torch.device("cuda", 0)
    tb = torch.from_numpy(base).to(dev)
    tq = torch.from_numpy(queries).to(dev)
    tid = torch.empty(m, K, dtype=torch.int64, device=dev)
    td = torch.empty(m, K, dtype=torch.float32, device=dev)
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(D, "l2")
    eng.set_base_device(tb.data_ptr(), N, 0)
    eng.set_option("i8_filter", 2)
    eng.set_option("async_search", 1)
    s = torch.cuda.Stream(device=dev)
    eng.search_device(tq.data_ptr(), m, K, tid.data_ptr(), td.data_ptr(), s.cuda_stream)
    eng.sync()
    st = _stats(eng)
    eng.close()
    _same(tid.cpu().numpy().astype(np.uint64), td.cpu().numpy(), iid_ref[0], iid_ref[1], st)
    assert st["i8_sample"] == 1 and st["redo_overflows"] == 0, st
