"""The tail of a speculating search: the redo pass filters with tau_r = min(proven tau, S_k'),
S_k' = the k-th exact score of the failed list itself; the waves of its scan that hold no live query slot only
stage; the select stages of the long lists run on a side stream beside the short lists' stage.  None of it changes a
result: ids and distance bits are the oracle's in every case below."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, K = 262_144 + 4_096, 128, 10   # (the smallest index on which the sampled pass reads 1/16 of the rows)


@pytest.fixture(scope="module")
def gpu():
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_device_count() >= 1, "these tests need a HIP device"
    return L


@pytest.fixture(scope="module")
def iid():
    rng = np.random.RandomState(20261)
    return rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((8192, D)).astype(np.float32)


@pytest.fixture(scope="module")
def iid_ref(oracle, iid):
    base, queries = iid
    return oracle.brute_force(base, queries, K, oracle.METRIC_L2_F32, n_threads=16)


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
    return {s: eng.get_stat(s) for s in ("redo_queries", "redo_candidates", "redo_overflows", "spec_rank")}


def _run(base, queries, k, metric="l2", **opts):
    eng = _engine(base, metric, **opts)
    ids, dists = eng.query_k_batch(queries, k)
    prof, st = eng.get_profile(), _stats(eng)
    eng.close()
    return ids, dists, prof, st


def test_bound_on_and_off_agree(gpu, iid, iid_ref):
    """j = 2, 300 queries, both filters: exact with and without the bound, the same queries fail (the main pass is
    the same), and the redo lists with the bound hold no more keys than without -- tau_r <= tau -- and fewer in all.
    (Measured on MI355X, 28 failing queries: int8 filter 1 754 keys against 11 307, ratio 0.155; fp16 form 4 175
    against 4 453, 0.938 -- a query that fails there rarely has k rows in its list, so rarely a bound.)"""
    base, queries = iid
    m = 300
    total = {0: 0, 1: 0}
    for i8_filter in (2, 0):
        st = {}
        for bound in (1, 0):
            ids, dists, prof, st[bound] = _run(base, queries[:m], K, i8_filter=i8_filter, spec_rank=2, redo_bound=bound)
            _same(ids, dists, iid_ref[0][:m], iid_ref[1][:m], (i8_filter, bound, prof, st[bound]))
            assert prof["retries"] == 0 and st[bound]["spec_rank"] == 2, (prof, st[bound])
            total[bound] += st[bound]["redo_candidates"]
        print(f"i8_filter {i8_filter}: redo lists of {st[1]['redo_queries']} queries hold {st[1]['redo_candidates']} keys with "
              f"the bound, {st[0]['redo_candidates']} without ({st[1]['redo_candidates'] / max(1, st[0]['redo_candidates']):.3f})")
        assert st[1]["redo_queries"] == st[0]["redo_queries"] > 0, st
        assert st[1]["redo_candidates"] <= st[0]["redo_candidates"], st
    print(f"both filters: {total[1]} keys with the bound, {total[0]} without ({total[1] / max(1, total[0]):.3f})")
    assert total[1] < total[0], total


@pytest.fixture(scope="module")
def tied(oracle):
    """every row twice (all scores come in equal pairs: whatever S_k' is, another row ties with it exactly at the redo
    threshold), and for the first 40 queries the row of the 5th pair a third time: their 9th, 10th and 11th best are
    byte-identical rows and the k-th place goes to the lower id"""
    rng = np.random.RandomState(77)
    half = rng.standard_normal((N // 2, D)).astype(np.float32)
    queries = rng.standard_normal((600, D)).astype(np.float32)
    h5 = oracle.brute_force(half, queries[:40], 5, oracle.METRIC_L2_F32, n_threads=16)[0][:, 4].astype(np.int64)
    assert len(set(h5.tolist())) == 40
    base = np.concatenate([half, half[h5], half], 0)
    rids, rd = oracle.brute_force(base, queries, K + 1, oracle.METRIC_L2_F32, n_threads=16)
    # the cases are what they are meant to be (checked here, on the CPU): places 9-11 tie bit for bit, the oracle
    # ranks them by id, and the 10th place is the third copy -- the lower id of the 10th / 11th.  (A query whose best
    # rows hold another query's tripled row does not count: there are 40 tripled rows among 133 120.)
    r11 = rd.view(np.uint32)
    good = [i for i in range(40)
            if r11[i, 8] == r11[i, 9] == r11[i, 10] and rids[i, 8] == h5[i] and rids[i, 9] == N // 2 + i
            and rids[i, 10] == N // 2 + 40 + h5[i]]
    assert len(good) >= 35, good
    return base, queries, np.ascontiguousarray(rids[:, :K]), np.ascontiguousarray(rd[:, :K])


@pytest.mark.parametrize("i8_filter", [2, 0])
@pytest.mark.parametrize("rank", [1, 2])
def test_ties_at_the_kth_place_across_the_redo_threshold(gpu, tied, i8_filter, rank):
    base, queries, rids, rd = tied
    m = 300 if rank == 1 else 600   # (j = 1 fails ~44 % of a batch: 300 queries fit the 256 slots)
    ids, dists, prof, st = _run(base, queries[:m], K, i8_filter=i8_filter, spec_rank=rank)
    print(f"i8_filter {i8_filter}, j = {rank}: {st}")
    _same(ids, dists, rids[:m], rd[:m], (prof, st))
    assert prof["retries"] == 0 and st["spec_rank"] == rank and st["redo_queries"] > 0, (prof, st)


@pytest.mark.parametrize("i8_filter", [2, 0])
def test_fewer_than_k_rows_under_the_speculative_threshold(gpu, oracle, iid, i8_filter):
    """j = 1 on 300 queries.  100 of them sit next to five near copies of themselves, planted at random rows: where
    the sample holds one of the five (1 - (15/16)^5 = 28 %) the best sampled row is a copy, the list holds the five
    copies and nothing else -- fewer than k rows, a slot whose bound is +inf and which falls back to the proven tau.
    The other queries fail at the iid rate of j = 1 (44 %); those whose list held k rows (the int8 filter's wider
    slack gives many such lists, the fp16 form's few) have a bound.  The bound never lengthens a list."""
    base, queries = iid
    rng = np.random.RandomState(3)
    base = base.copy()
    q = queries[:300].copy()
    rows = rng.choice(N, 500, replace=False).reshape(100, 5)
    for i in range(100):
        base[rows[i]] = q[i] + np.float32(0.01) * rng.standard_normal((5, D)).astype(np.float32)
    rids, rd = oracle.brute_force(base, q, K, oracle.METRIC_L2_F32, n_threads=16)
    res = {}
    for bound in (1, 0):
        ids, dists, prof, st = _run(base, q, K, i8_filter=i8_filter, spec_rank=1, redo_bound=bound)
        _same(ids, dists, rids, rd, (bound, prof, st))
        assert prof["retries"] == 0 and st["redo_overflows"] == 0, (prof, st)
        res[bound] = st
    print(f"i8_filter {i8_filter}: {res}")
    assert res[1]["redo_queries"] == res[0]["redo_queries"] >= 20, res   # (~28 planted + ~90 iid)
    assert res[1]["redo_candidates"] <= res[0]["redo_candidates"], res     # (tau_r <= tau)


def test_inner_product_and_dim_64(gpu, oracle):
    """the bound is a score in true units: inner product with ip_rescale (the filter sees c_q q, so the bound passes
    through qscale) and d = 64 (the fp16 form's own redo instance), j = 2, with and without the bound"""
    rng = np.random.RandomState(65)
    for d, metric, om in ((128, "ip", "METRIC_IP_F32"), (64, "l2", "METRIC_L2_F32")):
        base = rng.standard_normal((N, d)).astype(np.float32)
        queries = rng.standard_normal((400, d)).astype(np.float32)
        if metric == "ip":
            queries *= rng.uniform(0.01, 30.0, (400, 1)).astype(np.float32)
        rids, rd = oracle.brute_force(base, queries, K, getattr(oracle, om), n_threads=16)
        res = {}
        for bound in (1, 0):
            opts = {"ip_rescale": 1} if metric == "ip" else {}
            ids, dists, prof, st = _run(base, queries, K, metric, spec_rank=2, redo_bound=bound, **opts)
            _same(ids, dists, rids, rd, (d, metric, bound, prof, st))
            assert prof["retries"] == 0 and st["redo_queries"] > 0, (d, metric, prof, st)
            res[bound] = st
        print(f"d {d} {metric}: {res}")
        assert res[1]["redo_queries"] == res[0]["redo_queries"], res
        assert res[1]["redo_candidates"] <= res[0]["redo_candidates"], res   # (tau_r <= tau; equal when no failed list held k rows)


@pytest.mark.parametrize("i8_filter", [2, 0])
@pytest.mark.parametrize("m,rank,lo,hi", [(2048, 2, 65, 256), (300, 2, 1, 64), (300, 9, 0, 0)])
def test_live_wave_groups_of_the_redo_tile(gpu, iid, iid_ref, i8_filter, m, rank, lo, hi):
    """j = 2 fails P(Bin(9, 1/16) >= 2) = 10.5 % of a batch: ~215 of 2 048 queries -- all four wave groups of the redo
    tile's 256 slots hold queries, the last one partly -- and ~31 of 300: wave group 0 alone multiplies, the other
    three only stage.  j = 9: nobody fails and every workgroup of the redo scan leaves at once."""
    base, queries = iid
    ids, dists, prof, st = _run(base, queries[:m], K, i8_filter=i8_filter, spec_rank=rank)
    print(f"i8_filter {i8_filter}, {m} queries, j = {rank}: {st}")
    _same(ids, dists, iid_ref[0][:m], iid_ref[1][:m], (prof, st))
    assert prof["retries"] == 0 and st["spec_rank"] == rank and st["redo_overflows"] == 0, (prof, st)
    assert lo <= st["redo_queries"] <= hi, st
    if hi == 0:
        assert st["redo_candidates"] == 0, st


def test_both_select_stages_and_the_redo_pass_in_one_search(gpu, iid, iid_ref, capfd, monkeypatch):
    """4 096 queries on the int8 filter with j = 3: the lists reach past 512 keys (the second wave stage has work --
    read from the library's own report of the list lengths) and ~1.5 % of the batch fails, so the redo pass follows
    the join of the two streams; one stream and two give the same exact results"""
    base, queries = iid
    m = 4096
    monkeypatch.setenv("EXPANN_DEBUG_LISTS", "1")
    res = {}
    for overlap in (1, 0):
        capfd.readouterr()
        ids, dists, prof, st = _run(base, queries[:m], K, i8_filter=2, spec_rank=3, select_overlap=overlap)
        longest = [int(x) for x in re.findall(r"\[lists\] attempt 0 .* max (\d+),", capfd.readouterr().err)]
        print(f"select_overlap {overlap}: longest list {longest}, {st}")
        _same(ids, dists, iid_ref[0][:m], iid_ref[1][:m], (overlap, prof, st))
        assert prof["retries"] == 0 and st["redo_overflows"] == 0 and st["redo_queries"] > 0, (prof, st)
        assert longest and longest[0] > 512, longest
        res[overlap] = (ids, dists, st)
    assert np.array_equal(res[1][0], res[0][0]) and np.array_equal(res[1][1].view(np.uint32), res[0][1].view(np.uint32))
    assert res[1][2] == res[0][2], res


def test_interleaved_deferred_searches_join_the_side_stream(gpu, iid, iid_ref):
    """the same search three times back to back in the deferred form, on two different batches (A, B, A), one
    expann_sync: a search's long-list stages have joined the caller's stream before the next search's sampled pass
    zeroes the counters and reuses the lists"""
    import torch
    base, queries = iid
    m = 4096
    dev = torch.device("cuda", 0)
    eng = _engine(base, i8_filter=2, spec_rank=3, async_search=1)
    eng.set_profiling(False)
    s = torch.cuda.Stream(device=dev)
    outs = []
    with torch.cuda.stream(s):
        for lo in (0, m, 0):
            tq = torch.from_numpy(queries[lo:lo + m]).to(dev)
            ids = torch.empty(m, K, dtype=torch.int64, device=dev)
            dd = torch.empty(m, K, dtype=torch.float32, device=dev)
            eng.search_device(tq.data_ptr(), m, K, ids.data_ptr(), dd.data_ptr(), s.cuda_stream)
            outs.append((lo, tq, ids, dd))
    eng.sync()
    st = _stats(eng)
    eng.close()
    print(f"three deferred searches: {st}")
    for lo, _, ids, dd in outs:
        _same(ids.cpu().numpy().astype(np.uint64), dd.cpu().numpy(), iid_ref[0][lo:lo + m], iid_ref[1][lo:lo + m], (lo, st))
    assert st["redo_queries"] > 0 and st["redo_overflows"] == 0 and st["redo_candidates"] > 0, st


def test_rank_one_still_overflows_the_redo_pass(gpu, iid, iid_ref):
    """j = 1 fails 44 % of 4 096 queries, far more than the 256 slots: the overflow is reported and the search is
    repeated with proven thresholds, as before the bound"""
    base, queries = iid
    m = 4096
    ids, dists, prof, st = _run(base, queries[:m], K, spec_rank=1)
    _same(ids, dists, iid_ref[0][:m], iid_ref[1][:m], (prof, st))
    assert prof["retries"] >= 1 and st["redo_overflows"] >= 1, (prof, st)
    assert st["spec_rank"] == K, st
