"""Product-quantised rows (EXPANN_DTYPE_PQ8, expann_amd/csrc/scan_pq.hpp) against THE PQ RULE of include/expann_hip.h
restated in float32 NumPy.  Every comparison is exact: ids equal, distances equal as float32 bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = np.uint64(2 ** 64 - 1)
STEP = 256  # rows of a workgroup step


def reference(codebooks, codes, queries, k, metric, id_offset=0):
    """THE PQ RULE: tables over j in order, the sum over i in order, one float32 operation at a time."""
    M, _, dsub = codebooks.shape
    q = np.asarray(queries, np.float32).reshape(len(queries), M, 1, dsub)
    T = np.zeros((len(queries), M, 256), np.float32)
    for j in range(dsub):
        if metric == "l2":
            t = q[..., j] - codebooks[None, :, :, j]
            T = T + t * t
        else:
            T = T + q[..., j] * codebooks[None, :, :, j]
    S = T[:, 0, codes[:, 0]]
    for i in range(1, M):
        S = S + T[:, i, codes[:, i]]
    score = S if metric == "l2" else np.float32(0) - S
    ids = np.full((len(queries), k), PAD, dtype=np.uint64)
    dists = np.full((len(queries), k), np.inf, dtype=np.float32)
    rid = np.arange(len(codes), dtype=np.int64)
    for j, s in enumerate(score):
        order = np.lexsort((rid, s))[:k]
        ids[j, :len(order)] = (order + id_offset).astype(np.uint64)
        dists[j, :len(order)] = s[order]
    return ids, dists


def same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def engine(codebooks, codes, metric):
    from expann_amd import GpuBruteForceEngine
    M, _, dsub = codebooks.shape
    eng = GpuBruteForceEngine(M * dsub, metric, "pq8", codebooks=codebooks)
    eng.store_many_vectors(codes)
    eng.build()
    return eng


def gaussian(rng, M, dsub, n, m):
    return (rng.standard_normal((M, 256, dsub)).astype(np.float32), rng.integers(0, 256, (n, M), dtype=np.uint8),
            rng.standard_normal((m, M * dsub)).astype(np.float32))


@pytest.mark.parametrize("m", [1, 9, 100])
@pytest.mark.parametrize("dsub", [1, 3, 8])
@pytest.mark.parametrize("M", [8, 16, 24, 32, 64, 72, 128])
def test_every_tile_class_at_ragged_ends(M, dsub, m):
    n = 2 * STEP + 37
    cb, codes, queries = gaussian(np.random.default_rng(1000 * M + 10 * dsub + m), M, dsub, n, m)
    for metric in ("l2", "ip"):
        want = reference(cb, codes, queries, 300, metric)
        eng = engine(cb, codes, metric)
        assert eng.size() == n and eng.get_stat("base_bytes") == n * M and eng.get_stat("pq_m") == M
        for k in (1, 10, 300):
            same(eng.query_k_batch(queries, k), (want[0][:, :k], want[1][:, :k]))
        assert eng.get_stat("pq_launches") > 0
        eng.close()


@pytest.mark.parametrize("M,dsub", [(8, 2), (24, 1), (128, 4)])
def test_code_and_centroid_order(M, dsub):
    """centroid c of sub-quantiser i is the constant c + 256 i; a query of ones in sub-vector i0 alone scores
    -dsub (code_i0 + 256 i0) under the inner product -- a swapped axis or a wrong byte changes every score"""
    rng = np.random.default_rng(M)
    cb = np.broadcast_to((np.arange(256) + 256.0 * np.arange(M)[:, None])[:, :, None], (M, 256, dsub)).astype(np.float32)
    codes = rng.integers(0, 256, (300, M), dtype=np.uint8)
    picks = [0, 1, M // 2, M - 2, M - 1]
    queries = np.zeros((len(picks), M * dsub), np.float32)
    for r, i0 in enumerate(picks):
        queries[r, i0 * dsub:(i0 + 1) * dsub] = 1.0
    eng = engine(cb, codes, "ip")
    ids, dists = eng.query_k_batch(queries, 300)
    eng.close()
    same((ids, dists), reference(cb, codes, queries, 300, "ip"))
    for r, i0 in enumerate(picks):
        assert np.array_equal(dists[r], -np.float32(dsub) * (codes[ids[r].astype(np.int64), i0] + np.float32(256 * i0)))


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_summation_order(metric):
    """table entries over eight decades: a tree or a reversed sum differs in the last bits"""
    M, dsub = 64, 4
    cb, codes, queries = gaussian(np.random.default_rng(5), M, dsub, 2 * STEP + 37, 9)
    cb *= (10.0 ** (np.arange(M) % 9 - 4)).astype(np.float32)[:, None, None]
    eng = engine(cb, codes, metric)
    got = eng.query_k_batch(queries, 100)
    eng.close()
    same(got, reference(cb, codes, queries, 100, metric))


@pytest.mark.parametrize("k", [10, 6000])
def test_ties_end_on_the_lowest_ids_and_zero_is_positive(k):
    M, dsub = 16, 8
    rng = np.random.default_rng(7)
    cb, three, queries = gaussian(rng, M, dsub, 3, 5)
    codes = three[rng.integers(0, 3, 5000)]
    queries[4] = 0.0
    for metric in ("l2", "ip"):
        eng = engine(cb, codes, metric)
        ids, dists = eng.query_k_batch(queries, k)
        eng.close()
        same((ids, dists), reference(cb, codes, queries, k, metric))
        assert (ids[:, 5000:] == PAD).all() and np.isinf(dists[:, 5000:]).all()
    assert np.array_equal(ids[4, :10], np.arange(10, dtype=np.uint64))
    assert (dists[4, :min(k, 5000)].view(np.uint32) == 0).all()  # inner product, all-zero query: +0.0, never -0.0


@pytest.mark.parametrize("sample_pass", [0, 1])
@pytest.mark.parametrize("k", [10, 100])
def test_threshold_levels(k, sample_pass):
    """70 000 rows: the ladder from a keep-all level 0 ("sample_pass" 0) and from the sampled class minima (1)"""
    M, dsub, n, m = 16, 8, 70_000, 64
    cb, codes, queries = gaussian(np.random.default_rng(k), M, dsub, n, m)
    eng = engine(cb, codes, "l2")
    eng.set_option("sample_pass", sample_pass)
    got = eng.query_k_batch(queries, k)
    levels, launches = eng.get_profile()["levels"], eng.get_stat("pq_launches")
    eng.close()
    assert levels >= 2 and launches >= levels  # a thresholded level ran, on this kernel
    same(got, reference(cb, codes, queries, k, "l2"))


def test_device_rows_with_id_offset_and_device_search():
    import torch
    from expann_amd import GpuBruteForceEngine
    M, dsub, n, m, k, off = 24, 3, 3000, 33, 10, 1 << 33
    cb, codes, queries = gaussian(np.random.default_rng(11), M, dsub, n, m)
    t_rows, tq = torch.from_numpy(codes).cuda(), torch.from_numpy(queries).cuda()
    ids = torch.empty(m, k, dtype=torch.int64, device="cuda")
    dd = torch.empty(m, k, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng = GpuBruteForceEngine(M * dsub, "ip", "pq8", codebooks=cb)
    eng.set_base_device(t_rows.data_ptr(), n, off)
    eng.search_device(tq.data_ptr(), m, k, ids.data_ptr(), dd.data_ptr(), 0)
    torch.cuda.synchronize()
    host = eng.query_k_batch(queries, k)
    eng.close()
    want = reference(cb, codes, queries, k, "ip", off)
    same(host, want)
    same((ids.cpu().numpy().view(np.uint64), dd.cpu().numpy()), want)


def test_what_is_not_offered_is_refused_and_leaves_the_handle_as_it_was():
    from expann_amd import GpuBruteForceEngine, _lib
    M, dsub = 8, 2
    cb, codes, queries = gaussian(np.random.default_rng(13), M, dsub, 100, 4)
    for kw in ({"dtype": "pq8"}, {"dtype": "f32", "codebooks": cb}, {"dtype": "pq8", "codebooks": np.zeros((4, 256, 4), np.float32)}):  # (M = 4)
        with pytest.raises((ValueError, _lib.ExpannError)):
            GpuBruteForceEngine(16, "l2", **kw)
    eng = engine(cb, codes, "l2")
    with pytest.raises(ValueError):
        eng.store_many_vectors(np.zeros((1, M + 8), np.uint8))
    for call in (lambda: eng.store_many_vectors(codes[:1]), lambda: eng.reserve(200), lambda: eng.remove([0]),
                 eng.compact_row_filter, lambda: eng.score_ids(queries[0], [0]),
                 lambda: eng.query_k_batch_asym(np.zeros((1, 16), np.int8), 1),
                 lambda: eng.range_search(queries[:1], 1.0, 5),
                 lambda: eng.set_row_filter(np.ones(100, bool)), lambda: eng.set_row_groups(np.zeros(100, np.uint32))):
        with pytest.raises(_lib.ExpannError) as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED and "EXPANN_DTYPE_PQ8 rows" in str(e.value)
    assert eng.size() == 100
    got = eng.query_k_batch(queries, 10)
    eng.close()
    same(got, reference(cb, codes, queries, 10, "l2"))
