"""4-bit product-quantised rows (EXPANN_DTYPE_PQ4, expann_amd/csrc/scan_pq4.hpp) against THE PQ4 RULE of
include/expann_hip.h restated in float32 NumPy.  Every comparison is exact: ids equal, distances equal as float32 bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = np.uint64(2 ** 64 - 1)
TILE = 512  # rows of a tile of scan_pq4_mfma_kernel
F = np.float32


def reference(codebooks, codes, queries, k, metric, id_offset=0):
    """THE PQ4 RULE, one float32 operation at a time.  codes are unpacked, [n, M] in [0, 15]."""
    M, _, dsub = codebooks.shape
    q = np.asarray(queries, F).reshape(len(queries), M, 1, dsub)
    T = np.zeros((len(queries), M, 16), F)
    for j in range(dsub):  # step 1
        if metric == "l2":
            t = q[..., j] - codebooks[None, :, :, j]
            T = T + t * t
        else:
            T = T + q[..., j] * codebooks[None, :, :, j]
    if metric == "ip":
        T = F(0) - T
    lo = T.min(axis=2)  # step 2
    span = (T.max(axis=2) - lo).max(axis=1)
    safe = np.where(span > 0, span, F(1))
    r = np.where(span > 0, F(255) / safe, F(0)).astype(F)  # step 3
    step = np.where(span > 0, safe / F(255), F(0)).astype(F)
    u = np.minimum(F(255), np.rint((T - lo[:, :, None]) * r[:, None, None])).astype(np.int64)  # step 4
    bias = lo[:, 0]  # step 5
    for i in range(1, M):
        bias = bias + lo[:, i]
    S = np.zeros((len(queries), len(codes)), np.int64)  # step 6
    for i in range(M):
        S += u[:, i, codes[:, i]]
    dist = bias[:, None] + step[:, None] * S.astype(F)  # step 7
    ids, dists = np.full((len(queries), k), PAD, dtype=np.uint64), np.full((len(queries), k), np.inf, dtype=F)
    rid = np.arange(len(codes), dtype=np.int64)
    for j, s in enumerate(S):
        order = np.lexsort((rid, s))[:k]
        ids[j, :len(order)] = (order + id_offset).astype(np.uint64)
        dists[j, :len(order)] = dist[j, order]
    return ids, dists


def same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def engine(codebooks, codes, metric):
    from expann_amd import GpuBruteForceEngine, pack_pq4
    M, _, dsub = codebooks.shape
    eng = GpuBruteForceEngine(M * dsub, metric, "pq4", codebooks=codebooks)
    eng.store_many_vectors(pack_pq4(codes))
    eng.build()
    return eng


def gaussian(rng, M, dsub, n, m):
    return (rng.standard_normal((M, 16, dsub)).astype(F), rng.integers(0, 16, (n, M), dtype=np.uint8),
            rng.standard_normal((m, M * dsub)).astype(F))


@pytest.mark.parametrize("m", [1, 65, 100])
@pytest.mark.parametrize("dsub", [1, 3, 8])
@pytest.mark.parametrize("M", [16, 32, 48, 64, 80, 128, 256])
def test_every_m_class_at_ragged_ends(M, dsub, m):
    """the tables of a query tile stay in LDS up to M = 128 (kPQ4ResidentMaxM) and stream through two stages above it:
    128 and 256 are the two sides of that boundary"""
    n = 2 * TILE + 37
    cb, codes, queries = gaussian(np.random.default_rng(1000 * M + 10 * dsub + m), M, dsub, n, m)
    for metric in ("l2", "ip"):
        want = reference(cb, codes, queries, 300, metric)
        eng = engine(cb, codes, metric)
        assert eng.size() == n and eng.get_stat("base_bytes") == n * M // 2 and eng.get_stat("pq_m") == M
        for k in (1, 10, 300):
            same(eng.query_k_batch(queries, k), (want[0][:, :k], want[1][:, :k]))
        assert eng.get_stat("pq4_launches") > 0
        eng.close()


@pytest.mark.parametrize("M,dsub", [(16, 1), (48, 2), (256, 4)])
def test_nibble_and_centroid_order(M, dsub):
    """centroid c of sub-quantiser i is the constant c + 16 i, the query is ones in sub-vector i0 alone: r = 17 / dsub
    is exact, S = 17 (15 - code_i0) -- a swapped nibble, axis or sub-quantiser changes the order of the ids"""
    rng = np.random.default_rng(M)
    cb = np.broadcast_to((np.arange(16) + 16.0 * np.arange(M)[:, None])[:, :, None], (M, 16, dsub)).astype(F)
    codes = rng.integers(0, 16, (300, M), dtype=np.uint8)
    picks = [0, 1, M // 2, M - 2, M - 1]
    queries = np.zeros((len(picks), M * dsub), F)
    for row, i0 in enumerate(picks):
        queries[row, i0 * dsub:(i0 + 1) * dsub] = 1.0
    eng = engine(cb, codes, "ip")
    ids, dists = eng.query_k_batch(queries, 300)
    eng.close()
    same((ids, dists), reference(cb, codes, queries, 300, "ip"))
    for row, i0 in enumerate(picks):
        assert np.array_equal(ids[row].astype(np.int64), np.lexsort((np.arange(300), -codes[:, i0].astype(np.int64))))


@pytest.mark.parametrize("kind", ["ties", "decades"])
def test_quantisation_edges(kind):
    """ties: integer centroids in [0, 510], both ends in one sub-quantiser, r = 0.5, odd entries round half to even.
    decades: one sub-quantiser sets the step.  The all-zero query has span = 0: ids 0 .. k-1 and +0.0, never -0.0."""
    M, n, k = 32, 2 * TILE + 37, 50
    rng = np.random.default_rng(3)
    cb, codes, _ = gaussian(rng, M, 1, n, 1)
    if kind == "ties":
        cb = rng.integers(0, 511, (M, 16, 1)).astype(F)
        cb[0, 0], cb[0, 1] = 0.0, 510.0
    else:
        cb *= (10.0 ** (np.arange(M) % 9 - 4)).astype(F)[:, None, None]
    queries = np.stack([np.ones(M, F), np.zeros(M, F)])
    eng = engine(cb, codes, "ip")
    ids, dists = eng.query_k_batch(queries, k)
    eng.close()
    same((ids, dists), reference(cb, codes, queries, k, "ip"))
    assert np.array_equal(ids[1], np.arange(k, dtype=np.uint64)) and (dists[1].view(np.uint32) == 0).all()


@pytest.mark.parametrize("k", [10, 6000])
def test_ties_end_on_the_lowest_ids_and_padding(k):
    M, dsub = 16, 8
    rng = np.random.default_rng(7)
    cb, three, queries = gaussian(rng, M, dsub, 3, 5)
    codes = three[rng.integers(0, 3, 5000)]
    for metric in ("l2", "ip"):
        eng = engine(cb, codes, metric)
        ids, dists = eng.query_k_batch(queries, k)
        eng.close()
        same((ids, dists), reference(cb, codes, queries, k, metric))
        assert (ids[:, 5000:] == PAD).all() and np.isinf(dists[:, 5000:]).all()


@pytest.mark.parametrize("k", [10, 100])
def test_threshold_levels(k):
    M, dsub, n, m = 32, 4, 70_000, 64
    cb, codes, queries = gaussian(np.random.default_rng(k), M, dsub, n, m)
    eng = engine(cb, codes, "l2")
    got = eng.query_k_batch(queries, k)
    levels, launches = eng.get_profile()["levels"], eng.get_stat("pq4_launches")
    eng.close()
    assert levels >= 2 and launches >= levels  # a thresholded level ran, on this kernel
    same(got, reference(cb, codes, queries, k, "l2"))


def test_device_rows_with_id_offset_and_device_search():
    import torch
    from expann_amd import GpuBruteForceEngine, pack_pq4
    M, dsub, n, m, k, off = 48, 3, 3000, 33, 10, 1 << 33
    cb, codes, queries = gaussian(np.random.default_rng(11), M, dsub, n, m)
    t_rows, tq = torch.from_numpy(pack_pq4(codes)).cuda(), torch.from_numpy(queries).cuda()
    ids, dd = torch.empty(m, k, dtype=torch.int64, device="cuda"), torch.empty(m, k, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng = GpuBruteForceEngine(M * dsub, "ip", "pq4", codebooks=cb)
    eng.set_base_device(t_rows.data_ptr(), n, off)
    eng.search_device(tq.data_ptr(), m, k, ids.data_ptr(), dd.data_ptr(), 0)
    torch.cuda.synchronize()
    host = eng.query_k_batch(queries, k)
    eng.close()
    want = reference(cb, codes, queries, k, "ip", off)
    same(host, want)
    same((ids.cpu().numpy().view(np.uint64), dd.cpu().numpy()), want)


def test_what_is_not_offered_is_refused_and_leaves_the_handle_as_it_was():
    from expann_amd import GpuBruteForceEngine, _lib, pack_pq4
    M, dsub = 16, 2
    cb, codes, queries = gaussian(np.random.default_rng(13), M, dsub, 100, 4)
    for kw in ({}, {"codebooks": np.zeros((8, 16, 4), F)}, {"codebooks": np.zeros((M, 256, dsub), F)}):  # missing; M = 8; 256 centroids
        with pytest.raises((ValueError, _lib.ExpannError)):
            GpuBruteForceEngine(32, "l2", "pq4", **kw)
    eng = engine(cb, codes, "l2")
    for call in (lambda: eng.store_many_vectors(pack_pq4(codes[:1])), lambda: eng.reserve(200), lambda: eng.remove([0]),
                 eng.compact_row_filter, lambda: eng.score_ids(queries[0], [0]),
                 lambda: eng.query_k_batch_asym(np.zeros((1, 32), np.int8), 1),
                 lambda: eng.range_search(queries[:1], 1.0, 5),
                 lambda: eng.set_row_filter(np.ones(100, bool)), lambda: eng.set_row_groups(np.zeros(100, np.uint32))):
        with pytest.raises(_lib.ExpannError) as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED and "EXPANN_DTYPE_PQ4 rows" in str(e.value)
    assert eng.size() == 100
    got = eng.query_k_batch(queries, 10)
    eng.close()
    same(got, reference(cb, codes, queries, 10, "l2"))
