"""4-bit rows against int8 queries (EXPANN_DTYPE_I4, expann_amd/csrc/scan_i4.hpp) against NumPy in int64 on the
unpacked rows, ranked by (float32(score), id).  Every comparison is exact: ids equal, distances equal as float32 bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = np.uint64(2 ** 64 - 1)
TILE = 512  # rows of a tile (kHamTB)
KC = 128    # elements of a stage (kI4KC)
METRICS = ["ip", "l2"]


def reference(rows, queries, k, metric, id_offset=0):
    from expann_amd import unpack_i4
    q, b = queries.astype(np.int64), unpack_i4(rows).astype(np.int64)
    score = -(q @ b.T)
    if metric == "l2":
        score = (q * q).sum(1)[:, None] + 2 * score + (b * b).sum(1)[None, :]
    ids = np.full((len(q), k), PAD, dtype=np.uint64)
    dists = np.full((len(q), k), np.inf, dtype=np.float32)
    rid = np.arange(len(rows), dtype=np.int64)
    for j, s in enumerate(score):
        order = np.lexsort((rid, s.astype(np.float32)))[:k]
        ids[j, :len(order)] = (order + id_offset).astype(np.uint64)
        dists[j, :len(order)] = s[order].astype(np.float32)
    return ids, dists


def nibbles(rng, n, dim):
    from expann_amd import pack_i4
    return pack_i4(rng.integers(-8, 8, (n, dim), dtype=np.int8))


def int8(rng, m, dim):
    return rng.integers(-128, 128, (m, dim), dtype=np.int8)


def engine(rows, dim, metric, dtype="i4"):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(dim, metric, dtype)
    eng.store_many_vectors(rows)
    eng.build()
    return eng


def same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def search(rows, queries, k, metric):
    eng = engine(rows, queries.shape[1], metric)
    got = eng.query_k_batch(queries, k)
    eng.close()
    return got


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m", [1, 17, 100])
@pytest.mark.parametrize("dim", sorted({64, 192, KC, KC + 64, 1536, 4096}))
def test_chunks_ragged_tiles_and_query_tiles(dim, m, metric):
    """one k-step, no power of two, one chunk, a chunk + a k-step, many chunks; two tiles and a ragged third"""
    n = 2 * TILE + 37
    rng = np.random.default_rng(dim + m)
    rows, queries = nibbles(rng, n, dim), int8(rng, m, dim)
    want = reference(rows, queries, 300, metric)
    eng = engine(rows, dim, metric)
    for k in (1, 10, 300):
        same(eng.query_k_batch(queries, k), (want[0][:, :k], want[1][:, :k]))
    assert eng.get_stat("i4_mfma_launches") > 0 and eng.get_stat("base_bytes") == n * dim // 2
    eng.close()


@pytest.mark.parametrize("metric", METRICS)
def test_nibble_order_and_sign(metric):
    """a query that is nonzero at one element: a wrong permutation or a swapped low / high nibble changes the score"""
    from expann_amd import pack_i4
    dim = 64
    rng = np.random.default_rng(2)
    values = rng.integers(-8, 8, (40, dim), dtype=np.int8)
    values[0, 0::2], values[0, 1::2] = 7, -8
    values[1, 0::2], values[1, 1::2] = -8, 7
    queries = np.zeros((16, dim), np.int8)
    queries[np.arange(16), 16 + np.arange(16)] = 100 + np.arange(16)
    rows = pack_i4(values)
    same(search(rows, queries, 40, metric), reference(rows, queries, 40, metric))


@pytest.mark.parametrize("metric", METRICS)
def test_extreme_scores_are_exact(metric):
    from expann_amd import pack_i4
    dim = 4096
    rng = np.random.default_rng(5)
    values = rng.integers(-8, 8, (700, dim), dtype=np.int8)
    values[3], values[650] = -8, 7
    rows = pack_i4(values)
    queries = np.stack([np.full(dim, -128, np.int8), np.full(dim, 127, np.int8)])
    ids, dists = search(rows, queries, 700, metric)
    same((ids, dists), reference(rows, queries, 700, metric))
    if metric == "ip":
        assert (ids[0, 0], dists[0, 0], ids[0, -1], dists[0, -1]) == (3, -4096 * 128 * 8, 650, 4096 * 128 * 7)
        assert (ids[1, 0], dists[1, 0], ids[1, -1], dists[1, -1]) == (650, -4096 * 127 * 7, 3, 4096 * 127 * 8)


@pytest.mark.parametrize("metric", METRICS)
def test_ties_end_on_the_lowest_ids(metric):
    dim = 128
    rng = np.random.default_rng(7)
    rows = np.repeat(nibbles(rng, 1, dim), 5000, axis=0)
    queries = int8(rng, 3, dim)
    got = search(rows, queries, 10, metric)
    assert np.array_equal(got[0], np.tile(np.arange(10, dtype=np.uint64), (3, 1)))
    same(got, reference(rows, queries, 10, metric))
    # three codes over 70 000 rows: the threshold ladder runs, and every level meets thousands of ties
    rows = nibbles(rng, 3, dim)[rng.integers(0, 3, 70_000)]
    queries = int8(rng, 17, dim)
    same(search(rows, queries, 100, metric), reference(rows, queries, 100, metric))


def test_fewer_rows_than_k_pads_the_tail():
    rng = np.random.default_rng(3)
    rows, queries = nibbles(rng, 5, 64), int8(rng, 4, 64)
    ids, dists = search(rows, queries, 10, "l2")
    same((ids, dists), reference(rows, queries, 10, "l2"))
    assert (ids[:, 5:] == PAD).all() and np.isinf(dists[:, 5:]).all()


def test_device_rows_with_id_offset_and_device_search():
    import torch
    from expann_amd import GpuBruteForceEngine
    n, dim, m, k, off = 3000, 256, 33, 10, 1 << 33
    rng = np.random.default_rng(11)
    rows, queries = nibbles(rng, n, dim), int8(rng, m, dim)
    t_rows, tq = torch.from_numpy(rows).cuda(), torch.from_numpy(queries).cuda()
    ids = torch.empty(m, k, dtype=torch.int64, device="cuda")
    dd = torch.empty(m, k, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng = GpuBruteForceEngine(dim, "l2", "i4")
    eng.set_base_device(t_rows.data_ptr(), n, off)
    eng.search_device(tq.data_ptr(), m, k, ids.data_ptr(), dd.data_ptr(), 0)
    torch.cuda.synchronize()
    host = eng.query_k_batch(queries, k)
    eng.close()
    want = reference(rows, queries, k, "l2", off)
    same(host, want)
    same((ids.cpu().numpy().view(np.uint64), dd.cpu().numpy()), want)


def test_what_is_not_offered_is_refused_and_leaves_the_handle_as_it_was():
    from expann_amd import _lib
    rng = np.random.default_rng(13)
    rows, queries = nibbles(rng, 100, 64), int8(rng, 4, 64)
    eng = engine(rows, 64, "ip")
    for call in (lambda: eng.store_many_vectors(rows[:1]), lambda: eng.reserve(200), lambda: eng.remove([0]),
                 eng.compact_row_filter, lambda: eng.score_ids(queries[0], [0]), lambda: eng.query_k_batch_asym(queries, 1),
                 lambda: eng.range_search(np.zeros((1, 64), np.float32), 1.0, 5),
                 lambda: eng.set_row_filter(np.ones(100, bool)), lambda: eng.set_row_groups(np.zeros(100, np.uint32))):
        with pytest.raises(_lib.ExpannError) as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED
    assert eng.size() == 100
    got = eng.query_k_batch(queries, 10)
    eng.close()
    same(got, reference(rows, queries, 10, "ip"))


@pytest.mark.parametrize("metric,dim", [("ip", 64), ("ip", 1536), ("l2", 64), ("l2", 896)])
def test_equal_to_an_i8_engine_over_the_unpacked_rows(metric, dim):
    from expann_amd import unpack_i4
    rng = np.random.default_rng(dim)
    rows, queries = nibbles(rng, 3000, dim), int8(rng, 33, dim)
    i8 = engine(unpack_i4(rows), dim, metric, "i8")
    want = i8.query_k_batch(queries, 10)
    i8.close()
    same(search(rows, queries, 10, metric), want)
