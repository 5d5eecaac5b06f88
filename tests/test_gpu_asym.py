"""Packed-bit rows against int8 queries (expann_search_asym_i8, expann_amd/csrc/scan_asym.hpp) against NumPy in int64:
score = sum q - 2 q . bits.  Every comparison is exact: ids equal, distances equal as float32 bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = np.uint64(2 ** 64 - 1)
TILE = 512  # rows of a tile (kHamTB)


def reference(rows, queries, k, id_offset=0):
    q = queries.astype(np.int64)
    score = q.sum(1)[:, None] - 2 * q @ np.unpackbits(rows, axis=1, bitorder="little").T.astype(np.int64)
    ids = np.full((len(q), k), PAD, dtype=np.uint64)
    dists = np.full((len(q), k), np.inf, dtype=np.float32)
    rid = np.arange(len(rows), dtype=np.int64)
    for j, s in enumerate(score):
        order = np.lexsort((rid, s))[:k]
        ids[j, :len(order)] = (order + id_offset).astype(np.uint64)
        dists[j, :len(order)] = s[order].astype(np.float32)
    return ids, dists


def bits(rng, n, dim):
    return rng.integers(0, 256, (n, dim // 8), dtype=np.uint8)


def int8(rng, m, dim, lo=-128, hi=128):
    return rng.integers(lo, hi, (m, dim), dtype=np.int8)


def engine(rows, dim):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(dim, "hamming", "b1")
    eng.store_many_vectors(rows)
    eng.build()
    return eng


def same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("m", [1, 17, 100])
@pytest.mark.parametrize("dim", [64, 192, 512, 576, 1536, 4096])
def test_chunks_ragged_tiles_and_query_tiles(dim, m):
    """one k-step, no power of two, one chunk, a chunk + a k-step, 3 and 8 chunks; two tiles and a ragged third"""
    n = 2 * TILE + 37
    rng = np.random.default_rng(dim + m)
    rows, queries = bits(rng, n, dim), int8(rng, m, dim)
    want = reference(rows, queries, 300)
    eng = engine(rows, dim)
    for k in (1, 10, 300):
        same(eng.query_k_batch_asym(queries, k), (want[0][:, :k], want[1][:, :k]))
    assert eng.get_stat("asym_mfma_launches") > 0
    eng.close()


def test_extreme_scores_are_exact():
    dim = 4096
    rng = np.random.default_rng(5)
    rows = bits(rng, 700, dim)
    rows[3], rows[650] = 0xFF, 0
    queries = np.stack([np.full(dim, -128, np.int8), np.full(dim, 127, np.int8)])
    got = engine(rows, dim)
    ids, dists = got.query_k_batch_asym(queries, 700)
    got.close()
    same((ids, dists), reference(rows, queries, 700))
    assert dists[0, 0] == -524288.0 and ids[0, 0] == 650 and dists[0, -1] == 524288.0 and ids[0, -1] == 3


def test_ties_end_on_the_lowest_ids():
    dim = 128
    rng = np.random.default_rng(7)
    rows = np.repeat(bits(rng, 1, dim), 5000, axis=0)
    queries = int8(rng, 3, dim)
    eng = engine(rows, dim)
    got = eng.query_k_batch_asym(queries, 10)
    eng.close()
    assert np.array_equal(got[0], np.tile(np.arange(10, dtype=np.uint64), (3, 1)))
    same(got, reference(rows, queries, 10))
    # three codes over 70 000 rows: the threshold ladder runs, and every level meets thousands of ties
    rows = bits(rng, 3, dim)[rng.integers(0, 3, 70_000)]
    queries = int8(rng, 17, dim, -1, 2)
    eng = engine(rows, dim)
    got = eng.query_k_batch_asym(queries, 100)
    eng.close()
    same(got, reference(rows, queries, 100))


def test_sign_queries_rank_as_hamming_does():
    n, dim, m, k = 3000, 256, 33, 10
    rng = np.random.default_rng(9)
    rows, codes = bits(rng, n, dim), bits(rng, m, dim)
    signs = (2 * np.unpackbits(codes, axis=1, bitorder="little").astype(np.int16) - 1).astype(np.int8)
    eng = engine(rows, dim)
    ham_ids, ham_d = eng.query_k_batch(codes, k)
    ids, dists = eng.query_k_batch_asym(signs, k)
    eng.close()
    assert np.array_equal(ids, ham_ids)
    assert np.array_equal(dists, 2 * ham_d - dim)


def test_fewer_rows_than_k_pads_the_tail():
    rng = np.random.default_rng(3)
    rows, queries = bits(rng, 5, 64), int8(rng, 4, 64)
    eng = engine(rows, 64)
    ids, dists = eng.query_k_batch_asym(queries, 10)
    eng.close()
    same((ids, dists), reference(rows, queries, 10))
    assert (ids[:, 5:] == PAD).all() and np.isinf(dists[:, 5:]).all()


def test_refusals_and_their_order():
    """what is wrong by kind or value is named before what is merely not built yet"""
    import ctypes as C
    from expann_amd import GpuBruteForceEngine, _lib
    INVALID_ARG, NOT_BUILT, UNSUPPORTED = _lib.ERR_INVALID_ARG, _lib.ERR_NOT_BUILT, _lib.ERR_UNSUPPORTED
    q = np.zeros((1, 64), np.int8)
    ids = np.zeros((1, 8193), np.uint64)

    def code(eng, queries, k, out=ids):
        return eng._L.expann_search_asym_i8(eng._h, queries.ctypes.data if queries is not None else None, 1, k,
                                            out.ctypes.data if out is not None else None, None)
    i8 = GpuBruteForceEngine(64, "ip", "i8")
    assert code(i8, q, 1) == UNSUPPORTED  # (not built either: the kind comes first)
    i8.close()
    eng = GpuBruteForceEngine(64, "hamming", "b1")
    assert code(eng, q, 8193) == UNSUPPORTED and code(eng, q, 1) == NOT_BUILT
    eng.store_many_vectors(np.zeros((3, 8), np.uint8))
    eng.build()
    assert code(eng, None, 1) == INVALID_ARG and code(eng, q, 1, None) == INVALID_ARG and code(eng, q, 0) == INVALID_ARG
    assert code(eng, q, 8193) == UNSUPPORTED and code(eng, q, 8192) == _lib.OK
    assert eng._L.expann_search_asym_i8_device(eng._h, None, 1, 1, C.c_void_p(ids.ctypes.data), None, None) == INVALID_ARG
    eng.close()


def test_device_rows_with_id_offset_and_device_search():
    import torch
    from expann_amd import GpuBruteForceEngine
    n, dim, m, k, off = 3000, 256, 33, 10, 1 << 33
    rng = np.random.default_rng(11)
    rows, queries = bits(rng, n, dim), int8(rng, m, dim)
    t_rows, tq = torch.from_numpy(rows).cuda(), torch.from_numpy(queries).cuda()
    ids = torch.empty(m, k, dtype=torch.int64, device="cuda")
    dd = torch.empty(m, k, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng = GpuBruteForceEngine(dim, "hamming", "b1")
    eng.set_base_device(t_rows.data_ptr(), n, off)
    eng.search_asym_device(tq.data_ptr(), m, k, ids.data_ptr(), dd.data_ptr(), 0)
    torch.cuda.synchronize()
    host = eng.query_k_batch_asym(queries, k)
    eng.close()
    want = reference(rows, queries, k, off)
    same(host, want)
    same((ids.cpu().numpy().view(np.uint64), dd.cpu().numpy()), want)
