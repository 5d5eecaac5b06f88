"""Packed-bit rows under the Hamming distance (EXPANN_DTYPE_B1, expann_amd/csrc/scan_hamming.hpp): the VALU form
("scan_kernel" 1) and the form on the int8 matrix cores (2) against a NumPy count of the differing bits.  Every
comparison is exact: ids equal, distances equal as float32 bits."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = np.uint64(2 ** 64 - 1)
_HPP = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "expann_amd", "csrc",
                         "scan_hamming.hpp")).read()
VALU_ROWS = int(re.search(r"kHamValuRows = (\d+);", _HPP).group(1))  # rows of a workgroup step, form 1
MFMA_ROWS = int(re.search(r"kHamTB == (\d+),", _HPP).group(1))       # rows of a tile, form 2
STAT = {1: "hamming_valu_launches", 2: "hamming_mfma_launches"}


def reference(rows, queries, k, id_offset=0):
    b = np.unpackbits(rows, axis=1, bitorder="little")
    ids = np.full((len(queries), k), PAD, dtype=np.uint64)
    dists = np.full((len(queries), k), np.inf, dtype=np.float32)
    rid = np.arange(len(rows), dtype=np.int64)
    for j, q in enumerate(np.unpackbits(queries, axis=1, bitorder="little")):
        score = (b != q).sum(axis=1, dtype=np.int64)
        order = np.lexsort((rid, score))[:k]
        ids[j, :len(order)] = (order + id_offset).astype(np.uint64)
        dists[j, :len(order)] = score[order].astype(np.float32)
    return ids, dists


def bits(rng, n, dim):
    return rng.integers(0, 256, (n, dim // 8), dtype=np.uint8)


def engine(rows, dim, scan_kernel=0):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(dim, "hamming", "b1")
    eng.store_many_vectors(rows)
    eng.build()
    eng.set_option("scan_kernel", scan_kernel)
    return eng


def same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def ran(eng, form):
    assert eng.get_stat(STAT[form]) > 0 and eng.get_stat(STAT[3 - form]) == 0


@pytest.mark.parametrize("m", [1, 17, 100])
@pytest.mark.parametrize("form,dim", [(2, 64), (2, 192), (2, 512), (2, 1024), (1, 64), (1, 192), (1, 512), (1, 1024),
                                      (1, 1088), (1, 4096)])
def test_both_forms_at_ragged_tiles_and_query_tiles(form, dim, m):
    n = 2 * (MFMA_ROWS if form == 2 else VALU_ROWS) + 37
    rng = np.random.default_rng(dim + m)
    rows, queries = bits(rng, n, dim), bits(rng, m, dim)
    want = reference(rows, queries, 300)
    eng = engine(rows, dim, form)
    assert eng.size() == n and eng.get_stat("base_bytes") == n * dim // 8
    for k in (1, 10, 300):
        same(eng.query_k_batch(queries, k), (want[0][:, :k], want[1][:, :k]))
    ran(eng, form)
    eng.close()


def test_the_matrix_core_form_ends_at_1024_bits():
    rows = bits(np.random.default_rng(1), 100, 1088)
    eng = engine(rows, 1088, 2)
    with pytest.raises(RuntimeError):
        eng.query_k_batch(rows[:2], 1)
    eng.close()


@pytest.mark.parametrize("m,form", [(4095, 1), (4096, 2)])
def test_auto_picks_by_batch(m, form):
    """both sides of the auto rule at 65 536 rows (bf_plan.hpp); every 64th query against the reference"""
    n, dim, k = 65_536, 256, 10
    rng = np.random.default_rng(m)
    rows, queries = bits(rng, n, dim), bits(rng, m, dim)
    eng = engine(rows, dim)
    ids, dists = eng.query_k_batch(queries, k)
    ran(eng, form)
    eng.close()
    same((ids[::64], dists[::64]), reference(rows, queries[::64], k))


@pytest.mark.parametrize("form", [1, 2])
def test_ties_end_on_the_lowest_ids(form):
    dim = 128
    rng = np.random.default_rng(7)
    # (a) identical rows: ids 0..9, one score
    rows = np.repeat(bits(rng, 1, dim), 5000, axis=0)
    queries = bits(rng, 3, dim)
    eng = engine(rows, dim, form)
    ids, dists = eng.query_k_batch(queries, 10)
    eng.close()
    assert np.array_equal(ids, np.tile(np.arange(10, dtype=np.uint64), (3, 1)))
    assert (dists == dists[:, :1]).all()
    same((ids, dists), reference(rows, queries, 10))
    # (b) three codes over 70 000 rows, (c) two queries that are stored rows: score 0 first
    codes = bits(rng, 3, dim)
    rows = codes[rng.integers(0, 3, 70_000)]
    queries = np.concatenate([bits(rng, 15, dim), codes[:2]])
    eng = engine(rows, dim, form)
    got = eng.query_k_batch(queries, 100)
    ran(eng, form)
    eng.close()
    same(got, reference(rows, queries, 100))
    assert (got[1][-2:, 0] == 0).all()


@pytest.mark.parametrize("form", [1, 2])
def test_fewer_rows_than_k_pads_the_tail(form):
    rng = np.random.default_rng(3)
    rows, queries = bits(rng, 5, 64), bits(rng, 4, 64)
    eng = engine(rows, 64, form)
    ids, dists = eng.query_k_batch(queries, 10)
    eng.close()
    same((ids, dists), reference(rows, queries, 10))
    assert (ids[:, 5:] == PAD).all() and np.isinf(dists[:, 5:]).all()


@pytest.mark.parametrize("form", [1, 2])
def test_device_rows_with_id_offset_and_device_search(form):
    import torch
    from expann_amd import GpuBruteForceEngine
    n, dim, m, k, off = 3000, 256, 33, 10, 1 << 33
    rng = np.random.default_rng(11)
    rows, queries = bits(rng, n, dim), bits(rng, m, dim)
    t_rows, tq = torch.from_numpy(rows).cuda(), torch.from_numpy(queries).cuda()
    ids = torch.empty(m, k, dtype=torch.int64, device="cuda")
    dd = torch.empty(m, k, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng = GpuBruteForceEngine(dim, "hamming", "b1")
    eng.set_base_device(t_rows.data_ptr(), n, off)
    eng.set_option("scan_kernel", form)
    eng.search_device(tq.data_ptr(), m, k, ids.data_ptr(), dd.data_ptr(), 0)
    torch.cuda.synchronize()
    host = eng.query_k_batch(queries, k)
    eng.close()
    want = reference(rows, queries, k, off)
    same(host, want)
    same((ids.cpu().numpy().view(np.uint64), dd.cpu().numpy()), want)
