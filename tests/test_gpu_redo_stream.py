"""The redo pass of the int8 filter (expann_amd/csrc/scan_redo_i8.hpp): redo_stream_i8_kernel reads
the int8 copy in a streaming loop -- every wave one contiguous range of 16-row columns -- and files its own hits
into the redo lists.  Forced with i8_filter = 2 and spec_rank = j; ids and distance bits are the CPU oracle's in every
case, no tolerance.

Small indexes on purpose: below 262 144 rows the sampled pass reads 16 384 rows whatever N is -- half of 32 768 rows,
41 % of 40 037 -- so a query fails the check of rank j at about P(Bin(k - 1, share) >= j): nearly always at j = 1,
half of the time at j = 5, a few per cent at j = 8.  The live counts below were observed on MI355X with these seeds
and are asserted by class."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, K = 128, 10
I8F = "scan_gemm_i8w<128,F32L2>"   # the int8 filter's main scan as expann_profile names it
SIZES = (32_768, 33_000, 40_037)   # the int8 forms' minimum; a multiple of 8 but not of 64; not a multiple of 16
STATS = ("redo_queries", "redo_candidates", "redo_overflows", "spec_rank")


@pytest.fixture(scope="module")
def gpu():
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_device_count() >= 1, "these tests need a HIP device"
    return L


@pytest.fixture(scope="module")
def iid(oracle):
    """one iid base per N with 600 queries and their exact results, computed once"""
    out = {}
    for n in SIZES:
        rng = np.random.RandomState(n)
        base = rng.standard_normal((n, D)).astype(np.float32)
        queries = rng.standard_normal((600, D)).astype(np.float32)
        out[n] = (base, queries) + tuple(oracle.brute_force(base, queries, K, oracle.METRIC_L2_F32, n_threads=16))
    return out


def _engine(base, **opts):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(base.shape[1], "l2")
    eng.store_many_vectors(base)
    eng.build()
    for name, val in opts.items():
        eng.set_option(name, val)
    eng.set_profiling(True)
    return eng


def _same(ids, dists, rids, rd, what=""):
    assert np.array_equal(ids, rids), what
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32)), what


def _run(base, queries, **opts):
    eng = _engine(base, i8_filter=2, **opts)
    ids, dists = eng.query_k_batch(queries, K)
    prof, st = eng.get_profile(), {s: eng.get_stat(s) for s in STATS}
    eng.close()
    assert prof["retries"] > 0 or prof["scan_kernel"] == I8F, prof   # (a retry may end on the fp16 form)
    return ids, dists, prof, st


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("rank", [5, 7])
def test_ragged_row_counts(gpu, iid, n, rank):
    """300 queries at j = 5 (observed: 135, 130 and 70 fail at the three sizes -- two or three walks, one per 64-slot
    block) and j = 7 (14, 24, 11: one walk).
    32 768 rows are 2 048 columns, fewer than the grid has waves: most waves have an empty range; 33 000 rows end
    24 rows into a 64-row tile, 40 037 rows end 5 rows into a column: padding rows and a partial last column, which
    must not appear in a result."""
    base, queries, rids, rd = iid[n]
    m = 300
    ids, dists, prof, st = _run(base, queries[:m], spec_rank=rank)
    print(f"N {n}, j = {rank}: {st}")
    assert ids.max() < n, ids.max()
    _same(ids, dists, rids[:m], rd[:m], (prof, st))
    assert prof["retries"] == 0 and st["spec_rank"] == rank and st["redo_overflows"] == 0, (prof, st)
    assert 0 < st["redo_queries"] <= 256 and st["redo_candidates"] > 0, st


@pytest.mark.parametrize("m,rank,lo,hi", [(300, 7, 1, 16), (300, 6, 17, 64), (300, 4, 65, 256), (300, 3, 65, 256),
                                          (100, 9, 0, 0)])
def test_live_count_classes(gpu, iid, m, rank, lo, hi):
    """N = 40 037.  1-16 live slots: one query group is multiplied; 17-64: several groups in one walk of the rows;
    65-256: several walks, one per 64-slot block; 0: every wave leaves at once and nothing is filed.
    Observed on MI355X, 300 queries: j = 8: 1 fails, j = 7: 11, j = 6: 35, j = 5: 70, j = 4: 144 (three walks, the
    last with one query group), j = 3: 216 (four walks); j = 1, 2: more than the 256 slots.  100 queries, j = 9: 0."""
    base, queries, rids, rd = iid[40_037]
    ids, dists, prof, st = _run(base, queries[:m], spec_rank=rank)
    print(f"{m} queries, j = {rank}: {st}")
    _same(ids, dists, rids[:m], rd[:m], (prof, st))
    assert prof["retries"] == 0 and st["spec_rank"] == rank and st["redo_overflows"] == 0, (prof, st)
    assert lo <= st["redo_queries"] <= hi, st
    if hi == 0:
        assert st["redo_candidates"] == 0, st


def test_more_failing_queries_than_slots(gpu, iid):
    """j = 1 on 32 768 rows fails nearly every one of 600 queries, more than the 256 slots: the overflow is reported
    and the search is repeated with proven thresholds"""
    base, queries, rids, rd = iid[32_768]
    ids, dists, prof, st = _run(base, queries, spec_rank=1)
    print(f"j = 1, 600 queries: retries {prof['retries']}, {st}")
    _same(ids, dists, rids, rd, (prof, st))
    assert prof["retries"] >= 1 and st["redo_overflows"] >= 1, (prof, st)
    assert st["spec_rank"] == K, st


N_BIG, REDO_CAP = 262_144 + 4_096, 256


def test_a_redo_list_beyond_its_capacity(gpu, oracle, capfd, monkeypatch):
    """No capacity does this on the small indexes above: their sampled pass reads 41-50 % of the rows, so the proven
    threshold is tight and the redo lists (43 keys on average with redo_bound = 0) are shorter than the main lists
    (89 at most at j = 7).  N_BIG is the smallest index on which the sampled pass reads 1/16 of the rows: there the
    main lists of j = 1 are short and the proven-threshold lists of the redo pass several hundred keys long.
    First at the default capacity, where the library's own report gives the longest main list and the stats the mean
    redo list: REDO_CAP lies between them, so at cand_capacity = REDO_CAP the main lists fit and a redo list cannot.
    The kernel keeps counting and drops the keys, the select reports cnt > cap, the search is repeated and is exact.
    The failing queries fit the 256 slots in the first run (no retry there), so the overflow is a list's.
    Observed on MI355X: the longest main list holds 243 keys, the mean redo list more than 256."""
    rng = np.random.RandomState(20262)
    base = rng.standard_normal((N_BIG, D)).astype(np.float32)
    queries = rng.standard_normal((300, D)).astype(np.float32)
    rids, rd = oracle.brute_force(base, queries, K, oracle.METRIC_L2_F32, n_threads=16)
    monkeypatch.setenv("EXPANN_DEBUG_LISTS", "1")
    report = r"\[lists\] attempt 0 cap (\d+): .* max (\d+), overflow flag (\d+)"
    capfd.readouterr()
    ids, dists, prof, st = _run(base, queries, spec_rank=1, redo_bound=0)
    first = re.search(report, capfd.readouterr().err)
    print(f"default capacity: {st}, main lists: {first and first.groups()}")
    _same(ids, dists, rids, rd, (prof, st))
    assert prof["retries"] == 0 and 0 < st["redo_queries"] <= 256 and st["redo_overflows"] == 0, (prof, st)
    assert first and int(first.group(2)) <= REDO_CAP < st["redo_candidates"] / st["redo_queries"], (first.groups(), st)
    ids, dists, prof, st = _run(base, queries, spec_rank=1, redo_bound=0, cand_capacity=REDO_CAP)
    first = re.search(report, capfd.readouterr().err)
    print(f"cand_capacity {REDO_CAP}: retries {prof['retries']}, {st}, main lists: {first and first.groups()}")
    _same(ids, dists, rids, rd, (prof, st))
    assert first and int(first.group(1)) == REDO_CAP and int(first.group(3)) == 0, first and first.groups()
    assert prof["retries"] >= 1 and st["redo_overflows"] >= 1, (prof, st)


def test_ties_across_the_redo_threshold(gpu, oracle):
    """tests/test_gpu_redo_tail.py's construction at N = 40 040: every row twice -- whatever the redo threshold is,
    another row ties with it exactly -- and for the first 40 queries the row of the 5th pair a third time, so that
    places 9, 10 and 11 are byte-identical rows and the k-th place goes to the lower id"""
    rng = np.random.RandomState(77)
    half_n = 20_000
    half = rng.standard_normal((half_n, D)).astype(np.float32)
    queries = rng.standard_normal((300, D)).astype(np.float32)
    h5 = oracle.brute_force(half, queries[:40], 5, oracle.METRIC_L2_F32, n_threads=16)[0][:, 4].astype(np.int64)
    assert len(set(h5.tolist())) == 40
    base = np.concatenate([half, half[h5], half], 0)
    rids, rd = oracle.brute_force(base, queries, K + 1, oracle.METRIC_L2_F32, n_threads=16)
    r11 = rd.view(np.uint32)
    good = [i for i in range(40)
            if r11[i, 8] == r11[i, 9] == r11[i, 10] and rids[i, 8] == h5[i] and rids[i, 9] == half_n + i
            and rids[i, 10] == half_n + 40 + h5[i]]
    assert len(good) >= 35, good
    rids, rd = np.ascontiguousarray(rids[:, :K]), np.ascontiguousarray(rd[:, :K])
    for rank in (4, 5):
        ids, dists, prof, st = _run(base, queries, spec_rank=rank)
        print(f"tied rows, j = {rank}: {st}")
        _same(ids, dists, rids, rd, (rank, prof, st))
        assert prof["retries"] == 0 and st["spec_rank"] == rank and st["redo_queries"] > 0, (prof, st)


def test_clipped_rows(gpu, oracle, iid):
    """five rows scaled by 1e3 among the iid rows: their integer row term leaves the range the filter keeps, bp sits
    at its lower clamp limit, the rows pass every live query's filter in the redo scan too and are filed with the
    key -inf.  200 queries at j = 1: nearly all fail and fit the 256 slots."""
    base, queries, _, _ = iid[33_000]
    base = base.copy()
    rows = [0, 16_383, 20_011, 32_767, 32_999]   # (the first and the last row, a tile's last row, a column's first)
    base[rows] *= np.float32(1e3)
    q = queries[:200]
    rids, rd = oracle.brute_force(base, q, K, oracle.METRIC_L2_F32, n_threads=16)
    ids, dists, prof, st = _run(base, q, spec_rank=1)
    print(f"clipped rows, j = 1: retries {prof['retries']}, {st}")
    _same(ids, dists, rids, rd, (prof, st))
    assert prof["retries"] == 0 and st["redo_overflows"] == 0, (prof, st)
    assert 100 <= st["redo_queries"] <= 200, st
    assert st["redo_candidates"] >= len(rows) * st["redo_queries"], st   # (every clipped row is in every redo list)


def test_back_to_back_deferred_searches(gpu, iid):
    """three deferred searches (A, B, A) on one stream with one sync, each with failing queries: the redo lists,
    their counters and the redo word are reused from search to search"""
    import torch
    base, queries, rids, rd = iid[40_037]
    m = 300
    dev = torch.device("cuda", 0)
    eng = _engine(base, i8_filter=2, spec_rank=5, async_search=1)
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
    st = {s_: eng.get_stat(s_) for s_ in STATS}
    eng.close()
    print(f"three deferred searches: {st}")
    for lo, _, ids, dd in outs:
        _same(ids.cpu().numpy().astype(np.uint64), dd.cpu().numpy(), rids[lo:lo + m], rd[lo:lo + m], (lo, st))
    assert st["redo_queries"] >= 3 * 65 and st["redo_overflows"] == 0 and st["redo_candidates"] > 0, st
