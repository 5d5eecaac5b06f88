"""Range search of the brute-force engine (THE RANGE RULE, include/expann_hip.h): every row with
score <= the query's radius, counted exactly, the nearest max_results of them in (score, id) order.  Every comparison
is exact: ids equal, distances equal as uint32 bit patterns, counts equal.

The expected answer comes from the unchanged oracle: oracle.brute_force(base, queries, K) is each query's sorted
(score, id) prefix; for radius r the answer is that prefix cut at dists <= r and the count is its length -- valid
while the count stays below K, which every case asserts."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = np.uint64(2 ** 64 - 1)
N, D, M = 65_573, 128, 300
K_REF = 20_000
KMAX = 16_384  # the longest candidate list: more rows in range than this go through the top-k pipeline


@pytest.fixture(scope="module")
def gpu():
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_device_count() >= 1, "these tests need a HIP device"
    return L


def _engine(base, metric="l2", dtype="f32", **opts):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(base.shape[1], metric, dtype=dtype)
    eng.store_many_vectors(base)
    eng.build()
    for name, val in opts.items():
        eng.set_option(name, val)
    eng.set_profiling(True)
    return eng


def below(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def expected(ref, radii, max_results, id_offset=0, full=False):
    """(ids, dists, counts) from the oracle's sorted prefixes ref = (ids[m, K], dists[m, K]); full: K is the whole
    index, so a count of K is proven too"""
    rids, rd = ref
    radii = np.asarray(radii, np.float32)
    with np.errstate(invalid="ignore"):
        mask = (rd <= radii[:, None]) & (rids != PAD)
    counts = mask.sum(1)
    assert full or counts.max() < rd.shape[1], "a count reaches the oracle's K: the prefix does not prove it"
    m = rd.shape[0]
    ids = np.full((m, max_results), PAD, np.uint64)
    dists = np.full((m, max_results), np.inf, np.float32)
    w = min(max_results, rd.shape[1])
    keep = mask[:, :w]  # (the prefix is sorted: the in-range rows are its first counts[i] entries)
    ids[:, :w][keep] = rids[:, :w][keep] + np.uint64(id_offset)
    dists[:, :w][keep] = rd[:, :w][keep]
    return ids, dists, counts.astype(np.uint32)


def same(got, want, what=""):
    ids, dists, counts = got
    wids, wd, wc = want
    assert np.array_equal(counts, wc), f"{what}: counts differ at {np.flatnonzero(counts != wc)[:8]}"
    if wids.shape[1]:
        assert np.array_equal(ids, wids), f"{what}: ids differ in rows {np.flatnonzero((ids != wids).any(1))[:8]}"
        assert np.array_equal(dists.view(np.uint32), wd.view(np.uint32)), f"{what}: distance bits differ"


def mixed_radii(rd, ts=(1, 10, 100, 1000, 3000), empty_every=6):
    """query i: the exact bits of its t-th distance, t cycling; every empty_every-th query: just below its nearest"""
    m = rd.shape[0]
    r = np.array([rd[i, ts[i % len(ts)] - 1] for i in range(m)], np.float32)
    if empty_every:
        r[::empty_every] = below(rd[::empty_every, 0])
    return r


WIDE_TS = (9_000, 16_384, 16_385, 17_000)


def wide_case(ref):
    """24 queries whose t-th distance, t around the longest list, is the radius"""
    rids, rd = ref
    sub = (rids[:24], rd[:24])
    radii = np.array([rd[i, WIDE_TS[i % 4] - 1] for i in range(24)], np.float32)
    return sub, radii


@pytest.fixture(scope="module")
def big():
    rng = np.random.RandomState(4081)
    base = rng.standard_normal((N, D)).astype(np.float32)
    queries = rng.standard_normal((M, D)).astype(np.float32)
    return base, queries


@pytest.fixture(scope="module")
def big_ref(big, oracle):
    """computed once, shared, never changed: every query's K_REF nearest rows"""
    ref = oracle.brute_force(big[0], big[1], K_REF, oracle.METRIC_L2_F32, n_threads=8)
    for a in ref:
        a.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def big_eng(gpu, big):
    eng = _engine(big[0])
    yield eng
    eng.close()


def stats(eng):
    return {s: eng.get_stat("range_" + s) for s in ("list_queries", "topk_queries", "retries")}


# ---- matrix-core form and boundaries ------------------------------------------------------------------
def test_mixed_radii_on_the_matrix_core_form(big, big_ref, big_eng):
    radii = mixed_radii(big_ref[1])
    big_eng.get_profile()
    got = big_eng.range_search(big[1], radii, 4096)
    prof = big_eng.get_profile()
    want = expected(big_ref, radii, 4096)
    assert (want[2][::6] == 0).all() and want[2].max() >= 3000
    same(got, want, "mixed radii")
    assert (got[0][::6] == PAD).all() and np.isinf(got[1][::6]).all()
    assert prof["scan_kernel"].startswith("scan_gemm_f16"), prof
    st = stats(big_eng)
    assert st["list_queries"] == M and st["topk_queries"] == 0, st


def ties_case(big, big_ref):
    """50 rows appended three more times each; row j's original is the t-th neighbour of query j"""
    base, queries = big
    rids, rd = big_ref
    rows, ts = [], []
    for j in range(50):
        t = (1, 10, 100)[j % 3]
        while int(rids[j, t - 1]) in rows:  # (a row another query took: the next neighbour)
            t += 1
        rows.append(int(rids[j, t - 1]))
        ts.append(t)
    dup = np.repeat(base[rows], 3, axis=0)
    base2 = np.ascontiguousarray(np.concatenate([base, dup]))
    radii = np.array([rd[j, ts[j] - 1] for j in range(50)], np.float32)
    return base2, np.ascontiguousarray(queries[:50]), rows, radii


def test_inclusive_boundary_with_ties(gpu, big, big_ref, oracle):
    base2, q, rows, radii = ties_case(big, big_ref)
    ref2 = oracle.brute_force(base2, q, 400, oracle.METRIC_L2_F32, n_threads=8)
    eng = _engine(base2)
    try:
        got = eng.range_search(q, radii, 256)
        same(got, expected(ref2, radii, 256), "ties, radius on the score")
        for j, r in enumerate(rows):  # all four copies, in id order, at the end of the row
            c = int(got[2][j])
            copies = [r, N + 3 * j, N + 3 * j + 1, N + 3 * j + 2]
            assert [int(x) for x in got[0][j, c - 4:c]] == copies, j
            assert len(set(got[1][j, c - 4:c].view(np.uint32).tolist())) == 1
        lo = below(radii)
        got = eng.range_search(q, lo, 256)
        same(got, expected(ref2, lo, 256), "ties, radius just below")
        for j, r in enumerate(rows):
            assert not np.isin(got[0][j], np.array([r, N + 3 * j, N + 3 * j + 1, N + 3 * j + 2], np.uint64)).any(), j
    finally:
        eng.close()


def test_truncation(big, big_ref, big_eng):
    radii = mixed_radii(big_ref[1])
    got = big_eng.range_search(big[1], radii, 16)
    want = expected(big_ref, radii, 16)
    assert (want[2] > 16).sum() > 100
    same(got, want, "truncated to 16")
    assert np.array_equal(got[2], expected(big_ref, radii, 4096)[2])


@pytest.mark.parametrize("max_results", [8192, 100])
def test_wide_radii(big, big_ref, big_eng, max_results):
    sub, radii = wide_case(big_ref)
    got = big_eng.range_search(big[1][:24], radii, max_results)
    want = expected(sub, radii, max_results)
    same(got, want, "wide radii")
    n_top = int((want[2] > KMAX).sum())
    assert 0 < n_top < 24 and (want[2] == KMAX).any()
    st = stats(big_eng)
    assert st["topk_queries"] == n_top and st["list_queries"] == 24 - n_top, st


# ---- count-only and capacity ----------------------------------------------------------------------------
def test_count_only(gpu, big, big_ref, big_eng):
    radii = mixed_radii(big_ref[1])
    ids, dists, counts = big_eng.range_search(big[1], radii, 0)
    assert ids.shape == (M, 0) and np.array_equal(counts, expected(big_ref, radii, 0)[2])
    sub, wide = wide_case(big_ref)
    q = np.ascontiguousarray(big[1][:24])
    counts = np.zeros(24, np.uint32)
    rc = gpu.expann_range_search(big_eng._h, q.ctypes.data, wide.ctypes.data, 24, 0, None, None, counts.ctypes.data)
    assert rc == 0 and np.array_equal(counts, expected(sub, wide, 0)[2])


def test_small_lists_forced(big, big_ref, big_eng):
    radii = mixed_radii(big_ref[1])
    big_eng.set_option("cand_capacity", 256)
    try:
        got = big_eng.range_search(big[1], radii, 4096)
        st = stats(big_eng)
    finally:
        big_eng.set_option("cand_capacity", 0)
    same(got, expected(big_ref, radii, 4096), "cand_capacity 256")
    assert st["retries"] > 0 and st["list_queries"] == M, st


# ---- other paths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(3000, 128), (1000, 48)])
def test_direct_path_small_index(gpu, oracle, n, d):
    rng = np.random.RandomState(n + d)
    base = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((7, d)).astype(np.float32)
    ref = oracle.brute_force(base, queries, n, oracle.METRIC_L2_F32, n_threads=4)
    radii = mixed_radii(ref[1], ts=(1, 10, 100, 500), empty_every=5)
    eng = _engine(base)
    try:
        eng.get_profile()
        got = eng.range_search(queries, radii, 512)
        assert eng.get_profile()["scan_kernel"].startswith("scan_filter_f32")
        same(got, expected(ref, radii, 512, full=True), "direct path")
    finally:
        eng.close()


def test_direct_path_forced_on_the_big_index(big, big_ref, big_eng):
    radii = mixed_radii(big_ref[1])[:40]
    sub = (big_ref[0][:40], big_ref[1][:40])
    big_eng.set_option("scan_kernel", 1)
    try:
        big_eng.get_profile()
        got = big_eng.range_search(big[1][:40], radii, 4096)
        prof = big_eng.get_profile()
    finally:
        big_eng.set_option("scan_kernel", 0)
    assert prof["scan_kernel"].startswith("scan_filter_f32"), prof
    same(got, expected(sub, radii, 4096), "scan_kernel = 1")


def ip_case(big):
    """inner product: 64 queries whose norms span two decades (the case ip_rescale exists for)"""
    rng = np.random.RandomState(77)
    q = big[1][:64] * (10.0 ** rng.uniform(-1.0, 1.0, size=(64, 1))).astype(np.float32)
    return np.ascontiguousarray(q.astype(np.float32))


def test_inner_product(gpu, big, oracle):
    base = big[0]
    q = ip_case(big)
    ref = oracle.brute_force(base, q, 3000, oracle.METRIC_IP_F32, n_threads=8)
    radii = mixed_radii(ref[1], ts=(1, 10, 100, 1000))
    assert (radii < 0).all()  # score = -dot: the near rows have negative scores
    eng = _engine(base, "ip")
    try:
        eng.get_profile()
        got = eng.range_search(q, radii, 2048)
        assert eng.get_profile()["scan_kernel"].startswith("scan_gemm_f16")
        same(got, expected(ref, radii, 2048), "inner product, negative radii")
        # positive radii: "dot >= -r" holds for more than half of the rows -- the count from every row's score
        q3 = np.ascontiguousarray(big[1][:3])
        pos = np.array([0.5, 2.0, 0.25], np.float32)
        want_c = []
        for i in range(3):
            _, sc = oracle.filter_by_score(base, q3[i], np.arange(N), np.inf, oracle.METRIC_IP_F32)
            assert sc.size == N
            want_c.append(int((sc <= pos[i]).sum()))
        assert min(want_c) > KMAX
        ref3 = oracle.brute_force(base, q3, 100, oracle.METRIC_IP_F32, n_threads=4)
        ids, dists, counts = eng.range_search(q3, pos, 100)
        assert counts.tolist() == want_c
        assert np.array_equal(ids, ref3[0]) and np.array_equal(dists.view(np.uint32), ref3[1].view(np.uint32))
        assert stats(eng)["topk_queries"] == 3
    finally:
        eng.close()


def test_binary16_rows(gpu, big, oracle):
    base16 = big[0].astype(np.float16)
    up = np.ascontiguousarray(base16.astype(np.float32))
    q = big[1]
    ref = oracle.brute_force(up, q, 1500, oracle.METRIC_L2_F32, n_threads=8)
    radii = mixed_radii(ref[1], ts=(1, 10, 100, 1000))
    want = expected(ref, radii, 1024)
    e16, e32 = _engine(base16, dtype="f16"), _engine(up)
    try:
        e16.get_profile()
        g16, g32 = e16.range_search(q, radii, 1024), e32.range_search(q, radii, 1024)
        assert e16.get_profile()["scan_kernel"].startswith("scan_gemm_f16")
        same(g16, want, "f16 rows against the oracle over the upcast rows")
        same(g16, g32, "f16 rows against the f32 index of the upcast rows")
        e16.set_option("scan_kernel", 1)
        e16.get_profile()
        g16 = e16.range_search(q[:20], radii[:20], 1024)
        assert e16.get_profile()["scan_kernel"].startswith("scan_filter_f32_any")
        same(g16, tuple(a[:20] for a in want), "f16 rows, direct path")
    finally:
        e16.close()
        e32.close()


@pytest.mark.parametrize("n,d,m,kernel", [(40_000, 144, 64, "scan_gemm_f16kl"), (5_000, 48, 9, "scan_filter_f32_any")])
def test_run_time_dims(gpu, oracle, n, d, m, kernel):
    rng = np.random.RandomState(n + d)
    base = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((m, d)).astype(np.float32)
    ref = oracle.brute_force(base, queries, 1500, oracle.METRIC_L2_F32, n_threads=8)
    radii = mixed_radii(ref[1], ts=(1, 10, 100, 1000))
    eng = _engine(base)
    try:
        eng.get_profile()
        got = eng.range_search(queries, radii, 1024)
        assert eng.get_profile()["scan_kernel"].startswith(kernel)
        same(got, expected(ref, radii, 1024), f"d = {d}")
    finally:
        eng.close()


def test_device_buffers(gpu, big, big_ref):
    import torch
    from expann_amd import GpuBruteForceEngine
    base, queries = big
    radii = mixed_radii(big_ref[1])
    off = 1_000_003
    dev = torch.device("cuda:0")
    t_base = torch.from_numpy(base).to(dev)
    eng = GpuBruteForceEngine(D, "l2")
    try:
        eng.set_base_device(t_base.data_ptr(), N, id_offset=off)
        st = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(st):
            t_q = torch.from_numpy(queries).to(dev, non_blocking=False)
            t_r = torch.from_numpy(radii).to(dev)
            t_ids = torch.zeros((M, 64), dtype=torch.int64, device=dev)
            t_d = torch.zeros((M, 64), dtype=torch.float32, device=dev)
            t_c = torch.zeros(M, dtype=torch.int32, device=dev)
            eng.range_search_device(t_q.data_ptr(), t_r.data_ptr(), M, 64, t_ids.data_ptr(), t_d.data_ptr(), t_c.data_ptr(),
                                    stream=st.cuda_stream)
            got = (t_ids.cpu().numpy().view(np.uint64), t_d.cpu().numpy(), t_c.cpu().numpy().view(np.uint32))
            same(got, expected(big_ref, radii, 64, id_offset=off), "device buffers, id_offset")
            # count only on device buffers: ids and dists NULL
            t_c.zero_()
            eng.range_search_device(t_q.data_ptr(), t_r.data_ptr(), M, 0, 0, 0, t_c.data_ptr(), stream=st.cuda_stream)
            assert np.array_equal(t_c.cpu().numpy().view(np.uint32), got[2])
    finally:
        eng.close()


# ---- edge cases ---------------------------------------------------------------------------------------------
def test_special_radii(gpu, big, big_ref, big_eng, oracle):
    q = np.ascontiguousarray(big[1][:12])
    radii = np.array([np.nan, -np.inf, big_ref[1][2, 9]] * 4, np.float32)
    ids, dists, counts = big_eng.range_search(q, radii, 32)
    same((ids, dists, counts), expected((big_ref[0][:12], big_ref[1][:12]), radii, 32), "NaN and -inf")
    assert (counts[0::3] == 0).all() and (counts[1::3] == 0).all() and (counts[2::3] > 0).any()
    # +inf on the big index: every row, through the top-k pipeline
    ids, dists, counts = big_eng.range_search(q[:5], np.float32(np.inf), 16)
    assert (counts == N).all() and stats(big_eng)["topk_queries"] == 5
    assert np.array_equal(ids, big_ref[0][:5, :16]) and np.array_equal(dists.view(np.uint32), big_ref[1][:5, :16].view(np.uint32))
    # +inf on a 3 000-row index: count n, every row ascending
    rng = np.random.RandomState(3128)
    base = rng.standard_normal((3000, 128)).astype(np.float32)
    qs = rng.standard_normal((7, 128)).astype(np.float32)
    ref = oracle.brute_force(base, qs, 3000, oracle.METRIC_L2_F32, n_threads=4)
    eng = _engine(base)
    try:
        ids, dists, counts = eng.range_search(qs, np.inf, 4096)
        assert (counts == 3000).all()
        assert np.array_equal(ids[:, :3000], ref[0]) and (ids[:, 3000:] == PAD).all()
        assert np.array_equal(dists[:, :3000].view(np.uint32), ref[1].view(np.uint32)) and np.isinf(dists[:, 3000:]).all()
    finally:
        eng.close()


def far_case(big):
    """20 queries; two lie outside the index's fp16 range (one component of 1e30, one of 1e4)"""
    q = np.ascontiguousarray(big[1][:20]).copy()
    q[3, 17] = np.float32(1e30)
    q[11, 5] = np.float32(1e4)
    return q


def test_query_outside_the_fp16_range(gpu, big, big_eng, oracle):
    q = far_case(big)
    ref = oracle.brute_force(big[0], q, 1500, oracle.METRIC_L2_F32, n_threads=8)
    radii = mixed_radii(ref[1], ts=(1, 10, 100, 1000), empty_every=0)
    assert np.isinf(ref[1][3]).all()
    radii[3] = np.float32(3.0e38)  # every score of that query is +inf: nothing is in range of a finite radius
    big_eng.get_profile()
    got = big_eng.range_search(q, radii, 1024)
    prof = big_eng.get_profile()
    want = expected(ref, radii, 1024)
    assert want[2][3] == 0 and want[2][11] >= 10
    same(got, want, "a batch with queries outside the fp16 range")
    assert prof["scan_kernel"].startswith("scan_filter_f32"), prof


def test_far_query_in_a_batch_whose_lists_overflow(gpu, big, big_eng, oracle):
    """the restart on the direct scan after the fp16 attempt's select has listed overflowing queries: lists of 256
    keys, one +inf radius (every row, through the top-k pipeline) beside the two far queries; every query is answered
    once and counted once"""
    q = far_case(big)
    ref = oracle.brute_force(big[0], q, 1500, oracle.METRIC_L2_F32, n_threads=8)
    radii = mixed_radii(ref[1], ts=(1, 10, 100, 1000), empty_every=0)
    radii[3] = np.float32(3.0e38)
    finite = radii.copy()
    radii[7] = np.float32(np.inf)
    want = [a.copy() for a in expected(ref, finite, 64)]
    want[0][7], want[1][7], want[2][7] = ref[0][7, :64], ref[1][7, :64], N
    big_eng.set_option("cand_capacity", 256)
    try:
        big_eng.get_profile()
        got = big_eng.range_search(q, radii, 64)
        prof, st = big_eng.get_profile(), stats(big_eng)
        counts_only = big_eng.range_search(q, radii, 0)[2]
        prof0, st0 = big_eng.get_profile(), stats(big_eng)
    finally:
        big_eng.set_option("cand_capacity", 0)
    same(got, tuple(want), "far queries and overflowing lists in one batch")
    n_over = int((want[2] > 256).sum())
    assert n_over >= 3
    assert st == {"list_queries": 19, "topk_queries": 1, "retries": n_over}, st
    # the profile holds the scan that stands, not the abandoned fp16 attempt: the direct scan of stage 1, and (rows
    # wanted) the scan of the plain pipeline that serves the one query of stage 3
    assert prof["scan_kernel"].startswith("scan_filter_f32") and prof["scan_launches"] == 2, prof
    assert prof0["scan_kernel"].startswith("scan_filter_f32") and prof0["scan_launches"] == 1, prof0
    assert np.array_equal(counts_only, want[2]) and st0 == st, st0  # (count only: the same stages, the same statistics)


def test_more_than_one_pass(gpu, oracle):
    rng = np.random.RandomState(14)
    base = rng.standard_normal((2048, 16)).astype(np.float32)
    queries = rng.standard_normal((33_000, 16)).astype(np.float32)
    ref = oracle.brute_force(base, queries, 64, oracle.METRIC_L2_F32, n_threads=8)
    radii = np.ascontiguousarray(ref[1][:, 4])
    eng = _engine(base)
    try:
        got = eng.range_search(queries, radii, 8)
        same(got, expected(ref, radii, 8), "33 000 queries")
        assert stats(eng)["list_queries"] == 33_000
    finally:
        eng.close()


def test_neighbourly_behaviour(gpu, big, big_ref, big_eng):
    from expann_amd import GpuBruteForceEngine, _lib
    base, queries = big
    radii = mixed_radii(big_ref[1])
    want = expected(big_ref, radii, 64)
    plain = lambda: big_eng.query_k_batch(queries, 10)
    bits = lambda r: (r[0].tobytes(), r[1].tobytes())
    a = plain()
    assert np.array_equal(a[0], big_ref[0][:, :10])
    same(big_eng.range_search(queries, radii, 64), want, "between two plain searches")
    assert bits(plain()) == bits(a)
    r1 = big_eng.range_search(queries, radii, 64)
    assert bits(plain()) == bits(a)
    r2 = big_eng.range_search(queries, radii, 64)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(r1, r2))
    # a row filter in force: UNSUPPORTED, the handle stays usable, and after the filter is cleared the search works
    big_eng.set_row_filter(np.arange(N) % 2 == 0)
    try:
        with pytest.raises(_lib.ExpannError) as e:
            big_eng.range_search(queries, radii, 64)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        assert big_eng.get_stat("filter_active") == 1
    finally:
        big_eng.set_row_filter(None)
    same(big_eng.range_search(queries, radii, 64), want, "after clear_row_filter")
    # groups that are merely set are ignored
    big_eng.set_row_groups((np.arange(N) % 7).astype(np.uint32))
    try:
        same(big_eng.range_search(queries, radii, 64), want, "with row groups set")
    finally:
        big_eng.set_row_groups(None)
    # m = 0 is OK
    one_q, one_r, one_c = np.zeros((1, D), np.float32), np.ones(1, np.float32), np.full(1, 77, np.uint32)
    one_ids = np.zeros((1, 8), np.uint64)
    assert gpu.expann_range_search(big_eng._h, one_q.ctypes.data, one_r.ctypes.data, 0, 8, one_ids.ctypes.data, None,
                                   one_c.ctypes.data) == 0 and one_c[0] == 77
    # before build(): NOT_BUILT
    eng = GpuBruteForceEngine(D, "l2")
    try:
        eng.store_many_vectors(base[:100])
        with pytest.raises(_lib.ExpannError) as e:
            eng.range_search(queries[:4], 1.0, 8)
        assert e.value.code == _lib.ERR_NOT_BUILT
        eng.build()
        assert eng.range_search(queries[:4], np.inf, 8)[2].tolist() == [100] * 4
    finally:
        eng.close()
