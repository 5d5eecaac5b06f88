"""Row groups of the brute-force engine: every query of a batch names the group whose rows it may
return.  The expected answer is the CPU oracle over base[groups == X] with its ids mapped back; ids are compared for
equality and distances as uint32 bit patterns, whichever of the four ways served the query."""
import numpy as np
import pytest

from row_groups_helpers import ANY, PAD, expected, expected_grouped, label_rows, list_kernel_tq, same, tier_stats

pytestmark = pytest.mark.gpu

N = 3000
TQ = list_kernel_tq()
# group sizes around the 16-row step (one below, at, one above), around the boundary case's L = 64, and two that span
# more than one row chunk of the list kernel (a chunk is at least 8 steps = 128 rows)
SIZES = [1, 15, 16, 17, 33, 64, 65, 300, 450]
LABELS = [7, 0, 1_000_003, 0xFFFFFFFE, 12, 640, 650, 3, 0x80000000]
REST = [100, 101, 102, 103, 104, 105, 106, 107]   # the other rows: groups of about 250
ABSENT = 555                                      # a label no row carries
# queries per label: 1, TQ and TQ + 1 of them (a lone query, a full tile, a tile and one more)
COUNTS = [TQ + 1, TQ, 1, TQ + 1, TQ, TQ + 1, TQ, TQ + 1, 2 * TQ + 1]


@pytest.fixture(scope="module")
def gpu():
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_device_count() >= 1, "these tests need a HIP device"
    return L


def _engine(base, metric="l2", dtype="f32"):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(base.shape[1], metric, dtype)
    eng.store_many_vectors(base)
    eng.build()
    return eng


def _batch(seed, with_any=False):
    """query labels in random order: COUNTS[i] queries for LABELS[i], one per rest label, two for the absent one"""
    qg = []
    for lab, c in zip(LABELS, COUNTS):
        qg += [lab] * c
    qg += REST + [ABSENT, ABSENT]
    if with_any:
        qg += [ANY] * (TQ + 3)
    qg = np.asarray(qg, np.uint32)
    return qg[np.random.RandomState(seed).permutation(qg.size)]


_cache = {}


def _setup(d, dtype, metric):
    """rows, labels, queries, query labels and one engine per configuration, made once and left unchanged"""
    key = (d, dtype, metric)
    if key not in _cache:
        rng = np.random.RandomState(1000 + d + (7 if dtype == "f16" else 0) + (13 if metric == "ip" else 0))
        base = rng.standard_normal((N, d)).astype(np.float32)
        if dtype == "f16":
            base = base.astype(np.float16).astype(np.float32)   # (the f16 engine answers as the f32 one over these)
        groups = label_rows(N, SIZES, LABELS, REST, seed=d)
        qg = _batch(seed=d + 1)
        queries = rng.standard_normal((qg.size, d)).astype(np.float32)
        eng = _engine(base, metric, dtype)
        eng.set_row_groups(groups)
        _cache[key] = (base, groups, queries, qg, eng)
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for v in _cache.values():
        v[4].close()
    _cache.clear()


# 1. the list kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("d", [128, 48])
@pytest.mark.parametrize("k", [10, 40])
def test_list_kernel(gpu, oracle, d, dtype, metric, k):
    base, groups, queries, qg, eng = _setup(d, dtype, metric)
    assert eng.get_stat("groups_active") == 1
    assert eng.get_stat("group_count") == len(SIZES) + len(REST)
    got = eng.query_k_batch(queries, k, groups=qg)
    want = expected_grouped(oracle, base, groups, queries, qg, k, ip=metric == "ip")
    same(got, want, (d, dtype, metric, k))
    st = tier_stats(eng)
    assert sum(st.values()) == qg.size, st
    assert st == {"list": qg.size - 2, "filter": 0, "any": 0, "pad": 2}, st
    assert eng.get_stat("group_filter_passes") == 0
    # the label no row carries came back as padding, and the groups smaller than k are padded behind their rows
    pad_rows = np.flatnonzero(qg == ABSENT)
    assert (got[0][pad_rows] == PAD).all() and np.isinf(got[1][pad_rows]).all()
    for lab, s in zip(LABELS, SIZES):
        rows = got[0][qg == lab]
        assert ((rows != PAD).sum(axis=1) == min(k, s)).all(), (lab, s)
        assert np.isin(rows[rows != PAD], np.flatnonzero(groups == lab)).all(), lab


@pytest.mark.parametrize("d,dtype", [(2064, "f32"), (4096, "f32"), (4096, "f16")])
def test_list_kernel_wide_rows(gpu, oracle, d, dtype):
    """a query tile of 8 x d floats beyond 64 KiB of LDS (d > 2048): the launch raises the kernel's limit first"""
    n = 400
    rng = np.random.RandomState(d)
    base = rng.standard_normal((n, d)).astype(np.float32)
    if dtype == "f16":
        base = base.astype(np.float16).astype(np.float32)
    groups = label_rows(n, [17, 150], [4, 5], [6], seed=d)
    qg = np.asarray([4] * (TQ + 1) + [5] * 3 + [6, ABSENT], np.uint32)
    queries = rng.standard_normal((qg.size, d)).astype(np.float32)
    eng = _engine(base, "l2", dtype)
    eng.set_row_groups(groups)
    same(eng.query_k_batch(queries, 10, groups=qg), expected_grouped(oracle, base, groups, queries, qg, 10))
    assert tier_stats(eng) == {"list": qg.size - 1, "filter": 0, "any": 0, "pad": 1}
    eng.close()


# 2. ties --------------------------------------------------------------------------------------
def test_ties_resolve_to_the_lower_id_within_the_group(gpu, oracle):
    rng = np.random.RandomState(5)
    block = rng.standard_normal((64, 128)).astype(np.float32)
    base = np.concatenate([block, block, block, rng.standard_normal((200, 128)).astype(np.float32)])
    groups = np.full(base.shape[0], 9, np.uint32)
    groups[:64] = 1
    groups[64:128] = 2      # the same rows under the other label
    groups[128:192] = 1
    queries = np.concatenate([block[:5] + 0.01, rng.standard_normal((4, 128)).astype(np.float32)]).astype(np.float32)
    qg = np.asarray([1, 2, 1, 2, 1, 1, 2, 1, 1], np.uint32)
    eng = _engine(base)
    eng.set_row_groups(groups)
    ids, dists = eng.query_k_batch(queries, 20, groups=qg)
    same((ids, dists), expected_grouped(oracle, base, groups, queries, qg, 20))
    for i in np.flatnonzero(qg == 1):
        assert (ids[i] < 192).all() and not ((ids[i] >= 64) & (ids[i] < 128)).any()
        # every row of the block is there twice: equal distances in pairs, the lower id first
        assert np.array_equal(ids[i][0::2] + np.uint64(128), ids[i][1::2])
        assert np.array_equal(dists[i][0::2].view(np.uint32), dists[i][1::2].view(np.uint32))
    for i in np.flatnonzero(qg == 2):
        assert ((ids[i] >= 64) & (ids[i] < 128)).all()
    eng.close()


# 3. the same answer as the bitmap --------------------------------------------------------------
def test_same_answer_as_the_row_filter_on_the_same_handle(gpu, oracle):
    from expann_amd import _lib
    base, groups, queries, qg, eng = _setup(128, "f32", "l2")
    grouped = eng.query_k_batch(queries, 10, groups=qg)
    for lab in (LABELS[3], LABELS[7], REST[2]):
        sel = np.flatnonzero(qg == lab)
        eng.set_row_filter(groups == lab)
        try:
            with pytest.raises(_lib.ExpannError) as ei:
                eng.query_k_batch(queries, 10, groups=qg)
            assert ei.value.code == _lib.ERR_UNSUPPORTED
            filtered = eng.query_k_batch(np.ascontiguousarray(queries[sel]), 10)
        finally:
            eng.set_row_filter(None)
        same((grouped[0][sel], grouped[1][sel]), filtered, lab)
    assert eng.get_stat("filter_active") == 0
    same(eng.query_k_batch(queries, 10, groups=qg), grouped)


# 4. ANY ---------------------------------------------------------------------------------------
def test_any_queries_get_the_plain_search(gpu, oracle):
    base, groups, queries, qg, eng = _setup(128, "f32", "l2")
    groups_x = groups.copy()
    loose = np.flatnonzero(groups == REST[0])[:40]
    groups_x[loose] = ANY                      # rows that belong to no group
    near = (base[loose[:6]] + 0.001).astype(np.float32)   # queries right beside such rows
    eng.set_row_groups(groups_x)
    try:
        # all ANY: the plain search, bit for bit
        q_all = np.concatenate([queries[:20], near])
        got = eng.query_k_batch(q_all, 10, groups=np.full(q_all.shape[0], ANY, np.uint32))
        same(got, eng.query_k_batch(q_all, 10))
        same(got, oracle.brute_force(base, q_all, 10, oracle.METRIC_L2_F32, n_threads=8))
        assert tier_stats(eng) == {"list": 0, "filter": 0, "any": q_all.shape[0], "pad": 0}
        assert np.isin(loose[:6], got[0][20:]).all()
        # mixed: the ANY rows equal the plain search of those queries; a labelled query never sees a loose row
        qg_m = _batch(seed=77, with_any=True)
        q_m = np.concatenate([near, queries, queries[:16] * np.float32(0.5)])[:qg_m.size]
        assert q_m.shape[0] == qg_m.size
        qg_m[:6] = [ANY, REST[0], ANY, REST[0], ANY, REST[0]]
        got = eng.query_k_batch(q_m, 10, groups=qg_m)
        same(got, expected_grouped(oracle, base, groups_x, q_m, qg_m, 10))
        a = np.flatnonzero(qg_m == ANY)
        same((got[0][a], got[1][a]), eng.query_k_batch(np.ascontiguousarray(q_m[a]), 10))
        st = tier_stats(eng)
        assert st["any"] == a.size and sum(st.values()) == qg_m.size, st
        assert not np.isin(got[0][qg_m != ANY], loose).any()
        assert np.isin(loose[[0, 2, 4]], got[0][[0, 2, 4]]).all()
    finally:
        eng.set_row_groups(groups)


# 5. filter groups through the matrix cores -------------------------------------------------------
def test_large_groups_take_filter_passes(gpu, oracle):
    n, d, m = 65_573, 128, 300
    rng = np.random.RandomState(4081)
    base = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((m, d)).astype(np.float32)
    u = rng.rand(n)
    groups = np.where(u < 0.45, 1, np.where(u < 0.90, 2, 10 + rng.randint(0, 65, n))).astype(np.uint32)
    qg = np.concatenate([np.full(110, 1), np.full(110, 2), 10 + rng.randint(0, 65, 78), [ABSENT, ANY]]).astype(np.uint32)
    qg = qg[rng.permutation(m)]
    eng = _engine(base)
    eng.set_row_groups(groups)
    got = eng.query_k_batch(queries, 10, groups=qg)
    assert eng.get_stat("group_filter_passes") == 2
    assert eng.get_stat("filter_active") == 0
    assert tier_stats(eng) == {"list": 78, "filter": 220, "any": 1, "pad": 1}
    same(got, expected_grouped(oracle, base, groups, queries, qg, 10))
    # the plain search is what it was
    same(eng.query_k_batch(queries[:40], 10), oracle.brute_force(base, queries[:40], 10, oracle.METRIC_L2_F32, n_threads=8))
    eng.close()


# 6. the boundary L ------------------------------------------------------------------------------
def test_group_list_rows_boundary(gpu, oracle):
    from expann_amd import _lib
    base, groups, queries, qg, eng = _setup(128, "f32", "l2")
    sel = np.flatnonzero((qg == 640) | (qg == 650))     # the groups of 64 and of 65 rows
    q, g = np.ascontiguousarray(queries[sel]), np.ascontiguousarray(qg[sel])
    want = expected_grouped(oracle, base, groups, q, g, 10)
    try:
        eng.set_option("group_list_rows", 64)
        same(eng.query_k_batch(q, 10, groups=g), want, "L = 64")
        assert tier_stats(eng) == {"list": int((g == 640).sum()), "filter": int((g == 650).sum()), "any": 0, "pad": 0}
        assert eng.get_stat("group_filter_passes") == 1 and eng.get_stat("filter_active") == 0
        eng.set_option("group_list_rows", 16384)
        same(eng.query_k_batch(q, 10, groups=g), want, "L = 16384")
        assert tier_stats(eng)["list"] == g.size and eng.get_stat("group_filter_passes") == 0
        with pytest.raises(_lib.ExpannError) as ei:
            eng.set_option("group_list_rows", 16385)
        assert ei.value.code == _lib.ERR_INVALID_ARG
    finally:
        eng.set_option("group_list_rows", 0)
    same(eng.query_k_batch(q, 10, groups=g), want, "auto")


# 7. device entry, id_offset, a second labelling -----------------------------------------------------
def test_device_entry_id_offset_and_relabelling(gpu, oracle):
    import torch
    from expann_amd import GpuBruteForceEngine
    base, groups, queries, qg, eng0 = _setup(128, "f32", "l2")
    off = 10 ** 9
    dev = torch.device("cuda", 0)
    tb = torch.from_numpy(base).to(dev)
    tq = torch.from_numpy(queries).to(dev)
    m, k = queries.shape[0], 10
    t_ids = torch.empty(m, k, dtype=torch.int64, device=dev)
    t_d = torch.empty(m, k, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    eng = GpuBruteForceEngine(128, "l2")
    eng.set_base_device(tb.data_ptr(), N, 0)
    eng.set_row_groups(groups)
    eng.set_base_device(tb.data_ptr(), N, off)           # a new base clears the groups
    assert eng.get_stat("groups_active") == 0 and eng.get_stat("group_count") == 0
    tg = torch.from_numpy(groups.view(np.int32)).to(dev)
    eng.set_row_groups_device(tg.data_ptr(), N)
    assert eng.get_stat("groups_active") == 1
    eng.search_device(tq.data_ptr(), m, k, t_ids.data_ptr(), t_d.data_ptr(), groups=qg)   # (returns drained)
    dev_got = (t_ids.cpu().numpy().view(np.uint64), t_d.cpu().numpy())
    host_got = eng.query_k_batch(queries, k, groups=qg)
    same(dev_got, host_got)
    same(host_got, expected_grouped(oracle, base, groups, queries, qg, k, id_offset=off))
    # a second labelling: the same group sizes on other rows
    groups2 = groups[np.random.RandomState(3).permutation(N)]
    eng.set_row_groups(groups2)
    got2 = eng.query_k_batch(queries, k, groups=qg)
    same(got2, expected_grouped(oracle, base, groups2, queries, qg, k, id_offset=off))
    assert not np.array_equal(got2[0], host_got[0])
    eng.close()


# 8. larger k ------------------------------------------------------------------------------------
def test_k_600(gpu, oracle):
    rng = np.random.RandomState(8)
    base = rng.standard_normal((N, 128)).astype(np.float32)
    groups = label_rows(N, [1000, 300], [21, 22], REST, seed=8)
    qg = np.asarray([21] * (TQ + 1) + [22] * 3 + [21, 22], np.uint32)
    queries = rng.standard_normal((qg.size, 128)).astype(np.float32)
    eng = _engine(base)
    eng.set_row_groups(groups)
    got = eng.query_k_batch(queries, 600, groups=qg)
    same(got, expected_grouped(oracle, base, groups, queries, qg, 600))
    assert tier_stats(eng)["list"] == qg.size
    assert ((got[0][qg == 22] != PAD).sum(axis=1) == 300).all()
    assert ((got[0][qg == 21] != PAD).sum(axis=1) == 600).all()
    eng.close()


def test_errors_of_the_set_and_search_calls(gpu):
    from expann_amd import GpuBruteForceEngine, _lib
    base, groups, queries, qg, eng = _setup(128, "f32", "l2")
    with pytest.raises(_lib.ExpannError) as ei:
        eng.set_row_groups(groups[:-1])                  # n != size
    assert ei.value.code == _lib.ERR_INVALID_ARG
    assert eng.get_stat("groups_active") == 1            # a failed call leaves the groups as they were
    fresh = GpuBruteForceEngine(128, "l2")
    fresh.store_many_vectors(base[:100])
    with pytest.raises(_lib.ExpannError) as ei:
        fresh.set_row_groups(groups[:100])               # no rows on the device yet
    assert ei.value.code == _lib.ERR_NOT_BUILT
    fresh.build()
    with pytest.raises(_lib.ExpannError) as ei:
        fresh.query_k_batch(queries[:3], 5, groups=qg[:3])   # no groups set
    assert ei.value.code == _lib.ERR_NOT_BUILT
    fresh.close()
    u8 = GpuBruteForceEngine(128, "l2", "u8")
    u8.store_many_vectors(np.zeros((64, 128), np.uint8))
    u8.build()
    with pytest.raises(_lib.ExpannError) as ei:
        u8.set_row_groups(np.zeros(64, np.uint32))
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    u8.close()
