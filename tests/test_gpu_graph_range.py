"""Range search of the graph engine (expann_graph_range_search and the calls on top of it) on the GPU.  Ids, distance
bits, counts and per-query distcomps are compared with the restatement of THE RANGE WALK RULE in
tests/graph_range_helpers.py (pinned on the CPU by tests/test_graph_range_abi.py), through the host-buffer and the
device-buffer entry point, over fp32 and binary16 handles, at a compiled dim (128) and a run-time one (48).  No
tolerance anywhere.  A restatement is computed once per (graph, ef, R, rank) and shared by the tests that need it."""
import ctypes as C

import numpy as np
import pytest

import graph_filter_helpers as H
import graph_groups_helpers as G
import graph_range_helpers as Rg

pytestmark = pytest.mark.gpu

M, EF_R, RANKS = Rg.M, Rg.EF_R, Rg.RANKS
DIMS = (128, 48)


class _Case:
    """a graph of 3000 rows, its fp32 handle (and binary16 one, on demand), its queries and memoised restatements"""

    def __init__(self, L, oracle, tmp, name, base, q):
        import torch
        self.L, self.base, self.q = L, base, q
        self.idx = H.build_index_cpu(tmp, base, name=name)
        self.g = H.IndexGraph(self.idx)
        assert self.g.n_layers >= 2
        self.Df = H.dist_f32_matrix(oracle, base, q)
        self.h = H.graph_from_index(L, self.idx, base)
        self._h16 = None
        self._radii, self._want = {}, {}
        self.tq = torch.from_numpy(q).cuda()
        torch.cuda.synchronize()

    @property
    def h16(self):
        if self._h16 is None:  # (sift_like rows are integers up to 255: exact in binary16)
            self._h16 = G.graph_f16_from_index(self.L, self.idx, self.base)
        return self._h16

    def radii(self, rank):
        if rank not in self._radii:
            self._radii[rank] = Rg.radii_at_rank(self.Df, rank)
        return self._radii[rank]

    def want(self, ef, R, rank):
        """the restatement over all queries: (ids, dists, counts, distcomps, peak candidates, peak nearest)"""
        key = (ef, R, rank)
        if key not in self._want:
            self._want[key] = Rg.range_walk(self.g, self.Df, self.radii(rank), R, ef)
        return self._want[key]

    def close(self):
        self.L.expann_graph_destroy(self.h)
        if self._h16 is not None:
            self.L.expann_graph_destroy(self._h16)


class _World:
    def __init__(self, tmp, oracle):
        from expann_amd import _lib
        self.tmp, self.oracle, self.L = tmp, oracle, _lib.load()
        self._cases = {}

    def dim(self, d):
        if d not in self._cases:
            rng = np.random.RandomState(2000 + d)
            base = H.sift_like(rng, Rg.N_ROWS, d)
            q = H.sift_like(rng, M, d, frac=True)
            self._cases[d] = _Case(self.L, self.oracle, self.tmp, "range", base, q)
        return self._cases[d]

    def dup(self):
        """375 distinct rows, each 8 times: equal distances on both sides of every radius and at the cap boundary;
        the queries are rows themselves for a third of the batch, so distance 0 ties too"""
        if "dup" not in self._cases:
            rng = np.random.RandomState(77)
            distinct = H.sift_like(rng, Rg.N_ROWS // 8, 128)
            base = np.ascontiguousarray(np.tile(distinct, (8, 1))[rng.permutation(Rg.N_ROWS)])
            q = H.sift_like(rng, M, 128, frac=True)
            q[::3] = base[rng.randint(0, Rg.N_ROWS, size=len(q[::3]))]
            self._cases["dup"] = _Case(self.L, self.oracle, self.tmp, "range_dup", base, q)
        return self._cases["dup"]

    def close(self):
        for c in self._cases.values():
            c.close()


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    w = _World(tmp_path_factory.mktemp("graph_range"), oracle)
    yield w
    w.close()


@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream()


def _stat(L, h, name):
    out = C.c_uint64()
    assert L.expann_graph_get_stat(h, name.encode(), C.byref(out)) == 0
    return out.value


def _host(L, h, q, radii, R, ef, dists=True, distcomps=True, ids=True):
    """expann_graph_range_search on host buffers pre-filled with a pattern no search writes:
    (rc, ids, dists, counts, distcomps)"""
    q = np.ascontiguousarray(q, np.float32)
    radii = np.ascontiguousarray(radii, np.float32)
    m = q.shape[0]
    o_ids = np.full((m, R), 5, np.uint64)
    o_d = np.full((m, R), -1.0, np.float32)
    o_cnt = np.full(m, 0xDEADBEEF, np.uint32)
    o_dc = np.full(m, 0xDEADBEEF, np.uint32)
    rc = L.expann_graph_range_search(h, q.ctypes.data, radii.ctypes.data, m, R, ef, o_ids.ctypes.data if ids else None,
                                     o_d.ctypes.data if dists else None, o_cnt.ctypes.data,
                                     o_dc.ctypes.data if distcomps else None)
    return rc, o_ids, o_d, o_cnt, o_dc


def _check(got, want, what):
    rc, ids, dists, counts, dc = got
    assert rc == 0, what
    bad = np.flatnonzero((ids != want[0]).any(1) | (dists.view(np.uint32) != want[1].view(np.uint32)).any(1) |
                         (counts != want[2]) | (dc != want[3]))
    assert bad.size == 0, (what, bad[:8], counts[bad[:8]], want[2][bad[:8]], dc[bad[:8]], want[3][bad[:8]])


def _plain(L, h, q, k, ef):
    from graph_ranged_helpers import search_mode
    rc, ids, dists, dc = search_mode(L, h, q, k, ef, 0)
    assert rc == 0, L.expann_graph_last_error(h)
    return ids, dists, dc


# ---- 1. bit equality with the restatement ---------------------------------------------------------
@pytest.mark.parametrize("ef,R", EF_R)
@pytest.mark.parametrize("d", DIMS)
def test_fp32_handle_is_the_restatement(world, d, ef, R):
    c = world.dim(d)
    for rank in RANKS:
        _check(_host(c.L, c.h, c.q, c.radii(rank), R, ef), c.want(ef, R, rank), (d, ef, R, rank))
        # the radius equals a distance exactly: the rank-th row itself is in range
        assert ((c.Df == c.radii(rank)[:, None]).sum(1) >= 1).all()
    assert c.L.expann_graph_last_kernel_ms(c.h) > 0
    if R > ef:  # `nearest` did grow past ef
        assert max(c.want(ef, R, rank)[5].max() for rank in RANKS) > ef + 1


@pytest.mark.parametrize("ef,R", EF_R)
@pytest.mark.parametrize("d", DIMS)
def test_f16_handle_is_the_fp32_handle(world, d, ef, R):
    """THE F16 ROW RULE: the binary16 handle of rows that are exact in binary16 returns the same bits"""
    c = world.dim(d)
    for rank in RANKS:
        _check(_host(c.L, c.h16, c.q, c.radii(rank), R, ef), c.want(ef, R, rank), (d, ef, R, rank))


def test_more_queries_than_resident_workgroups(world):
    """R = 4096 with a candidates heap of 8192 is 131 KB of LDS, one workgroup per CU: 300 queries are pulled by fewer
    workgroups than there are queries"""
    c = world.dim(128)
    L = c.L
    ef, R, rank = 60, 4096, 800
    assert L.expann_graph_set_option(c.h, b"cand_capacity", 8192) == 0
    try:
        got = _host(L, c.h, c.q, c.radii(rank), R, ef)
    finally:
        assert L.expann_graph_set_option(c.h, b"cand_capacity", 0) == 0
    _check(got, c.want(ef, R, rank), "R = 4096")


# ---- 2. ties --------------------------------------------------------------------------------------
@pytest.mark.parametrize("ef,R", EF_R)
def test_duplicated_rows(world, ef, R):
    c = world.dup()
    for rank in RANKS:
        radii = c.radii(rank)
        # equal distances on both sides of the radius: the rank-th distance occurs several times (8 copies of a row)
        assert ((c.Df == radii[:, None]).sum(1) >= 2).mean() > 0.9
        _check(_host(c.L, c.h, c.q, radii, R, ef), c.want(ef, R, rank), ("dup", ef, R, rank))
    assert (c.Df[::3].min(1) == 0).all()


# ---- 3. degenerate radii ----------------------------------------------------------------------------
@pytest.mark.parametrize("ef,R", EF_R)
@pytest.mark.parametrize("d", DIMS)
def test_a_radius_in_range_of_nothing_is_the_plain_walk(world, d, ef, R):
    c = world.dim(d)
    _, _, plain_dc = _plain(c.L, c.h, c.q, 1, ef)
    for r in (-1.0, float("nan")):
        rc, ids, dists, counts, dc = _host(c.L, c.h, c.q, np.full(M, r, np.float32), R, ef)
        assert rc == 0
        assert np.array_equal(dc, plain_dc) and not counts.any(), r
        assert (ids == H.PAD).all() and np.isinf(dists).all() and (dists > 0).all(), r


@pytest.mark.parametrize("ef,R", [(10, 8), (60, 16), (60, 60)])
@pytest.mark.parametrize("d", DIMS)
def test_an_infinite_radius_with_R_up_to_ef_is_the_plain_search(world, d, ef, R):
    c = world.dim(d)
    pi, pd, pdc = _plain(c.L, c.h, c.q, R, ef)
    rc, ids, dists, counts, dc = _host(c.L, c.h, c.q, np.full(M, np.inf, np.float32), R, ef)
    assert rc == 0
    assert np.array_equal(ids, pi) and np.array_equal(dists.view(np.uint32), pd.view(np.uint32))
    assert np.array_equal(dc, pdc) and (counts >= R).all() and (counts < dc).all()


# ---- 4. counting only, optional outputs -----------------------------------------------------------
@pytest.mark.parametrize("ef,R", [(10, 8), (60, 16)])
def test_counting_only_and_null_outputs(world, ef, R):
    """max_results = 0 has cap = ef, as R <= ef has: the counts (and distcomps) of case 1"""
    c = world.dim(128)
    for rank in RANKS:
        want = c.want(ef, R, rank)
        rc, _, _, counts, dc = _host(c.L, c.h, c.q, c.radii(rank), 0, ef, dists=False, ids=False)
        assert rc == 0, c.L.expann_graph_last_error(c.h)
        assert np.array_equal(counts, want[2]) and np.array_equal(dc, want[3]), rank
    rc, ids, dists, counts, dc = _host(c.L, c.h, c.q, c.radii(50), R, ef, dists=False, distcomps=False)
    want = c.want(ef, R, 50)
    assert rc == 0 and np.array_equal(ids, want[0]) and np.array_equal(counts, want[2])
    assert (dists == -1.0).all() and (dc == 0xDEADBEEF).all()  # nothing was written where NULL was passed


# ---- 5. soundness against the exact answer ----------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_soundness_against_the_exact_answer(world, d):
    """every returned id is truly in range (Df holds the oracle's brute-force distance of every pair), counts never
    exceed the true number, the returned count is min(counts, R), ascending order.  No recall threshold."""
    c = world.dim(d)
    seen = set()
    for ef, R in EF_R:
        for rank in RANKS:
            radii = c.radii(rank)
            rc, ids, dists, counts, _ = _host(c.L, c.h, c.q, radii, R, ef)
            assert rc == 0
            seen |= {"below ef"} if (counts < ef).any() else set()
            seen |= {"between ef and cap"} if R > ef and ((counts > ef) & (counts < R)).any() else set()
            seen |= {"beyond cap"} if (counts > max(ef, R)).any() else set()
            true = (c.Df <= radii[:, None]).sum(1)
            assert (counts <= true).all(), (ef, R, rank)
            kept = ids != H.PAD
            assert np.array_equal(kept.sum(1), np.minimum(counts, R)), (ef, R, rank)
            assert (kept[:, :-1] >= kept[:, 1:]).all()  # the padding is a tail
            exact = np.take_along_axis(c.Df, np.where(kept, ids, 0).astype(np.int64), axis=1)
            assert np.array_equal(dists[kept].view(np.uint32), exact[kept].view(np.uint32))
            assert (exact[kept] <= np.broadcast_to(radii[:, None], kept.shape)[kept]).all()
            assert (dists[:, :-1] <= dists[:, 1:])[kept[:, 1:]].all()  # ascending over the rows returned
            for i in range(0, M, 37):  # no row twice
                assert np.unique(ids[i][kept[i]]).size == kept[i].sum()
    assert seen == {"below ef", "between ef and cap", "beyond cap"}, seen


# ---- 6. redo and overflow -----------------------------------------------------------------------------
def _device(c, h, radii_t, R, ef, st, dists=True, distcomps=True):
    import torch
    ids = torch.full((M, max(R, 1)), -2, dtype=torch.int64, device="cuda")
    d = torch.full((M, max(R, 1)), -1.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((M,), -3, dtype=torch.int32, device="cuda")
    dc = torch.full((M,), -3, dtype=torch.int32, device="cuda")
    st.wait_stream(torch.cuda.current_stream())
    rc = c.L.expann_graph_range_search_device(h, c.tq.data_ptr(), radii_t.data_ptr(), M, R, ef, ids.data_ptr() if R else None,
                                              d.data_ptr() if dists else None, cnt.data_ptr(),
                                              dc.data_ptr() if distcomps else None, st.cuda_stream)
    return rc, ids, d, cnt, dc


def _np(out, R):
    rc, ids, d, cnt, dc = out
    return (rc, ids.cpu().numpy().view(np.uint64)[:, :R], d.cpu().numpy()[:, :R], cnt.cpu().numpy().view(np.uint32),
            dc.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("ef,R", [(20, 256), (60, 1024)])
def test_redo_serves_overflowed_walks(world, stream, ef, R):
    """a candidates heap of 8 overflows in the first launch; the redo launch walks those queries again and the rows,
    counts and distcomps are the default capacity's, through both entry points"""
    import torch
    c = world.dim(128)
    L, rank = c.L, 200
    want = c.want(ef, R, rank)
    assert want[4].max() > 8
    tr = torch.from_numpy(c.radii(rank)).cuda()
    assert L.expann_graph_sync(c.h) == 0
    assert L.expann_graph_set_option(c.h, b"cand_capacity", 8) == 0
    try:
        before = _stat(L, c.h, "distcomps")
        out = _device(c, c.h, tr, R, ef, stream)
        assert out[0] == 0 and L.expann_graph_sync(c.h) == 0, L.expann_graph_last_error(c.h)
        _check(_np(out, R), want, "device buffers, heap of 8")
        assert 0 < _stat(L, c.h, "redo_queries") <= M
        assert _stat(L, c.h, "distcomps") - before == int(want[3].sum())  # a redone walk is counted once
        _check(_host(L, c.h, c.q, c.radii(rank), R, ef), want, "host buffers, heap of 8")
    finally:
        assert L.expann_graph_set_option(c.h, b"cand_capacity", 0) == 0
    out = _device(c, c.h, tr, R, ef, stream)
    assert out[0] == 0 and L.expann_graph_sync(c.h) == 0
    _check(_np(out, R), want, "device buffers, automatic capacity")
    assert _stat(L, c.h, "redo_queries") == 0


def test_overflow_is_reported_and_leaves_the_handle_usable(world, stream):
    import torch
    from expann_amd import _lib
    c = world.dim(128)
    L, (ef, R), rank = c.L, (20, 256), 200
    tr = torch.from_numpy(c.radii(rank)).cuda()
    assert L.expann_graph_sync(c.h) == 0
    overflows = _stat(L, c.h, "redo_overflows")
    assert L.expann_graph_set_option(c.h, b"cand_capacity", 8) == 0
    assert L.expann_graph_set_option(c.h, b"redo_capacity", 8) == 0
    try:
        assert _host(L, c.h, c.q, c.radii(rank), R, ef)[0] == _lib.ERR_OVERFLOW
        assert b"overflow" in L.expann_graph_last_error(c.h)
        out = _device(c, c.h, tr, R, ef, stream)
        assert out[0] == 0
        assert L.expann_graph_sync(c.h) == _lib.ERR_OVERFLOW
        assert _stat(L, c.h, "redo_overflows") == overflows + 1
        assert L.expann_graph_sync(c.h) == 0  # reported once
    finally:
        assert L.expann_graph_set_option(c.h, b"cand_capacity", 0) == 0
        assert L.expann_graph_set_option(c.h, b"redo_capacity", 0) == 0
    _check(_host(L, c.h, c.q, c.radii(rank), R, ef), c.want(ef, R, rank), "after the overflow")
    pi, pd, pdc = _plain(L, c.h, c.q, 10, 40)  # visited sets were left clean for the plain walk too
    oi, od, odc = world.oracle.Graph(c.idx).query_k(c.q, 10, 40, False)
    assert np.array_equal(pi, oi) and np.array_equal(pd.view(np.uint32), od.view(np.uint32)) and np.array_equal(pdc, odc)


# ---- 7. device buffers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_device_buffer_call_equals_the_host_buffer_call(world, stream, d):
    import torch
    c = world.dim(d)
    L = c.L
    assert L.expann_graph_sync(c.h) == 0
    deferred, ranged = _stat(L, c.h, "deferred_searches"), _stat(L, c.h, "range_searches")
    for h in (c.h, c.h16):
        for (ef, R), rank in zip(EF_R, (10, 50, 200, 800)):
            tr = torch.from_numpy(c.radii(rank)).cuda()
            out = _device(c, h, tr, R, ef, stream)
            assert out[0] == 0, L.expann_graph_last_error(h)
            assert L.expann_graph_sync(h) == 0
            assert L.expann_graph_last_kernel_ms(h) > 0
            _check(_np(out, R), c.want(ef, R, rank), (d, ef, R, rank))
    assert _stat(L, c.h, "deferred_searches") == deferred + 4 and _stat(L, c.h, "range_searches") == ranged + 4
    # counting only with NULL ids, NULL dists and NULL distcomps
    tr = torch.from_numpy(c.radii(50)).cuda()
    out = _device(c, c.h, tr, 0, 60, stream, dists=False, distcomps=False)
    assert out[0] == 0 and L.expann_graph_sync(c.h) == 0
    assert np.array_equal(out[3].cpu().numpy().view(np.uint32), c.want(60, 16, 50)[2])
    assert (out[1] == -2).all() and (out[2] == -1).all() and (out[4] == -3).all()


def test_searches_enqueued_back_to_back_keep_their_results_apart(world, stream):
    """two range searches and a plain search on one stream, one sync"""
    import torch
    c = world.dim(128)
    L = c.L
    assert L.expann_graph_sync(c.h) == 0
    tr_a, tr_b = torch.from_numpy(c.radii(200)).cuda(), torch.from_numpy(c.radii(10)).cuda()
    a = _device(c, c.h, tr_a, 256, 20, stream)
    pids = torch.full((M, 10), -2, dtype=torch.int64, device="cuda")
    pd = torch.full((M, 10), -1.0, dtype=torch.float32, device="cuda")
    pdc = torch.full((M,), -3, dtype=torch.int32, device="cuda")
    rc_p = L.expann_graph_search_device(c.h, c.tq.data_ptr(), M, 10, 40, 0, pids.data_ptr(), pd.data_ptr(), pdc.data_ptr(),
                                        stream.cuda_stream)
    b = _device(c, c.h, tr_b, 16, 60, stream)
    assert a[0] == 0 and rc_p == 0 and b[0] == 0
    assert L.expann_graph_sync(c.h) == 0
    _check(_np(a, 256), c.want(20, 256, 200), "first range search")
    _check(_np(b, 16), c.want(60, 16, 10), "second range search")
    oi, od, odc = world.oracle.Graph(c.idx).query_k(c.q, 10, 40, False)
    assert np.array_equal(pids.cpu().numpy().view(np.uint64), oi)
    assert np.array_equal(pd.cpu().numpy().view(np.uint32), od.view(np.uint32))
    assert np.array_equal(pdc.cpu().numpy().view(np.uint32), odc.astype(np.uint32))


# ---- 8. errors, filters, groups ---------------------------------------------------------------------------
def test_errors_in_the_documented_order(world, stream):
    from expann_amd import _lib
    c = world.dim(128)
    L, h = c.L, c.h
    INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
    q, r = c.q[:4].copy(), c.radii(10)[:4].copy()
    ids, d = np.zeros((4, 8), np.uint64), np.zeros((4, 8), np.float32)
    cnt, dc = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    Q, Rr, I, D, Cn, Dc = (x.ctypes.data for x in (q, r, ids, d, cnt, dc))

    def both(queries, radii, m, R, ef, o_ids, o_cnt):
        rc_h = L.expann_graph_range_search(h, queries, radii, m, R, ef, o_ids, D, o_cnt, Dc)
        rc_d = L.expann_graph_range_search_device(h, queries, radii, m, R, ef, o_ids, D, o_cnt, Dc, stream.cuda_stream)
        assert rc_h == rc_d, (rc_h, rc_d)
        return rc_h
    assert L.expann_graph_sync(h) == 0
    deferred, ranged = _stat(L, h, "deferred_searches"), _stat(L, h, "range_searches")
    assert both(Q, Rr, 0, 8, 0, I, Cn) == INV         # ef_search == 0 comes before m == 0
    assert both(None, None, 0, 8, 10, None, None) == _lib.OK  # m == 0 comes before the pointers
    assert both(None, Rr, 4, 8, 10, I, Cn) == INV
    assert both(Q, None, 4, 8, 10, I, Cn) == INV
    assert both(Q, Rr, 4, 8, 10, I, None) == INV
    assert both(Q, Rr, 4, 8, 10, None, Cn) == INV
    assert both(Q, Rr, 4, 8, 4097, None, Cn) == INV   # a NULL pointer comes before the limits
    assert both(Q, Rr, 4, 8, 4097, I, Cn) == UNS
    assert both(Q, Rr, 4, 4097, 10, I, Cn) == UNS
    assert b"4096" in L.expann_graph_last_error(h)
    allow = np.ones(Rg.N_ROWS, bool)
    from expann_amd import pack_row_filter
    words = pack_row_filter(allow)
    assert L.expann_graph_set_row_filter(h, words.ctypes.data, words.size) == 0
    try:
        assert both(Q, Rr, 4, 8, 10, I, Cn) == UNS
        assert b"filter" in L.expann_graph_last_error(h)
        assert both(Q, Rr, 4, 4097, 10, None, Cn) == INV  # ... and the filter comes last
    finally:
        assert L.expann_graph_clear_row_filter(h) == 0
    assert _stat(L, h, "deferred_searches") == deferred and _stat(L, h, "range_searches") == ranged
    assert L.expann_graph_sync(h) == 0
    _check(_host(L, h, c.q, c.radii(50), 16, 60), c.want(60, 16, 50), "after the filter was cleared")
    assert _stat(L, h, "range_searches") == ranged + 1


def test_groups_are_ignored_and_other_searches_are_untouched(world):
    """row groups that are merely set change nothing; the plain, the filtered and the grouped search return after the
    range calls what they returned before them"""
    from expann_amd import pack_row_filter
    c = world.dim(128)
    L, h = c.L, c.h
    labels = (np.arange(Rg.N_ROWS) % 3).astype(np.uint32)
    qg = (np.arange(M) % 3).astype(np.uint32)
    words = pack_row_filter(np.arange(Rg.N_ROWS) % 2 == 0)

    def others():
        out = [_plain(L, h, c.q, 10, 40)]
        assert L.expann_graph_set_row_filter(h, words.ctypes.data, words.size) == 0
        out.append(_plain(L, h, c.q, 10, 40))
        assert L.expann_graph_clear_row_filter(h) == 0
        ids, d, dc = np.zeros((M, 10), np.uint64), np.zeros((M, 10), np.float32), np.zeros(M, np.uint32)
        assert L.expann_graph_search_grouped(h, c.q.ctypes.data, qg.ctypes.data, M, 10, 40, 0, ids.ctypes.data,
                                             d.ctypes.data, dc.ctypes.data) == 0
        out.append((ids, d, dc))
        return out
    assert L.expann_graph_set_row_groups(h, labels.ctypes.data, labels.size) == 0
    try:
        before = others()
        for (ef, R), rank in zip(EF_R, (800, 200, 50, 800)):
            _check(_host(L, h, c.q, c.radii(rank), R, ef), c.want(ef, R, rank), ("groups set", ef, R, rank))
        after = others()
    finally:
        assert L.expann_graph_clear_row_groups(h) == 0
    for b, a in zip(before, after):
        assert np.array_equal(b[0], a[0]) and np.array_equal(b[1].view(np.uint32), a[1].view(np.uint32))
        assert np.array_equal(b[2], a[2])
    oi, od, odc = world.oracle.Graph(c.idx).query_k(c.q, 10, 40, False)
    assert np.array_equal(after[0][0], oi) and np.array_equal(after[0][2], odc)


# ---- 9. the engine ------------------------------------------------------------------------------------------
def test_engine_range_search_is_the_c_call_on_its_graph(world, stream):
    import torch
    from expann_amd import AntitopoEngine, _lib
    c = world.dim(128)
    eng = AntitopoEngine(16, 80, 1, 0, False, dim=128)
    try:
        with pytest.raises(_lib.ExpannError) as ei:  # rows or not, before build() there is no graph
            eng.range_search(c.q, 1.0, 4)
        assert ei.value.code == _lib.ERR_NOT_BUILT
        with pytest.raises(_lib.ExpannError) as ei:
            eng.range_search_device(c.tq.data_ptr(), c.tq.data_ptr(), M, 4, c.tq.data_ptr(), 0, c.tq.data_ptr())
        assert ei.value.code == _lib.ERR_NOT_BUILT
        eng.load_index(c.idx)  # the graph of c.h: the same index file
        # ef_search unset: set as query_k sets it, from max(1, max_results)
        ids, dists, counts = eng.range_search(c.q, c.radii(10), 16)
        rc, wi, wd, wc, _ = _host(c.L, c.h, c.q, c.radii(10), 16, 16)
        assert rc == 0 and np.array_equal(ids, wi) and np.array_equal(dists.view(np.uint32), wd.view(np.uint32))
        assert np.array_equal(counts, wc)
        # ... and sticky: the next search runs at 16 too, whatever its max_results
        ids, dists, counts = eng.range_search(c.q, c.radii(200), 256)
        rc, wi, wd, wc, _ = _host(c.L, c.h, c.q, c.radii(200), 256, 16)
        assert rc == 0 and np.array_equal(ids, wi) and np.array_equal(counts, wc)
        eng.set_ef_search(60)
        for R, rank in ((16, 50), (1024, 800)):
            want = c.want(60, R, rank)
            ids, dists, counts = eng.range_search(c.q, c.radii(rank), R)
            assert np.array_equal(ids, want[0]) and np.array_equal(dists.view(np.uint32), want[1].view(np.uint32))
            assert np.array_equal(counts, want[2])
        # a scalar radius, and counting only
        r0 = float(np.median(c.radii(50)))
        ids, dists, counts = eng.range_search(c.q, r0, 0)
        assert ids.shape == (M, 0) and np.array_equal(counts, _host(c.L, c.h, c.q, np.full(M, r0, np.float32), 0, 60)[3])
        # device buffers
        want = c.want(60, 1024, 800)
        tr = torch.from_numpy(c.radii(800)).cuda()
        t_ids = torch.full((M, 1024), -2, dtype=torch.int64, device="cuda")
        t_d = torch.full((M, 1024), -1.0, dtype=torch.float32, device="cuda")
        t_c = torch.full((M,), -3, dtype=torch.int32, device="cuda")
        stream.wait_stream(torch.cuda.current_stream())
        eng.range_search_device(c.tq.data_ptr(), tr.data_ptr(), M, 1024, t_ids.data_ptr(), t_d.data_ptr(), t_c.data_ptr(),
                                stream=stream.cuda_stream)
        eng.sync()
        assert np.array_equal(t_ids.cpu().numpy().view(np.uint64), want[0])
        assert np.array_equal(t_d.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
        assert np.array_equal(t_c.cpu().numpy().view(np.uint32), want[2])
    finally:
        eng.close()
