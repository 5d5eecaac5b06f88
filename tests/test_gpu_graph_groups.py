"""Row groups of the graph engine (expann_graph_set_row_groups, expann_graph_search_grouped and the calls on top of
them) on the GPU.  Ids, distance bits and per-query distcomps of a batch in which every query names its own group
are compared with the restatement in tests/graph_groups_helpers.py (pinned on the CPU by
tests/test_graph_groups_abi.py and tests/test_graph_filter_abi.py), through the host-buffer and the device-buffer
entry point; then with the handle's own bitmap path, group by group.  No tolerance anywhere, and no search may end
in EXPANN_ERR_OVERFLOW: a candidates heap holds a vertex at most once, 3000 < the redo capacity 8192."""
import ctypes as C

import numpy as np
import pytest

import graph_filter_helpers as H
import graph_groups_helpers as G

pytestmark = pytest.mark.gpu

K, EFS, M = G.K, G.EFS, G.M
STATS = ("group_walk_queries", "group_scan_queries", "group_pad_queries")


class _Case:
    """a graph handle, its restatement, labels and query groups"""

    def __init__(self, L, oracle, idx, h, base, q):
        import torch
        self.L, self.oracle, self.idx, self.h, self.base, self.q = L, oracle, idx, h, base, q
        self.n = base.shape[0]
        self.g = H.IndexGraph(idx)
        assert self.g.n_layers >= 2
        self.og = oracle.Graph(idx)
        self.Df = H.dist_f32_matrix(oracle, base, q)
        self._Db = {0: self.Df}
        self.R = G.Restatement(self.g, self.Df, self.Db)
        self.labels, self.qg = G.make_labels(self.n), G.query_groups(M)
        G.check_classes(self.labels, self.qg, H.descent_ends(self.g, self.Df))
        self.tq = torch.from_numpy(q).cuda()
        self.tqg = torch.from_numpy(self.qg.view(np.int32)).cuda()
        self.h16 = None
        torch.cuda.synchronize()

    def Db(self, mode):
        if mode not in self._Db:
            self._Db[mode] = H.bottom_matrix(self.oracle, self.base, self.q, mode, self.Df)
        return self._Db[mode]


class _World:
    def __init__(self, tmp, oracle):
        from expann_amd import _lib
        self.tmp, self.oracle, self.L = tmp, oracle, _lib.load()
        self._cases = {}

    def dim(self, d):
        """n = 3000, M = 16, ef_construction = 80: the serial build through the C ABI at exactly the rows' dim"""
        if d not in self._cases:
            L = self.L
            rng = np.random.RandomState(1000 + d)
            base = H.sift_like(rng, G.N_ROWS, d)
            q = H.sift_like(rng, M, d, frac=True)
            idx = str(self.tmp / f"g_{d}.index")
            e = C.c_void_p()
            assert L.expann_antitopo_create(d, 0, 16, 80, 1, 0, 0, C.byref(e)) == 0
            assert L.expann_antitopo_store(e, base.ctypes.data, base.shape[0]) == 0
            assert L.expann_antitopo_save(e, idx.encode()) == 0
            L.expann_antitopo_destroy(e)
            self._cases[d] = _Case(L, self.oracle, idx, H.graph_from_index(L, idx, base), base, q)
        return self._cases[d]

    def f16(self, d):
        c = self.dim(d)
        if c.h16 is None:
            c.h16 = G.graph_f16_from_index(self.L, c.idx, c.base)
        return c

    def close(self):
        for c in self._cases.values():
            self.L.expann_graph_destroy(c.h)
            if c.h16 is not None:
                self.L.expann_graph_destroy(c.h16)


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    w = _World(tmp_path_factory.mktemp("graph_groups"), oracle)
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


def _stats(L, h):
    return [_stat(L, h, s) for s in STATS]


def _set(c, labels, flat_rows, h=None):
    L, h = c.L, h or c.h
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    assert L.expann_graph_set_option(h, b"filter_flat_rows", flat_rows) == 0
    assert L.expann_graph_set_row_groups(h, labels.ctypes.data, labels.size) == 0, L.expann_graph_last_error(h)


def _reset(c, h=None):
    L, h = c.L, h or c.h
    assert L.expann_graph_clear_row_groups(h) == 0
    assert L.expann_graph_clear_row_filter(h) == 0
    for opt in (b"filter_flat_rows", b"cand_capacity", b"redo_capacity"):
        assert L.expann_graph_set_option(h, opt, 0) == 0


def _out(m, k):
    """output tensors pre-filled with a pattern no search writes"""
    import torch
    return (torch.full((m, k), -2, dtype=torch.int64, device="cuda"),
            torch.full((m, k), -1.0, dtype=torch.float32, device="cuda"),
            torch.full((m,), -3, dtype=torch.int32, device="cuda"))


def _np(ids, dists, dc):
    return ids.cpu().numpy().view(np.uint64), dists.cpu().numpy(), dc.cpu().numpy().view(np.uint32)


def _enqueue_grouped(c, tqg, k, ef, mode, st, h=None):
    import torch
    ids, dists, dc = _out(M, k)
    st.wait_stream(torch.cuda.current_stream())
    rc = c.L.expann_graph_search_grouped_device(h or c.h, c.tq.data_ptr(), tqg.data_ptr(), M, k, ef, mode, ids.data_ptr(),
                                                dists.data_ptr(), dc.data_ptr(), st.cuda_stream)
    return rc, ids, dists, dc


def _enqueue_plain(c, k, ef, mode, st, h=None):
    import torch
    ids, dists, dc = _out(M, k)
    st.wait_stream(torch.cuda.current_stream())
    rc = c.L.expann_graph_search_device(h or c.h, c.tq.data_ptr(), M, k, ef, mode, ids.data_ptr(), dists.data_ptr(),
                                        dc.data_ptr(), st.cuda_stream)
    return rc, ids, dists, dc


def _sync(c, h=None):
    """no walk of these tests can overflow for good (module docstring)"""
    assert c.L.expann_graph_sync(h or c.h) == 0, c.L.expann_graph_last_error(h or c.h)


def _grouped_device(c, tqg, k, ef, mode, st, h=None):
    rc, ids, dists, dc = _enqueue_grouped(c, tqg, k, ef, mode, st, h)
    assert rc == 0, c.L.expann_graph_last_error(h or c.h)
    _sync(c, h)
    return _np(ids, dists, dc)


def _grouped_host(c, qg, k, ef, mode, h=None):
    qg = np.ascontiguousarray(qg, dtype=np.uint32)
    ids, dists, dc = np.zeros((M, k), np.uint64), np.zeros((M, k), np.float32), np.zeros(M, np.uint32)
    rc = c.L.expann_graph_search_grouped(h or c.h, c.q.ctypes.data, qg.ctypes.data, M, k, ef, mode, ids.ctypes.data,
                                         dists.ctypes.data, dc.ctypes.data)
    assert rc == 0, c.L.expann_graph_last_error(h or c.h)
    return ids, dists, dc


def _plain_device(c, k, ef, mode, st, h=None):
    rc, ids, dists, dc = _enqueue_plain(c, k, ef, mode, st, h)
    assert rc == 0, c.L.expann_graph_last_error(h or c.h)
    _sync(c, h)
    return _np(ids, dists, dc)


def _assert_equal(got, exp, what):
    """ids, distance bits and per-query distcomps, exactly"""
    assert np.array_equal(got[0], exp[0]), what
    assert np.array_equal(got[1].view(np.uint32), exp[1].view(np.uint32)), what
    assert np.array_equal(np.asarray(got[2]).astype(np.uint64), np.asarray(exp[2]).astype(np.uint64)), what


def _cand_cap(ef):
    cap = 256
    while cap < 16 * ef and cap < 8192:
        cap *= 2
    return cap


@pytest.mark.parametrize("d,mode", [(128, 0), (128, 1), (128, 2), (192, 0), (192, 1), (192, 2), (48, 0)])
def test_mixed_batch_equals_the_restatement(world, stream, d, mode):
    """one batch mixes every kind of query; "filter_flat_rows" = 1: everything but the 1-row group walks (the 7-row
    group visits the whole graph and is redone); 400: both regimes in one batch; 0: everything but ANY is scanned"""
    c = world.dim(d)
    L, h = c.L, c.h
    try:
        for flat in (1, 400, 0):
            _set(c, c.labels, flat)
            assert _stat(L, h, "groups_active") == 1 and _stat(L, h, "group_count") == 6
            for ef in EFS:
                exp = c.R.expected(c.labels, c.qg, K, ef, mode, flat)
                counts = [exp[3].count(x) for x in (G.WALK, G.SCAN, G.PAD)]
                assert all(counts), counts
                before = _stats(L, h)
                _assert_equal(_grouped_device(c, c.tqg, K, ef, mode, stream), exp, (flat, ef, "device buffers"))
                assert _stats(L, h) == [b + n for b, n in zip(before, counts)], (flat, ef)  # both kernels ran
                n_redo = sum(1 for p in exp[4].values() if p > _cand_cap(ef))
                assert _stat(L, h, "redo_queries") == n_redo, (flat, ef)
                if flat == 1 and ef == 10:
                    assert n_redo > 0
                _assert_equal(_grouped_host(c, c.qg, K, ef, mode), exp, (flat, ef, "host buffers"))
                assert _stats(L, h) == [b + 2 * n for b, n in zip(before, counts)], (flat, ef)
    finally:
        _reset(c)
    assert _stat(L, h, "groups_active") == 0 and _stat(L, h, "group_count") == 0


def test_one_group_equals_the_bitmap_path(world, stream):
    """all 48 queries name X: what set_row_filter(labels == X) plus the plain search give at the same option"""
    import torch
    from expann_amd import pack_row_filter
    c = world.dim(128)
    L, h = c.L, c.h
    try:
        for X in (5, 1, G.TOP):
            words = pack_row_filter(c.labels == np.uint32(X))
            tqg = torch.from_numpy(np.full(M, X, np.uint32).view(np.int32)).cuda()
            for flat in (1, 400):
                assert L.expann_graph_clear_row_groups(h) == 0
                assert L.expann_graph_set_option(h, b"filter_flat_rows", flat) == 0
                assert L.expann_graph_set_row_filter(h, words.ctypes.data, words.size) == 0
                bitmap = {ef: _plain_device(c, K, ef, 0, stream) for ef in EFS}
                assert L.expann_graph_clear_row_filter(h) == 0
                _set(c, c.labels, flat)
                for ef in EFS:
                    _assert_equal(_grouped_device(c, tqg, K, ef, 0, stream), bitmap[ef], (X, flat, ef))
                    _assert_equal(_grouped_host(c, np.full(M, X, np.uint32), K, ef, 0), bitmap[ef], (X, flat, ef, "host"))
        # an all-ANY batch is the plain unfiltered search, in all three modes
        tany = torch.from_numpy(np.full(M, G.ANY, np.uint32).view(np.int32)).cuda()
        for mode in (0, 1, 2):
            plain = _plain_device(c, K, 40, mode, stream)
            walked = _stat(L, h, "group_walk_queries")
            _assert_equal(_grouped_device(c, tany, K, 40, mode, stream), plain, ("ANY", mode))
            assert _stat(L, h, "group_walk_queries") == walked + M
    finally:
        _reset(c)


@pytest.mark.parametrize("d", [128, 192])
def test_binary16_rows(world, stream, d):
    """integer rows in [0, 255] are exact in binary16: the handle made by expann_graph_create_f16 answers as the fp32
    handle and as the restatement, in all three modes (compiled and run-time-dim instances over binary16 rows)"""
    c = world.f16(d)
    try:
        _set(c, c.labels, 400, c.h16)
        _set(c, c.labels, 400)
        for mode in (0, 1, 2):
            for ef in EFS:
                exp = c.R.expected(c.labels, c.qg, K, ef, mode, 400)
                got16 = _grouped_device(c, c.tqg, K, ef, mode, stream, c.h16)
                _assert_equal(got16, exp, (mode, ef, "restatement"))
                _assert_equal(got16, _grouped_device(c, c.tqg, K, ef, mode, stream), (mode, ef, "fp32 handle"))
        _assert_equal(_grouped_host(c, c.qg, K, 40, 0, c.h16), c.R.expected(c.labels, c.qg, K, 40, 0, 400), "host buffers")
    finally:
        _reset(c, c.h16)
        _reset(c)


def test_forced_redo(world, stream):
    """a first heap of 64 entries: some walked queries overflow it, the redo launch serves exactly those"""
    c = world.dim(128)
    L, h = c.L, c.h
    try:
        _set(c, c.labels, 400)
        assert L.expann_graph_set_option(h, b"cand_capacity", 64) == 0
        for ef in EFS:
            exp = c.R.expected(c.labels, c.qg, K, ef, 0, 400)
            n_over = sum(1 for p in exp[4].values() if p > 64)
            assert n_over > 0
            _assert_equal(_grouped_device(c, c.tqg, K, ef, 0, stream), exp, (ef, "device buffers"))
            assert _stat(L, h, "redo_queries") == n_over
            _assert_equal(_grouped_host(c, c.qg, K, ef, 0), exp, (ef, "host buffers"))
    finally:
        _reset(c)


def test_stream_order_and_state(world, stream):
    import torch
    from expann_amd import _lib, pack_row_filter
    c = world.dim(128)
    L, h = c.L, c.h
    unf = c.og.query_k(c.q, K, 40, False)
    other = G.other_labels(c.n)
    exp_a = c.R.expected(c.labels, c.qg, K, 40, 0, 400)
    exp_b = c.R.expected(other, c.qg, K, 40, 0, 400, labels_key="other")
    assert not np.array_equal(exp_a[0], exp_b[0])
    try:
        # plain searches before, between and after grouped ones; every search under the labels it was enqueued under
        p0 = _enqueue_plain(c, K, 40, 0, stream)
        _set(c, c.labels, 400)
        ga = _enqueue_grouped(c, c.tqg, K, 40, 0, stream)
        p1 = _enqueue_plain(c, K, 40, 0, stream)
        _set(c, other, 400)
        gb = _enqueue_grouped(c, c.tqg, K, 40, 0, stream)
        p2 = _enqueue_plain(c, K, 40, 0, stream)
        assert all(r[0] == 0 for r in (p0, ga, p1, gb, p2)), L.expann_graph_last_error(h)
        _sync(c)
        for r in (p0, p1, p2):
            _assert_equal(_np(*r[1:]), unf, "plain search")
        _assert_equal(_np(*ga[1:]), exp_a, "first labels")
        _assert_equal(_np(*gb[1:]), exp_b, "second labels")
        # wrong n, NULL labels: refused, the old groups still answer
        assert L.expann_graph_set_row_groups(h, c.labels.ctypes.data, c.n - 1) == _lib.ERR_INVALID_ARG
        assert b"labels" in L.expann_graph_last_error(h)
        assert L.expann_graph_set_row_groups(h, c.labels.ctypes.data, c.n + 1) == _lib.ERR_INVALID_ARG
        assert L.expann_graph_set_row_groups(h, None, c.n) == _lib.ERR_INVALID_ARG
        assert L.expann_graph_set_row_groups_device(h, None, c.n, None) == _lib.ERR_INVALID_ARG
        assert _stat(L, h, "groups_active") == 1 and _stat(L, h, "group_count") == 3
        _assert_equal(_grouped_host(c, c.qg, K, 40, 0), exp_b, "after the refused calls")
        # labels from a tensor written on a side stream, read in its order; the library keeps its own copy
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            t = torch.zeros(c.n, dtype=torch.int32, device="cuda")
            t.copy_(torch.from_numpy(c.labels.view(np.int32)).cuda(), non_blocking=True)
            rc = L.expann_graph_set_row_groups_device(h, t.data_ptr(), c.n, side.cuda_stream)
        assert rc == 0, L.expann_graph_last_error(h)
        t.zero_()
        torch.cuda.synchronize()
        assert _stat(L, h, "group_count") == 6
        _assert_equal(_grouped_device(c, c.tqg, K, 40, 0, stream), exp_a, "device labels")
        # the argument checks, in order: search_mode's, then query_groups, then groups, then the filter
        args = (c.tq.data_ptr(), c.tqg.data_ptr(), M, K, 40, 0)
        o = _out(M, K)
        outs = (o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), None)
        assert L.expann_graph_search_grouped_device(h, c.tq.data_ptr(), None, M, K, 40, 3, *outs) == _lib.ERR_INVALID_ARG
        assert L.expann_graph_search_grouped_device(h, c.tq.data_ptr(), None, 0, K, 40, 0, *outs) == 0  # m == 0
        assert L.expann_graph_search_grouped_device(h, c.tq.data_ptr(), None, M, K, 40, 0, *outs) == _lib.ERR_INVALID_ARG
        assert b"query_groups" in L.expann_graph_last_error(h)
        words = pack_row_filter(np.arange(c.n) % 2 == 0)
        assert L.expann_graph_set_row_filter(h, words.ctypes.data, words.size) == 0
        assert L.expann_graph_search_grouped_device(h, *args, *outs) == _lib.ERR_UNSUPPORTED
        assert L.expann_graph_search_grouped(h, c.q.ctypes.data, c.qg.ctypes.data, M, K, 40, 0, *outs[:3]) == _lib.ERR_UNSUPPORTED
        assert L.expann_graph_clear_row_filter(h) == 0
        _assert_equal(_grouped_device(c, c.tqg, K, 40, 0, stream), exp_a, "after clear_row_filter")
        assert L.expann_graph_clear_row_groups(h) == 0
        assert L.expann_graph_set_row_filter(h, words.ctypes.data, words.size) == 0
        assert L.expann_graph_search_grouped_device(h, *args, *outs) == _lib.ERR_NOT_BUILT  # (groups before the filter)
        assert L.expann_graph_clear_row_filter(h) == 0
        assert L.expann_graph_search_grouped_device(h, *args, *outs) == _lib.ERR_NOT_BUILT
        assert L.expann_graph_search_grouped(h, c.q.ctypes.data, c.qg.ctypes.data, M, K, 40, 0, *outs[:3]) == _lib.ERR_NOT_BUILT
        _sync(c)
        assert (o[0] == -2).all()  # no refused call wrote anything
        _assert_equal(_plain_device(c, K, 40, 0, stream), unf, "plain search after the clear")
    finally:
        _reset(c)


def test_engine_surface(world, stream, tmp_path):
    """AntitopoEngine.set_row_groups / query_many(groups=) / query_many_device(groups_ptr=); load_index clears the
    groups; the C entry points of the engine (gpu_antitopo_engine::query_k_batch_grouped), where a store clears them"""
    import torch
    from expann_amd import AntitopoEngine, _lib
    c = world.dim(128)
    L = c.L
    unf = c.og.query_k(c.q, K, 40, False)
    exp = c.R.expected(c.labels, c.qg, K, 40, 0, 0)  # the engine's automatic "filter_flat_rows": all but ANY scanned
    eng = AntitopoEngine(16, 80, 1, 0, False, dim=128)
    with pytest.raises(_lib.ExpannError) as ei:
        eng.set_row_groups(c.labels)
    assert ei.value.code == _lib.ERR_NOT_BUILT
    eng.load_index(c.idx)
    eng.set_ef_search(40)
    with pytest.raises(_lib.ExpannError) as ei:
        eng.query_many(c.q, K, groups=c.qg)  # no groups yet
    assert ei.value.code == _lib.ERR_NOT_BUILT
    eng.set_row_groups(c.labels)
    ids, dists = eng.query_many(c.q, K, groups=c.qg)
    assert np.array_equal(ids, exp[0]) and np.array_equal(dists.view(np.uint32), exp[1].view(np.uint32))
    ids, dists = eng.query_many(c.q, K)  # without groups= the labels are ignored
    assert np.array_equal(ids, unf[0]) and np.array_equal(dists.view(np.uint32), unf[1].view(np.uint32))
    # device labels, device buffers
    t = torch.from_numpy(c.labels.view(np.int32)).cuda()
    eng.set_row_groups_device(t.data_ptr(), c.n)
    dids, dd, _ = _out(M, K)
    stream.wait_stream(torch.cuda.current_stream())
    eng.query_many_device(c.tq.data_ptr(), M, K, dids.data_ptr(), dd.data_ptr(), stream.cuda_stream, groups_ptr=c.tqg.data_ptr())
    eng.sync()
    assert np.array_equal(dids.cpu().numpy().view(np.uint64), exp[0])
    assert np.array_equal(dd.cpu().numpy().view(np.uint32), exp[1].view(np.uint32))
    with pytest.raises(_lib.ExpannError) as ei:
        eng.set_row_groups(c.labels[:100])
    assert ei.value.code == _lib.ERR_INVALID_ARG
    eng.set_row_groups(None)
    with pytest.raises(_lib.ExpannError) as ei:
        eng.query_many(c.q, K, groups=c.qg)
    assert ei.value.code == _lib.ERR_NOT_BUILT
    eng.set_row_groups(c.labels)
    eng.load_index(c.idx)  # a run-time property: a load starts without groups
    with pytest.raises(_lib.ExpannError) as ei:
        eng.query_many(c.q, K, groups=c.qg)
    assert ei.value.code == _lib.ERR_NOT_BUILT
    eng.close()
    # the C entry points of the engine: before build, grouped query, a store clears the groups
    e = C.c_void_p()
    assert L.expann_antitopo_create(128, 0, 16, 80, 1, 0, 0, C.byref(e)) == 0
    try:
        qg = c.qg
        ids, dists = np.zeros((M, K), np.uint64), np.zeros((M, K), np.float32)
        assert L.expann_antitopo_set_row_groups(e, c.labels.ctypes.data, c.n) == _lib.ERR_NOT_BUILT
        assert L.expann_antitopo_query_grouped(e, c.q.ctypes.data, qg.ctypes.data, M, K, ids.ctypes.data,
                                               dists.ctypes.data) == _lib.ERR_NOT_BUILT
        assert L.expann_antitopo_load(e, c.idx.encode()) == 0
        assert L.expann_antitopo_set_ef_search(e, 40) == 0
        assert L.expann_antitopo_set_row_groups(e, c.labels.ctypes.data, c.n) == 0, L.expann_antitopo_last_error(e)
        assert L.expann_antitopo_query_grouped(e, c.q.ctypes.data, qg.ctypes.data, M, K, ids.ctypes.data,
                                               dists.ctypes.data) == 0, L.expann_antitopo_last_error(e)
        assert np.array_equal(ids, exp[0]) and np.array_equal(dists.view(np.uint32), exp[1].view(np.uint32))
        assert L.expann_antitopo_num_distcomps(e) == int(exp[2].sum())
        assert L.expann_antitopo_set_row_groups(e, None, 0) == 0
        assert L.expann_antitopo_query_grouped(e, c.q.ctypes.data, qg.ctypes.data, M, K, ids.ctypes.data,
                                               dists.ctypes.data) == _lib.ERR_NOT_BUILT
        assert L.expann_antitopo_set_row_groups(e, c.labels.ctypes.data, c.n) == 0
        assert L.expann_antitopo_store(e, c.base.ctypes.data, 1) == 0  # (the uploaded graph stays until the next build)
        assert L.expann_antitopo_query_grouped(e, c.q.ctypes.data, qg.ctypes.data, M, K, ids.ctypes.data,
                                               dists.ctypes.data) == _lib.ERR_NOT_BUILT
    finally:
        L.expann_antitopo_destroy(e)
