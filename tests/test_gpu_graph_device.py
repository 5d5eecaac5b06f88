"""Graph search on device buffers (expann_graph_search_device / expann_graph_sync and the engine calls on top):
queries and results are torch tensors, the search is enqueued on a torch stream, and ids, distance bits and
per-query distcomps must equal the oracle's walk of the same index file -- whichever launch served a query (the
first one, or the redo launch that walks the overflowed queries again at the larger heap), and whichever entry
point asked: the host-buffer call (expann_graph_search_mode) rides the same launches.  The yardsticks are
oracle.Graph(index).query_k for modes 0 and 1 and graph_ranged_helpers.ranged_expected for mode 2, never the
device path itself."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, EFS, M_PARITY, M_ALL = 10, (10, 40), 200, 300
PAD = np.uint64(2 ** 64 - 1)


def _sift_like(rng, n, d, frac=False):
    x = np.clip(np.round(np.abs(rng.standard_normal((n, d))) * 40.0), 0, 255).astype(np.float32)
    if frac:  # fractional parts: the uint8 path truncates the query
        x = np.minimum(255.5, x + rng.uniform(0, 0.99, size=x.shape)).astype(np.float32)
    return x


def _graph_from_index(L, idx, vectors):
    """expann_graph handle over an index file: every layer's lists as CSR, layer l at row l of the offsets"""
    from graph_helpers import read_index_edges
    hdr, layers = read_index_edges(idx)
    n, n_layers = hdr["n"], hdr["max_layer"]
    off = np.zeros((n_layers, n + 1), np.uint64)
    nbs, base = [], 0
    for layer in range(n_layers):
        deg = np.array([len(per[layer][0]) if layer < len(per) else 0 for per in layers], np.uint64)
        off[layer, 0] = base
        off[layer, 1:] = base + np.cumsum(deg)
        nbs += [per[layer][0] for per in layers if layer < len(per)]
        base += int(deg.sum())
    nb = np.concatenate(nbs).astype(np.uint32)
    vectors = np.ascontiguousarray(vectors, dtype=np.float32)
    h = C.c_void_p()
    rc = L.expann_graph_create(vectors.shape[1], 0, vectors.ctypes.data, n, n_layers, hdr["starting_vertex"],
                               off.ctypes.data, nb.ctypes.data, C.byref(h))
    assert rc == 0, L.expann_graph_last_error(None)
    return h, n_layers


class _World:
    """one serial build per dim through the antitopo engine (n = 3000, M = 16, ef_construction = 80), its index
    file, the oracle's graph of that file, the queries as a resident tensor, and the oracle's answers, each
    computed once"""

    def __init__(self, tmp, oracle):
        from expann_amd import _lib
        self.tmp, self.oracle, self.L = tmp, oracle, _lib.load()
        self._dims, self._expected = {}, {}

    def dim(self, d):
        import torch
        if d not in self._dims:
            rng = np.random.RandomState(1000 + d)
            base = _sift_like(rng, 3000, d)
            q = _sift_like(rng, M_ALL, d, frac=True)
            idx = str(self.tmp / f"dev_{d}.index")
            # (the engine of the C ABI at exactly d: the Python class pads 48 and 192 to a compiled dim)
            e = C.c_void_p()
            assert self.L.expann_antitopo_create(d, 0, 16, 80, 1, 0, 0, C.byref(e)) == 0
            assert self.L.expann_antitopo_store(e, base.ctypes.data, base.shape[0]) == 0
            assert self.L.expann_antitopo_save(e, idx.encode()) == 0
            self.L.expann_antitopo_destroy(e)
            h, n_layers = _graph_from_index(self.L, idx, base)
            assert n_layers >= 2  # several layers: the descent runs
            og = self.oracle.Graph(idx)
            assert (og.n, og.dim) == base.shape
            self._dims[d] = dict(base=base, q=q, idx=idx, h=h, og=og, tq=torch.from_numpy(q).cuda())
            torch.cuda.synchronize()
        return self._dims[d]

    def expected(self, d, mode, k, ef):
        """(ids, dists, distcomps) of the oracle for all M_ALL queries"""
        key = (d, mode, k, ef)
        if key not in self._expected:
            w = self.dim(d)
            self._expected[key] = w["og"].query_k(w["q"], k, ef, bool(mode))
        return self._expected[key]

    def close(self):
        for w in self._dims.values():
            self.L.expann_graph_destroy(w["h"])


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    w = _World(tmp_path_factory.mktemp("graph_device"), oracle)
    yield w
    w.close()


@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream()


def _enqueue(L, h, tq, m, k, ef, mode, st, want_dc=True):
    """expann_graph_search_device of the first m rows of tq on torch stream st (None: the handle's own);
    (rc, ids tensor, dists tensor, distcomps tensor or None), outputs pre-filled with a pattern no search writes"""
    import torch
    ids = torch.full((m, k), -2, dtype=torch.int64, device="cuda")
    dists = torch.full((m, k), -1.0, dtype=torch.float32, device="cuda")
    dc = torch.full((m,), -3, dtype=torch.int32, device="cuda") if want_dc else None
    if st is not None:
        st.wait_stream(torch.cuda.current_stream())
    else:
        torch.cuda.synchronize()
    rc = L.expann_graph_search_device(h, tq.data_ptr(), m, k, ef, mode, ids.data_ptr(), dists.data_ptr(),
                                      dc.data_ptr() if want_dc else None, st.cuda_stream if st is not None else None)
    return rc, ids, dists, dc


def _np(ids, dists, dc=None):
    out = (ids.cpu().numpy().view(np.uint64), dists.cpu().numpy())
    return out + ((dc.cpu().numpy().view(np.uint32),) if dc is not None else ())


def _assert_equal(got, exp, m, what):
    """ids, distance bits and (when asked for) per-query distcomps, exactly"""
    oids, od, odc = exp
    assert np.array_equal(got[0], oids[:m]), what
    assert np.array_equal(got[1].view(np.uint32), od[:m].view(np.uint32)), what
    if len(got) > 2:
        assert np.array_equal(got[2].astype(np.uint64), odc[:m]), what


def _stat(L, h, name):
    out = C.c_uint64()
    assert L.expann_graph_get_stat(h, name.encode(), C.byref(out)) == 0
    return out.value


def _search_and_check(world, d, h, mode, ef, st, m=M_PARITY, k=K):
    L, w = world.L, world.dim(d)
    rc, ids, dists, dc = _enqueue(L, h, w["tq"], m, k, ef, mode, st)
    assert rc == 0, L.expann_graph_last_error(h)
    assert L.expann_graph_sync(h) == 0, L.expann_graph_last_error(h)
    _assert_equal(_np(ids, dists, dc), world.expected(d, mode, k, ef), m, (d, mode, ef))
    return ids, dists


@pytest.mark.parametrize("d,mode", [(128, 0), (128, 1), (192, 0), (192, 1), (48, 0)])
def test_parity_with_the_oracle(world, stream, d, mode):
    """compiled (d = 128) and run-time-dim (192, 48) instances, fp32 and uint8 walks; one sync per search; the
    variant without a distcomps buffer returns the same ids and distances"""
    import torch
    L, w = world.L, world.dim(d)
    for ef in EFS:
        ids, dists = _search_and_check(world, d, w["h"], mode, ef, stream)
        assert L.expann_graph_last_kernel_ms(w["h"]) > 0
        rc, ids2, dists2, _ = _enqueue(L, w["h"], w["tq"], M_PARITY, K, ef, mode, stream, want_dc=False)
        assert rc == 0 and L.expann_graph_sync(w["h"]) == 0
        assert torch.equal(ids2, ids) and torch.equal(dists2.view(torch.int32), dists.view(torch.int32)), ef


def test_ranged_mode(world, stream, tmp_path, oracle):
    """mode 2 on a one-layer graph over Gaussian rows == graph_ranged_helpers.ranged_expected"""
    import torch
    from graph_ranged_helpers import build_layer0, graph_create_layer0, ranged_expected
    L = world.L
    rng = np.random.RandomState(64)
    n, d, m = 2000, 64, 64
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((m, d)).astype(np.float32)
    sv, lists0 = build_layer0(L, rows, tmp_path)
    h = graph_create_layer0(L, rows, lists0, sv)
    _, _, exp = ranged_expected(oracle, tmp_path, rows, lists0, sv, q, K, EFS)
    tq = torch.from_numpy(q).cuda()
    for ef in EFS:
        rc, ids, dists, dc = _enqueue(L, h, tq, m, K, ef, 2, stream)
        assert rc == 0, L.expann_graph_last_error(h)
        assert L.expann_graph_sync(h) == 0, L.expann_graph_last_error(h)
        _assert_equal(_np(ids, dists, dc), exp[ef], m, ef)
    L.expann_graph_destroy(h)


@pytest.mark.parametrize("mode", [0, 1])
def test_redo_on_the_device(world, stream, mode):
    """a first launch with a heap of 8 overflows; the redo launch walks those queries again and every row equals
    the oracle's; a redone query's distcomps are counted once"""
    L, w = world.L, world.dim(128)
    h = w["h"]
    assert L.expann_graph_set_option(h, b"cand_capacity", 8) == 0
    try:
        before = _stat(L, h, "distcomps")
        _search_and_check(world, 128, h, mode, 40, stream)
        redone = _stat(L, h, "redo_queries")
        assert 0 < redone <= M_PARITY
        assert _stat(L, h, "distcomps") - before == int(world.expected(128, mode, K, 40)[2][:M_PARITY].sum())
    finally:
        assert L.expann_graph_set_option(h, b"cand_capacity", 0) == 0
    _search_and_check(world, 128, h, mode, 40, stream)
    assert _stat(L, h, "redo_queries") == 0  # (the automatic capacity holds these walks)


def test_overflow_is_reported_and_leaves_the_handle_clean(world, stream):
    from expann_amd import _lib
    L, w = world.L, world.dim(128)
    h = w["h"]
    overflows = _stat(L, h, "redo_overflows")
    assert L.expann_graph_set_option(h, b"cand_capacity", 8) == 0
    assert L.expann_graph_set_option(h, b"redo_capacity", 16) == 0
    try:
        rc, ids, dists, dc = _enqueue(L, h, w["tq"], M_PARITY, K, 40, 0, stream)
        assert rc == 0, L.expann_graph_last_error(h)
        assert L.expann_graph_sync(h) == _lib.ERR_OVERFLOW
        assert b"overflow" in L.expann_graph_last_error(h)
        assert _stat(L, h, "redo_overflows") == overflows + 1
        assert L.expann_graph_sync(h) == 0  # reported once
    finally:
        assert L.expann_graph_set_option(h, b"cand_capacity", 0) == 0
        assert L.expann_graph_set_option(h, b"redo_capacity", 0) == 0
    for mode in (0, 1):  # visited sets and counters were left clean
        _search_and_check(world, 128, h, mode, 40, stream)
    assert _stat(L, h, "redo_overflows") == overflows + 1


def _host_call_and_check(world, d, h, mode, ef, what, m=M_PARITY, k=K):
    """a host-buffer call (expann_graph_search_mode) that must succeed and equal the oracle"""
    from graph_ranged_helpers import search_mode
    L, w = world.L, world.dim(d)
    rc, ids, dists, dc = search_mode(L, h, w["q"][:m], k, ef, mode)
    assert rc == 0, (what, L.expann_graph_last_error(h))
    _assert_equal((ids, dists, dc), world.expected(d, mode, k, ef), m, what)


@pytest.mark.parametrize("d,mode", [(128, 0), (128, 1), (192, 0)])
def test_host_buffer_call_redoes_overflowed_queries(world, d, mode):
    """a heap of 8 overflows in the first launch of a host-buffer call; without a redo launch that is final
    (EXPANN_ERR_OVERFLOW), so rc == 0 with the oracle's rows shows that the redo launch served those queries"""
    L, h = world.L, world.dim(d)["h"]
    assert L.expann_graph_set_option(h, b"cand_capacity", 8) == 0
    try:
        _host_call_and_check(world, d, h, mode, 40, "heap of 8")
        assert L.expann_graph_last_kernel_ms(h) > 0
    finally:
        assert L.expann_graph_set_option(h, b"cand_capacity", 0) == 0
    _host_call_and_check(world, d, h, mode, 40, "automatic capacity")


def test_host_buffer_call_reports_a_final_overflow(world, stream):
    from expann_amd import _lib
    from graph_ranged_helpers import search_mode
    L, w = world.L, world.dim(128)
    h = w["h"]
    assert L.expann_graph_set_option(h, b"cand_capacity", 8) == 0
    assert L.expann_graph_set_option(h, b"redo_capacity", 16) == 0
    try:
        rc, _, _, _ = search_mode(L, h, w["q"][:M_PARITY], K, 40, 0)
        assert rc == _lib.ERR_OVERFLOW
        assert b"overflow" in L.expann_graph_last_error(h)
    finally:
        assert L.expann_graph_set_option(h, b"cand_capacity", 0) == 0
        assert L.expann_graph_set_option(h, b"redo_capacity", 0) == 0
    # visited sets and counters were left clean, for both entry points
    _host_call_and_check(world, 128, h, 0, 40, "host-buffer call after the overflow")
    _search_and_check(world, 128, h, 0, 40, stream)


def test_entry_points_keep_their_reports_apart(world, stream):
    """a device search that ends in overflow, not yet synced; a host-buffer call in between succeeds and neither
    takes that report nor adds to the device-buffer statistics; the next sync reports the overflow exactly once"""
    from expann_amd import _lib
    L, w = world.L, world.dim(128)
    h = w["h"]
    assert L.expann_graph_sync(h) == 0
    assert L.expann_graph_set_option(h, b"cand_capacity", 8) == 0
    assert L.expann_graph_set_option(h, b"redo_capacity", 16) == 0
    try:
        rc, ids, dists, dc = _enqueue(L, h, w["tq"], M_PARITY, K, 40, 0, stream)
        assert rc == 0, L.expann_graph_last_error(h)
    finally:
        assert L.expann_graph_set_option(h, b"cand_capacity", 0) == 0
        assert L.expann_graph_set_option(h, b"redo_capacity", 0) == 0
    deferred, distcomps = _stat(L, h, "deferred_searches"), _stat(L, h, "distcomps")
    _host_call_and_check(world, 128, h, 0, 40, "host-buffer call before the sync")
    assert _stat(L, h, "deferred_searches") == deferred
    assert _stat(L, h, "distcomps") == distcomps
    assert L.expann_graph_sync(h) == _lib.ERR_OVERFLOW
    assert b"overflow" in L.expann_graph_last_error(h)
    assert L.expann_graph_sync(h) == 0
    assert _stat(L, h, "deferred_searches") == deferred
    # the device total behind "distcomps" does not see a host-buffer call either
    distcomps = _stat(L, h, "distcomps")
    _host_call_and_check(world, 128, h, 0, 40, "host-buffer call after the sync")
    _search_and_check(world, 128, h, 0, 40, stream)
    assert _stat(L, h, "distcomps") - distcomps == int(world.expected(128, 0, K, 40)[2][:M_PARITY].sum())


def test_searches_in_flight(world, stream):
    """eight searches on one stream and one sync; then a second stream, and a host-buffer call issued while a
    device search is outstanding"""
    import torch
    from graph_ranged_helpers import search_mode
    L, w = world.L, world.dim(128)
    h = w["h"]
    deferred = _stat(L, h, "deferred_searches")
    shapes = [(1, 1, 10), (7, 10, 40), (64, 32, 10), (300, 10, 10), (1, 32, 40), (7, 1, 40), (64, 10, 40), (300, 32, 40)]
    assert any(k > ef for _, k, ef in shapes)
    runs = []
    for m, k, ef in shapes:
        rc, ids, dists, dc = _enqueue(L, h, w["tq"], m, k, ef, 0, stream)
        assert rc == 0, L.expann_graph_last_error(h)
        runs.append((m, k, ef, ids, dists, dc))
    assert L.expann_graph_sync(h) == 0, L.expann_graph_last_error(h)
    for m, k, ef, ids, dists, dc in runs:
        got, exp = _np(ids, dists, dc), world.expected(128, 0, k, ef)
        _assert_equal(got, exp, m, (m, k, ef))
        if k > ef:  # padded as the oracle pads
            assert (got[0][:, ef:] == PAD).all() and np.isinf(got[1][:, ef:]).all()
    # a second stream: waits for what is outstanding on the first by itself
    rc, ids_a, dists_a, dc_a = _enqueue(L, h, w["tq"], 64, K, 40, 0, stream)
    assert rc == 0
    second = torch.cuda.Stream()
    rc, ids_b, dists_b, dc_b = _enqueue(L, h, w["tq"], M_PARITY, K, 10, 0, second)
    assert rc == 0, L.expann_graph_last_error(h)
    # a host-buffer call while the search on the second stream is outstanding
    rc, hids, hdists, hdc = search_mode(L, h, w["q"][:M_PARITY], K, 40, 1)
    assert rc == 0, L.expann_graph_last_error(h)
    _assert_equal((hids, hdists, hdc), world.expected(128, 1, K, 40), M_PARITY, "host-buffer call")
    assert L.expann_graph_sync(h) == 0, L.expann_graph_last_error(h)
    _assert_equal(_np(ids_a, dists_a, dc_a), world.expected(128, 0, K, 40), 64, "first stream")
    _assert_equal(_np(ids_b, dists_b, dc_b), world.expected(128, 0, K, 10), M_PARITY, "second stream")
    assert _stat(L, h, "deferred_searches") == deferred + len(shapes) + 2


def test_epoch_byte_visited_sets(world, stream, monkeypatch):
    """the same walks with one epoch byte per vertex instead of the bitsets"""
    L, w = world.L, world.dim(128)
    monkeypatch.setenv("EXPANN_GRAPH_VISITED_BYTES", "1")
    h, _ = _graph_from_index(L, w["idx"], w["base"])
    try:
        for ef in EFS:
            _search_and_check(world, 128, h, 0, ef, stream)
    finally:
        L.expann_graph_destroy(h)


def test_argument_errors_on_a_live_handle(world, stream):
    from expann_amd import _lib
    L = world.L
    w, w48 = world.dim(128), world.dim(48)
    h = w["h"]

    def rc_of(h, w, m, k, ef, mode, null_ids=False):
        import torch
        ids = torch.zeros((max(m, 1), max(k, 1)), dtype=torch.int64, device="cuda")
        dists = torch.zeros((max(m, 1), max(k, 1)), dtype=torch.float32, device="cuda")
        return L.expann_graph_search_device(h, w["tq"].data_ptr(), m, k, ef, mode, None if null_ids else ids.data_ptr(),
                                            dists.data_ptr(), None, stream.cuda_stream)
    deferred = _stat(L, h, "deferred_searches")
    assert rc_of(h, w, 4, 0, 10, 0) == _lib.ERR_INVALID_ARG
    assert rc_of(h, w, 4, 10, 0, 0) == _lib.ERR_INVALID_ARG
    assert rc_of(h, w, 4, 10, 4097, 0) == _lib.ERR_UNSUPPORTED
    assert rc_of(h, w, 4, 10, 10, 3) == _lib.ERR_INVALID_ARG
    assert rc_of(w48["h"], w48, 4, 10, 10, 1) == _lib.ERR_UNSUPPORTED
    assert b"64" in L.expann_graph_last_error(w48["h"])
    assert rc_of(h, w, 4, 10, 10, 0, null_ids=True) == _lib.ERR_INVALID_ARG
    assert rc_of(h, w, 0, 10, 10, 0) == _lib.OK
    assert _stat(L, h, "deferred_searches") == deferred  # none of them enqueued anything
    assert L.expann_graph_set_option(h, b"cand_capacity", 12) == _lib.ERR_INVALID_ARG
    assert L.expann_graph_set_option(h, b"redo_capacity", 16384) == _lib.ERR_INVALID_ARG
    assert L.expann_graph_set_option(h, b"no_such_option", 0) == _lib.ERR_INVALID_ARG
    out = C.c_uint64()
    assert L.expann_graph_get_stat(h, b"no_such_stat", C.byref(out)) == _lib.ERR_INVALID_ARG
    assert L.expann_graph_sync(h) == 0
    _search_and_check(world, 128, h, 0, 10, stream)  # the handle still answers


def test_engine_surface(world, stream):
    """AntitopoEngine.query_many_device + sync() == query_many of the same engine and the oracle; the sticky ef
    comes from the first k; set_compression("cast"); num_distcomps grows by the oracle's count across sync()"""
    import torch
    from expann_amd import AntitopoEngine, _lib
    w = world.dim(128)
    fresh = AntitopoEngine(16, 80, 1, 0, False, dim=128)
    tq = w["tq"]

    def device_query(eng, m, k):
        ids = torch.full((m, k), -2, dtype=torch.int64, device="cuda")
        dists = torch.full((m, k), -1.0, dtype=torch.float32, device="cuda")
        stream.wait_stream(torch.cuda.current_stream())
        eng.query_many_device(tq.data_ptr(), m, k, ids.data_ptr(), dists.data_ptr(), stream.cuda_stream)
        return ids, dists
    with pytest.raises(_lib.ExpannError) as ei:
        device_query(fresh, 8, K)
    assert ei.value.code == _lib.ERR_NOT_BUILT
    fresh.load_index(w["idx"])
    m = 64
    # the first k makes ef_search = 10; k = 5 afterwards still walks with 10
    for k, mode, name in ((10, 0, None), (5, 0, None), (5, 1, "cast")):
        if name:
            fresh.set_compression(name)
        before = int(fresh.param_list()["num_distcomps"])
        ids, dists = device_query(fresh, m, k)
        fresh.sync()
        counted = int(fresh.param_list()["num_distcomps"]) - before
        exp = world.expected(128, mode, k, 10)
        _assert_equal(_np(ids, dists), exp, m, (k, mode))
        assert counted == int(exp[2][:m].sum()), (k, mode)
        hids, hdists = fresh.query_many(w["q"][:m], k)
        _assert_equal((hids, hdists), exp, m, ("query_many", k, mode))
    fresh.close()


# ---- the handle's state over its lifetime -------------------------------------------------------------
LIFE_N, LIFE_D, LIFE_M, LIFE_EF = 4096, 64, 8, 40


class _Life:
    """4 096 rows, d = 64, M = 16: one serial build, its index file, the restatement of the walk
    (graph_filter_helpers, graph_groups_helpers), a filter that allows every second row, one that allows 7 rows,
    and two labellings"""

    def __init__(self, tmp, oracle, L):
        import torch
        import graph_filter_helpers as H
        import graph_groups_helpers as G
        from expann_amd import pack_row_filter
        self.L, self.H, self.G = L, H, G
        rng = np.random.RandomState(4096)
        self.base = _sift_like(rng, LIFE_N, LIFE_D)
        self.q = _sift_like(rng, LIFE_M, LIFE_D, frac=True)
        self.idx = str(tmp / "life.index")
        e = C.c_void_p()
        assert L.expann_antitopo_create(LIFE_D, 0, 16, 80, 1, 0, 0, C.byref(e)) == 0
        assert L.expann_antitopo_store(e, self.base.ctypes.data, LIFE_N) == 0
        assert L.expann_antitopo_save(e, self.idx.encode()) == 0
        L.expann_antitopo_destroy(e)
        self.g = H.IndexGraph(self.idx)
        self.Df = H.dist_f32_matrix(oracle, self.base, self.q)
        self._Db = {m: H.bottom_matrix(oracle, self.base, self.q, m, self.Df) for m in (0, 1, 2)}
        self.R = G.Restatement(self.g, self.Df, lambda mode: self._Db[mode])
        self.dense = np.arange(LIFE_N) % 2 == 0
        self.few = np.zeros(LIFE_N, bool)
        self.few[rng.choice(LIFE_N, 7, replace=False)] = True
        self.words = {name: pack_row_filter(a) for name, a in (("dense", self.dense), ("few", self.few))}
        self.labels = {"main": G.make_labels(LIFE_N), "other": G.other_labels(LIFE_N)}
        self.qg = G.query_groups(LIFE_M)
        self.tq = torch.from_numpy(self.q).cuda()
        self.tqg = torch.from_numpy(self.qg.view(np.int32)).cuda()
        torch.cuda.synchronize()

    def create(self):
        return _graph_from_index(self.L, self.idx, self.base)[0]

    def walk(self, mode, allow=None):
        ids, dists, dc, _ = self.H.walk(self.g, self.Df, self._Db[mode], allow, K, LIFE_EF, mode)
        return ids, dists, dc

    def scan(self, allow):
        """the exact scan of the allowed rows: the min(k, allowed) smallest (distance, id), distcomps = allowed"""
        ids = np.full((LIFE_M, K), PAD, np.uint64)
        dists = np.full((LIFE_M, K), np.inf, np.float32)
        dc = np.zeros(LIFE_M, np.uint64)
        for i in range(LIFE_M):
            oi, od, dc[i] = self.G.scan_one(self.Df[i], allow.astype(np.uint32), 1, K)
            ids[i, :len(oi)], dists[i, :len(od)] = oi, od
        return ids, dists, dc

    def set_filter(self, h, name):
        w = self.words[name]
        assert self.L.expann_graph_set_row_filter(h, w.ctypes.data, w.size) == 0, self.L.expann_graph_last_error(h)

    def set_groups(self, h, name):
        lab = self.labels[name]
        assert self.L.expann_graph_set_row_groups(h, lab.ctypes.data, lab.size) == 0, self.L.expann_graph_last_error(h)

    def device(self, h, mode, st):
        rc, ids, dists, dc = _enqueue(self.L, h, self.tq, LIFE_M, K, LIFE_EF, mode, st)
        assert rc == 0, self.L.expann_graph_last_error(h)
        assert self.L.expann_graph_sync(h) == 0, self.L.expann_graph_last_error(h)
        return _np(ids, dists, dc)

    def host(self, h, mode):
        from graph_ranged_helpers import search_mode
        rc, ids, dists, dc = search_mode(self.L, h, self.q, K, LIFE_EF, mode)
        assert rc == 0, self.L.expann_graph_last_error(h)
        return ids, dists, dc

    def grouped_device(self, h, mode, st):
        import torch
        ids = torch.full((LIFE_M, K), -2, dtype=torch.int64, device="cuda")
        dists = torch.full((LIFE_M, K), -1.0, dtype=torch.float32, device="cuda")
        dc = torch.full((LIFE_M,), -3, dtype=torch.int32, device="cuda")
        st.wait_stream(torch.cuda.current_stream())
        rc = self.L.expann_graph_search_grouped_device(h, self.tq.data_ptr(), self.tqg.data_ptr(), LIFE_M, K, LIFE_EF, mode,
                                                       ids.data_ptr(), dists.data_ptr(), dc.data_ptr(), st.cuda_stream)
        assert rc == 0, self.L.expann_graph_last_error(h)
        assert self.L.expann_graph_sync(h) == 0, self.L.expann_graph_last_error(h)
        return _np(ids, dists, dc)

    def grouped_host(self, h, mode):
        ids, dists, dc = np.zeros((LIFE_M, K), np.uint64), np.zeros((LIFE_M, K), np.float32), np.zeros(LIFE_M, np.uint32)
        rc = self.L.expann_graph_search_grouped(h, self.q.ctypes.data, self.qg.ctypes.data, LIFE_M, K, LIFE_EF, mode,
                                                ids.ctypes.data, dists.ctypes.data, dc.ctypes.data)
        assert rc == 0, self.L.expann_graph_last_error(h)
        return ids, dists, dc


@pytest.fixture(scope="module")
def life(tmp_path_factory, oracle):
    from expann_amd import _lib
    return _Life(tmp_path_factory.mktemp("graph_life"), oracle, _lib.load())


def test_state_set_and_forgotten_leaves_the_handle_as_it_was(life, stream):
    """filter, groups and the byte copies come and go between two plain searches, and the second equals the first
    bit for bit; every search in between equals the restatement of what is in force at that moment"""
    L, h = life.L, life.create()
    try:
        first_dev, first_host = life.device(h, 0, stream), life.host(h, 0)
        for got in (first_dev, first_host):
            _assert_equal(got, life.walk(0), LIFE_M, "first search")
        # a dense filter is walked ("filter_flat_rows" = 1: only a 1-row filter would be scanned) ...
        assert L.expann_graph_set_option(h, b"filter_flat_rows", 1) == 0
        life.set_filter(h, "dense")
        assert (_stat(L, h, "filter_active"), _stat(L, h, "filter_rows")) == (1, LIFE_N // 2)
        for got in (life.device(h, 0, stream), life.host(h, 0)):
            _assert_equal(got, life.walk(0, life.dense), LIFE_M, "dense filter")
        # ... and one of fewer than k rows is scanned, on auto
        assert L.expann_graph_set_option(h, b"filter_flat_rows", 0) == 0
        life.set_filter(h, "few")
        assert _stat(L, h, "filter_rows") == 7
        flat = _stat(L, h, "flat_searches")
        for got in (life.device(h, 0, stream), life.host(h, 0)):
            _assert_equal(got, life.scan(life.few), LIFE_M, "filter of 7 rows")
        assert _stat(L, h, "flat_searches") == flat + 2
        assert L.expann_graph_clear_row_filter(h) == 0
        for name in ("main", "other"):  # groups, forgotten, other groups, forgotten
            life.set_groups(h, name)
            assert _stat(L, h, "groups_active") == 1
            assert _stat(L, h, "group_count") == len(set(life.labels[name].tolist()) - {0xFFFFFFFF})
            exp = life.R.expected(life.labels[name], life.qg, K, LIFE_EF, 0, 0, labels_key=name)[:3]
            _assert_equal(life.grouped_device(h, 0, stream), exp, LIFE_M, (name, "grouped, device buffers"))
            _assert_equal(life.grouped_host(h, 0), exp, LIFE_M, (name, "grouped, host buffers"))
            assert L.expann_graph_clear_row_groups(h) == 0
            assert (_stat(L, h, "groups_active"), _stat(L, h, "group_count")) == (0, 0)
        for mode in (2, 1):  # the byte copies are made here
            _assert_equal(life.device(h, mode, stream), life.walk(mode), LIFE_M, ("mode", mode))
        last_dev, last_host = life.device(h, 0, stream), life.host(h, 0)
        for first, last in ((first_dev, last_dev), (first_host, last_host)):
            assert np.array_equal(first[0], last[0])
            assert np.array_equal(first[1].view(np.uint32), last[1].view(np.uint32))
            assert np.array_equal(first[2], last[2])
        assert [_stat(L, h, s) for s in ("filter_active", "groups_active", "group_count")] == [0, 0, 0]
    finally:
        L.expann_graph_destroy(h)


def test_a_destroyed_handle_gives_its_device_memory_back(life, stream):
    """20 times: create, filter, searches in every mode on both kinds of buffers, groups, grouped searches, a filter
    again, destroy.  Free device memory after the 20th cycle is within one handle's footprint -- rows, layer-0 lists
    at their stride, visited sets -- of what it was after the first: a group of the handle that stopped freeing
    itself would lose twenty.  This catches a leaked large buffer, not a leaked event or stream."""
    import torch
    L = life.L
    stride0 = max(4, (max(len(x) for x in life.g.adj[0]) + 3) // 4 * 4)
    slots = torch.cuda.get_device_properties(0).multi_processor_count * 16
    vis_bytes = (LIFE_N + 8191) // 8192 * 256 * 4  # one bitset
    footprint = LIFE_N * LIFE_D * 4 + LIFE_N * stride0 * 4 + slots * vis_bytes
    assert slots * vis_bytes >= 4 << 20 and footprint < 8 << 20
    free = []
    for cycle in range(20):
        h = life.create()
        assert L.expann_graph_set_option(h, b"filter_flat_rows", 1) == 0  # (the dense filter is walked: byte copies)
        life.set_filter(h, "dense")
        for mode in (0, 1, 2):
            life.device(h, mode, stream)
            life.host(h, mode)
        assert L.expann_graph_clear_row_filter(h) == 0
        assert L.expann_graph_set_option(h, b"filter_flat_rows", 0) == 0
        life.set_groups(h, "main")
        for mode in (0, 1, 2):
            life.grouped_device(h, mode, stream)
            life.grouped_host(h, mode)
        life.set_filter(h, "few")
        L.expann_graph_destroy(h)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print(f"free device memory after cycle 1: {free[0]}, after cycle 20: {free[-1]}; one handle: {footprint}")
    assert abs(free[0] - free[-1]) < footprint
