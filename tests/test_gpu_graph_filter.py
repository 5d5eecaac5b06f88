"""Row filter of the graph engine (expann_graph_set_row_filter and the calls on top of it) on the GPU.  Ids, distance
bits and per-query distcomps of a filtered walk are compared with the Python restatement of THE FILTER RULE in
tests/graph_filter_helpers.py (pinned on the CPU by tests/test_graph_filter_abi.py), through both the host-buffer
and the device-buffer entry point; the scan of a sparse filter with oracle.brute_force over the allowed rows.  The
one device-to-device comparison is the all-ones filter against the handle's own unfiltered answer."""
import ctypes as C

import numpy as np
import pytest

import graph_filter_helpers as H

pytestmark = pytest.mark.gpu

K, EFS, M = H.K, (10, 40), H.M_FILTER
PAD = H.PAD


class _Case:
    """a graph handle, its restatement and the distance matrices of its queries"""

    def __init__(self, L, oracle, h, g, base, q, ends=None):
        import torch
        self.L, self.oracle, self.h, self.g, self.base, self.q = L, oracle, h, g, base, q
        self.n = base.shape[0]
        self.Df = H.dist_f32_matrix(oracle, base, q)
        self._Db, self._exp = {0: self.Df}, {}
        self.ends = H.descent_ends(g, self.Df) if ends is None else ends
        self.filters = H.make_filters(self.n, self.ends, g.sv)
        self.tq = torch.from_numpy(q).cuda()
        torch.cuda.synchronize()

    def Db(self, mode):
        if mode not in self._Db:
            self._Db[mode] = H.bottom_matrix(self.oracle, self.base, self.q, mode, self.Df)
        return self._Db[mode]

    def expected(self, allow_key, allow, mode, ef, k=K):
        """(ids, dists, distcomps, peak) of the restatement, computed once per case"""
        key = (allow_key, mode, ef, k)
        if key not in self._exp:
            self._exp[key] = H.walk(self.g, self.Df, self.Db(mode), allow, k, ef, mode)
        return self._exp[key]


class _World:
    def __init__(self, tmp, oracle):
        from expann_amd import _lib
        self.tmp, self.oracle, self.L = tmp, oracle, _lib.load()
        self._cases = {}

    def _built(self, key, base, M_, efc):
        """serial build through the C ABI at exactly the rows' dim; (index path, handle)"""
        L = self.L
        idx = str(self.tmp / f"f_{key}.index")
        e = C.c_void_p()
        assert L.expann_antitopo_create(base.shape[1], 0, M_, efc, 1, 0, 0, C.byref(e)) == 0
        assert L.expann_antitopo_store(e, base.ctypes.data, base.shape[0]) == 0
        assert L.expann_antitopo_save(e, idx.encode()) == 0
        L.expann_antitopo_destroy(e)
        return idx, H.graph_from_index(L, idx, base)

    def dim(self, d):
        """n = 3000, M = 16, ef_construction = 80, several layers"""
        if d not in self._cases:
            rng = np.random.RandomState(1000 + d)
            base = H.sift_like(rng, H.N_ROWS, d)
            q = H.sift_like(rng, M, d, frac=True)
            idx, h = self._built(d, base, 16, 80)
            g = H.IndexGraph(idx)
            assert g.n_layers >= 2
            c = _Case(self.L, self.oracle, h, g, base, q)
            c.idx, c.og = idx, self.oracle.Graph(idx)
            self._cases[d] = c
        return self._cases[d]

    def ranged(self):
        """the one-layer d = 64 graph over Gaussian rows of the ranged test (mode 2)"""
        if "ranged" not in self._cases:
            from graph_ranged_helpers import build_layer0, graph_create_layer0
            rng = np.random.RandomState(64)
            n, d = 2000, 64
            rows = rng.standard_normal((n, d)).astype(np.float32)
            q = rng.standard_normal((M, d)).astype(np.float32)
            sv, lists0 = build_layer0(self.L, rows, self.tmp)
            h = graph_create_layer0(self.L, rows, lists0, sv)
            g = H.IndexGraph.single_layer(lists0, sv)
            self._cases["ranged"] = _Case(self.L, self.oracle, h, g, rows, q, ends=np.full(M, sv, np.int64))
        return self._cases["ranged"]

    def long_lists(self):
        """n = 2000, M = 40: bottom-layer lists longer than a wavefront"""
        if "long" not in self._cases:
            rng = np.random.RandomState(40)
            base = H.sift_like(rng, 2000, 128)
            q = H.sift_like(rng, M, 128, frac=True)
            idx, h = self._built("long", base, 40, 120)
            g = H.IndexGraph(idx)
            assert max(len(x) for x in g.adj[0]) > 64
            self._cases["long"] = _Case(self.L, self.oracle, h, g, base, q)
        return self._cases["long"]

    def close(self):
        for c in self._cases.values():
            self.L.expann_graph_destroy(c.h)


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    w = _World(tmp_path_factory.mktemp("graph_filter"), oracle)
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


def _set(c, words, flat_rows=1):
    L = c.L
    assert L.expann_graph_set_option(c.h, b"filter_flat_rows", flat_rows) == 0
    assert L.expann_graph_set_row_filter(c.h, words.ctypes.data, words.size) == 0, L.expann_graph_last_error(c.h)


def _enqueue(c, m, k, ef, mode, st):
    """expann_graph_search_device of the first m queries on torch stream st; (rc, ids, dists, distcomps) tensors,
    pre-filled with a pattern no search writes"""
    import torch
    ids = torch.full((m, k), -2, dtype=torch.int64, device="cuda")
    dists = torch.full((m, k), -1.0, dtype=torch.float32, device="cuda")
    dc = torch.full((m,), -3, dtype=torch.int32, device="cuda")
    st.wait_stream(torch.cuda.current_stream())
    rc = c.L.expann_graph_search_device(c.h, c.tq.data_ptr(), m, k, ef, mode, ids.data_ptr(), dists.data_ptr(),
                                        dc.data_ptr(), st.cuda_stream)
    return rc, ids, dists, dc


def _np(ids, dists, dc):
    return ids.cpu().numpy().view(np.uint64), dists.cpu().numpy(), dc.cpu().numpy().view(np.uint32)


def _device(c, k, ef, mode, st, m=M):
    rc, ids, dists, dc = _enqueue(c, m, k, ef, mode, st)
    assert rc == 0, c.L.expann_graph_last_error(c.h)
    assert c.L.expann_graph_sync(c.h) == 0, c.L.expann_graph_last_error(c.h)
    return _np(ids, dists, dc)


def _host(c, k, ef, mode, m=M):
    from graph_ranged_helpers import search_mode
    rc, ids, dists, dc = search_mode(c.L, c.h, c.q[:m], k, ef, mode)
    assert rc == 0, c.L.expann_graph_last_error(c.h)
    return ids, dists, dc


def _assert_equal(got, exp, what):
    """ids, distance bits and per-query distcomps, exactly"""
    m = got[0].shape[0]
    assert np.array_equal(got[0], exp[0][:m]), what
    assert np.array_equal(got[1].view(np.uint32), exp[1][:m].view(np.uint32)), what
    assert np.array_equal(got[2].astype(np.uint64), exp[2][:m]), what


def _check_filters(c, mode, st, names=H.FILTER_NAMES, efs=EFS):
    L = c.L
    try:
        for name in names:
            allow, words = c.filters[name]
            _set(c, words)
            assert _stat(L, c.h, "filter_active") == 1 and _stat(L, c.h, "filter_rows") == int(allow.sum())
            for ef in efs:
                exp = c.expected(name, allow, mode, ef)
                _assert_equal(_device(c, K, ef, mode, st), exp, (name, ef, "device buffers"))
                _assert_equal(_host(c, K, ef, mode), exp, (name, ef, "host buffers"))
                if name == "ones":  # the rule reduces to the unfiltered walk: the handle's own answer
                    assert L.expann_graph_clear_row_filter(c.h) == 0
                    _assert_equal(_device(c, K, ef, mode, st), exp, (name, ef, "no filter"))
                    _set(c, words)
    finally:
        assert L.expann_graph_clear_row_filter(c.h) == 0
        assert L.expann_graph_set_option(c.h, b"filter_flat_rows", 0) == 0
    assert _stat(L, c.h, "filter_active") == 0 and _stat(L, c.h, "filter_rows") == c.n


@pytest.mark.parametrize("d,mode", [(128, 0), (128, 1), (192, 0), (192, 1), (48, 0)])
def test_filtered_walk_equals_the_restatement(world, stream, d, mode):
    """compiled (d = 128) and run-time-dim (192, 48) instances, fp32 and uint8 walks, every filter of
    graph_filter_helpers.make_filters, "filter_flat_rows" = 1 (always walk)"""
    c = world.dim(d)
    flat = _stat(c.L, c.h, "flat_searches")
    _check_filters(c, mode, stream)
    assert _stat(c.L, c.h, "flat_searches") == flat  # every one of them walked
    # the restatement without a filter is the oracle's walk of the same index file
    oids, od, odc = c.og.query_k(c.q, K, 40, bool(mode))
    _assert_equal((oids, od, odc), c.expected("none", None, mode, 40), "oracle")


def test_filtered_walk_in_the_ranged_mode(world, stream):
    """mode 2 on the one-layer d = 64 graph of the ranged test"""
    _check_filters(world.ranged(), 2, stream)


def test_lists_longer_than_a_wavefront(world, stream):
    _check_filters(world.long_lists(), 0, stream, names=("every_second",))


def test_redo_under_a_filter(world, stream):
    """a first heap of the largest power of two below the restatement's peak for the 10 % filter: some but not all
    queries overflow it, the redo launch serves exactly those, the results do not change; a redo capacity below the
    peak is EXPANN_ERR_OVERFLOW at the sync and leaves the handle usable"""
    from expann_amd import _lib
    c = world.dim(128)
    L, h = c.L, c.h
    allow, words = c.filters["random_10"]
    ef = 10
    exp = c.expected("random_10", allow, 0, ef)
    peak = exp[3]
    cap = 1 << (int(peak.max() - 1).bit_length() - 1)
    n_over = int((peak > cap).sum())
    assert cap < peak.max() and 0 < n_over < M
    try:
        _set(c, words)
        assert L.expann_graph_set_option(h, b"cand_capacity", cap) == 0
        _assert_equal(_device(c, K, ef, 0, stream), exp, "device buffers")
        assert _stat(L, h, "redo_queries") == n_over
        _assert_equal(_host(c, K, ef, 0), exp, "host buffers")
        overflows = _stat(L, h, "redo_overflows")
        assert 16 < peak.min()  # both capacities below every query's peak
        assert L.expann_graph_set_option(h, b"cand_capacity", 8) == 0
        assert L.expann_graph_set_option(h, b"redo_capacity", 16) == 0
        rc, ids, dists, dc = _enqueue(c, M, K, ef, 0, stream)
        assert rc == 0, L.expann_graph_last_error(h)
        assert L.expann_graph_sync(h) == _lib.ERR_OVERFLOW
        assert b"overflow" in L.expann_graph_last_error(h)
        assert _stat(L, h, "redo_overflows") == overflows + 1
        assert L.expann_graph_sync(h) == 0
        assert L.expann_graph_set_option(h, b"cand_capacity", 0) == 0
        assert L.expann_graph_set_option(h, b"redo_capacity", 0) == 0
        _assert_equal(_device(c, K, ef, 0, stream), exp, "after the overflow")  # visited sets and counters are clean
    finally:
        assert L.expann_graph_set_option(h, b"cand_capacity", 0) == 0
        assert L.expann_graph_set_option(h, b"redo_capacity", 0) == 0
        assert L.expann_graph_clear_row_filter(h) == 0
        assert L.expann_graph_set_option(h, b"filter_flat_rows", 0) == 0


def _scan_expected(c, allow, k):
    """oracle.brute_force over base[allowed], ids mapped back, padded"""
    rows = np.flatnonzero(allow)
    ids = np.full((M, k), PAD, np.uint64)
    dists = np.full((M, k), np.inf, np.float32)
    if rows.size:
        kk = min(k, rows.size)
        bi, bd = c.oracle.brute_force(c.base[rows], c.q, kk, c.oracle.METRIC_L2_F32, n_threads=4)
        ids[:, :kk] = rows[bi.astype(np.int64)].astype(np.uint64)
        dists[:, :kk] = bd
    return ids, dists, np.full(M, rows.size, np.uint64)


@pytest.mark.parametrize("d", [128, 192])
def test_sparse_filters_are_scanned(world, stream, d):
    from expann_amd import pack_row_filter
    c = world.dim(d)
    L, h = c.L, c.h
    rng = np.random.RandomState(300)
    try:
        for count in (0, 1, 7, 300):
            allow = np.zeros(c.n, bool)
            allow[rng.choice(c.n, count, replace=False)] = True
            if count == 7:
                allow[:] = False
                allow[[0, 31, 32, 1500, 2975, 2976, c.n - 1]] = True  # word edges and the last row
            _set(c, pack_row_filter(allow), flat_rows=300)
            assert _stat(L, h, "filter_rows") == count
            exp = _scan_expected(c, allow, K)
            for mode in (0, 1):  # the scan is fp32 whatever the mode
                flat = _stat(L, h, "flat_searches")
                _assert_equal(_device(c, K, 40, mode, stream), exp, (count, mode, "device buffers"))
                _assert_equal(_host(c, K, 40, mode), exp, (count, mode, "host buffers"))
                assert _stat(L, h, "flat_searches") == flat + 2
            if count == 300:
                for k in (1, 64, 300, 301):  # k = 300 keeps every allowed row, 301 pads
                    got = _device(c, k, 40, 0, stream)
                    _assert_equal(got, _scan_expected(c, allow, k), (count, k))
                # the same filter with the option at 1 is walked
                flat = _stat(L, h, "flat_searches")
                assert L.expann_graph_set_option(h, b"filter_flat_rows", 1) == 0
                exp_w = c.expected("sparse_300", allow, 0, 40)
                _assert_equal(_device(c, K, 40, 0, stream), exp_w, "walked")
                _assert_equal(_host(c, K, 40, 0), exp_w, "walked, host buffers")
                assert _stat(L, h, "flat_searches") == flat
                # one row more than the option allows: walked too
                assert L.expann_graph_set_option(h, b"filter_flat_rows", 299) == 0
                _assert_equal(_device(c, K, 40, 0, stream), exp_w, "299 < 300 rows")
                assert _stat(L, h, "flat_searches") == flat
    finally:
        assert L.expann_graph_clear_row_filter(h) == 0
        assert L.expann_graph_set_option(h, b"filter_flat_rows", 0) == 0


def test_set_search_clear_search(world, stream):
    """after the clear the handle answers as the oracle's unfiltered walk; a failed set leaves the filter as it was;
    the option's own validation"""
    from expann_amd import _lib
    c = world.dim(128)
    L, h = c.L, c.h
    allow, words = c.filters["every_second"]
    unf = c.og.query_k(c.q, K, 40, False)
    try:
        _set(c, words)
        exp = c.expected("every_second", allow, 0, 40)
        _assert_equal(_device(c, K, 40, 0, stream), exp, "set")
        # too few words, NULL bits: refused, the filter stays
        assert L.expann_graph_set_row_filter(h, words.ctypes.data, words.size - 1) == _lib.ERR_INVALID_ARG
        assert b"words" in L.expann_graph_last_error(h)
        assert L.expann_graph_set_row_filter(h, None, words.size) == _lib.ERR_INVALID_ARG
        assert L.expann_graph_set_row_filter_device(h, None, words.size, None) == _lib.ERR_INVALID_ARG
        assert _stat(L, h, "filter_active") == 1 and _stat(L, h, "filter_rows") == int(allow.sum())
        _assert_equal(_host(c, K, 40, 0), exp, "after the refused calls")
        # more words than needed are fine
        longer = np.concatenate([words, np.full(3, 0xFFFFFFFF, np.uint32)])
        assert L.expann_graph_set_row_filter(h, longer.ctypes.data, longer.size) == 0
        assert _stat(L, h, "filter_rows") == int(allow.sum())
        assert L.expann_graph_clear_row_filter(h) == 0
        _assert_equal(_device(c, K, 40, 0, stream), unf, "cleared")
        _assert_equal(_host(c, K, 40, 0), unf, "cleared, host buffers")
        assert L.expann_graph_set_option(h, b"filter_flat_rows", -1) == _lib.ERR_INVALID_ARG
        assert L.expann_graph_set_option(h, b"filter_flat_rows", 12) == 0  # a row count: no power-of-two rule
        assert L.expann_graph_set_option(h, b"cand_capacity", 12) == _lib.ERR_INVALID_ARG
    finally:
        assert L.expann_graph_clear_row_filter(h) == 0
        assert L.expann_graph_set_option(h, b"filter_flat_rows", 0) == 0


def test_a_filter_change_waits_for_the_searches_in_flight(world, stream):
    """device searches enqueued before the set keep their unfiltered answers, those after it are filtered; then the
    other way round with the clear"""
    c = world.dim(128)
    L, h = c.L, c.h
    allow, words = c.filters["random_10"]
    unf = c.og.query_k(c.q, K, 40, False)
    exp = c.expected("random_10", allow, 0, 40)
    try:
        before = [_enqueue(c, M, K, 40, 0, stream) for _ in range(4)]
        _set(c, words)
        after = [_enqueue(c, M, K, 40, 0, stream) for _ in range(2)]
        assert L.expann_graph_clear_row_filter(h) == 0
        last = _enqueue(c, M, K, 40, 0, stream)
        assert all(r[0] == 0 for r in before + after + [last])
        assert L.expann_graph_sync(h) == 0, L.expann_graph_last_error(h)
        for r in before:
            _assert_equal(_np(*r[1:]), unf, "enqueued before the set")
        for r in after:
            _assert_equal(_np(*r[1:]), exp, "enqueued under the filter")
        _assert_equal(_np(*last[1:]), unf, "enqueued after the clear")
    finally:
        assert L.expann_graph_clear_row_filter(h) == 0
        assert L.expann_graph_set_option(h, b"filter_flat_rows", 0) == 0


def test_filter_bits_from_a_tensor_on_a_side_stream(world, stream):
    import torch
    c = world.dim(128)
    L, h = c.L, c.h
    allow, words = c.filters["last_word_set"]
    side = torch.cuda.Stream()
    try:
        assert L.expann_graph_set_option(h, b"filter_flat_rows", 1) == 0
        with torch.cuda.stream(side):  # the bits are written on the side stream, and read in its order
            t = torch.zeros(words.size, dtype=torch.int32, device="cuda")
            t.copy_(torch.from_numpy(words.view(np.int32)).cuda(), non_blocking=True)
            rc = L.expann_graph_set_row_filter_device(h, t.data_ptr(), words.size, side.cuda_stream)
        assert rc == 0, L.expann_graph_last_error(h)
        t.zero_()  # the library has its own copy
        torch.cuda.synchronize()
        assert _stat(L, h, "filter_rows") == int(allow.sum())
        _assert_equal(_device(c, K, 40, 0, stream), c.expected("last_word_set", allow, 0, 40), "device bits")
    finally:
        assert L.expann_graph_clear_row_filter(h) == 0
        assert L.expann_graph_set_option(h, b"filter_flat_rows", 0) == 0


def test_engine_surface(world, stream):
    """AntitopoEngine.set_row_filter: NOT_BUILT before build; under a filter every query gets K allowed rows,
    ascending, with the oracle's fp32 distances -- properties that hold whether the engine's automatic
    "filter_flat_rows" sends the filter to the walk or to the scan --; None clears; load_index clears"""
    import torch
    from expann_amd import AntitopoEngine, _lib
    c = world.dim(128)
    eng = AntitopoEngine(16, 80, 1, 0, False, dim=128)
    allow, words = c.filters["every_second"]
    with pytest.raises(_lib.ExpannError) as ei:
        eng.set_row_filter(allow)
    assert ei.value.code == _lib.ERR_NOT_BUILT
    eng.load_index(c.idx)
    eng.set_ef_search(40)
    unf = c.og.query_k(c.q, K, 40, False)

    def check_filtered(ids, dists, what):
        assert (ids != PAD).all(), what  # 1500 allowed rows, all reachable: K results each
        rows = ids.astype(np.int64)
        assert allow[rows].all(), what
        assert np.array_equal(dists.view(np.uint32), np.take_along_axis(c.Df, rows, axis=1).view(np.uint32)), what
        assert (np.diff(dists, axis=1) >= 0).all(), what
        assert not np.array_equal(ids, unf[0]), what  # (the unfiltered answers hold odd rows)

    assert not allow[unf[0].astype(np.int64)].all()
    eng.set_row_filter(allow.astype(np.uint8))
    check_filtered(*eng.query_many(c.q, K), "host bits, host buffers")
    # the device-buffer query under the filter, bits from device memory
    t = torch.from_numpy(words.view(np.int32)).cuda()
    eng.set_row_filter_device(t.data_ptr(), words.size)
    dids = torch.full((M, K), -2, dtype=torch.int64, device="cuda")
    dd = torch.full((M, K), -1.0, dtype=torch.float32, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    eng.query_many_device(c.tq.data_ptr(), M, K, dids.data_ptr(), dd.data_ptr(), stream.cuda_stream)
    eng.sync()
    check_filtered(dids.cpu().numpy().view(np.uint64), dd.cpu().numpy(), "device bits, device buffers")
    with pytest.raises(_lib.ExpannError) as ei:
        eng.set_row_filter(allow[:100])  # too few words for 3000 rows
    assert ei.value.code == _lib.ERR_INVALID_ARG
    eng.set_row_filter(None)
    ids, dists = eng.query_many(c.q, K)
    assert np.array_equal(ids, unf[0]) and np.array_equal(dists.view(np.uint32), unf[1].view(np.uint32))
    eng.set_row_filter(allow)
    eng.load_index(c.idx)  # a run-time property: a load starts without a filter
    ids, dists = eng.query_many(c.q, K)
    assert np.array_equal(ids, unf[0]) and np.array_equal(dists.view(np.uint32), unf[1].view(np.uint32))
    eng.close()
