"""The graph engine over binary16 rows on the GPU (THE F16 ROW RULE, include/expann_hip.h): a handle made by
expann_graph_create_f16 from the halves returns what the handle made by expann_graph_create from (float)row returns
-- ids, fp32 distance bits (compared as uint32) and distcomps -- from every entry point and in every mode.

One serial host build per case (graph_filter_helpers.build_index_cpu, M = 16, ef_construction = 80) over rows that
ARE binary16 values, then two handles over its CSR arrays.  Where the oracle answers (modes 0 and 1:
oracle.Graph.query_k walks the index file of the upcast rows) the fp32 handle is held to it as well; mode 2 has no
multi-layer oracle, so there the fp32 handle is held to the Python restatement of the walk
(graph_filter_helpers.walk, pinned on the CPU by tests/test_graph_filter_abi.py) on the first 48 queries.

The engine-level cases of the issue's CPU list that need an expann_antitopo handle (expann_antitopo_create asks for a
device) are here too: expann_antitopo_set_rows_f16 after a store, the refusal of a NaN and of 70000.0, the saved
file, and the refusal to load rows that are not binary16 values."""
import ctypes as C

import numpy as np
import pytest

import graph_filter_helpers as H

pytestmark = pytest.mark.gpu

K, EFS, M_Q, M_WALK = 10, (10, 40), 300, 48
INVALID_ARG = 1


def _gauss_f16(rng, n, d):
    """Gaussian rows rounded to binary16 (as fp32)"""
    return rng.standard_normal((n, d)).astype(np.float16).astype(np.float32)


def _mixed(rng, n, d, rows=True):
    """Subnormals and mixed magnitudes.  A third of the vectors hold only binary16 subnormals (|x| < 6.1e-5) and
    exact zeros: every distance among them is decided by subnormal components alone, so it changes if anything is
    flushed.  The other vectors mix, component by component, a third subnormals, a tenth exact zeros and values up
    to 1e3.  rows: rounded to binary16; queries stay fp32 at the same scales."""
    sub = rng.randint(1, 1024, size=(n, d)).astype(np.float32) * np.float32(2.0 ** -24) * rng.choice([-1.0, 1.0], size=(n, d))
    if not rows:  # fp32 queries: anywhere in the subnormal range, not on its grid
        sub = (sub * rng.uniform(0.5, 1.0, size=(n, d))).astype(np.float32)
    big = rng.uniform(-1e3, 1e3, size=(n, d)).astype(np.float32)
    u = rng.rand(n, d)
    x = np.where(u < 1 / 3, sub, np.where(u < 1 / 3 + 0.1, 0.0, big)).astype(np.float32)
    tiny = np.where(rng.rand(n, d) < 0.2, 0.0, sub).astype(np.float32)
    x[np.arange(n) % 3 == 0] = tiny[np.arange(n) % 3 == 0]
    if rows:
        x = x.astype(np.float16).astype(np.float32)
        h = x.astype(np.float16).view(np.uint16)
        assert (((h & 0x7C00) == 0) & ((h & 0x03FF) != 0)).mean() > 1 / 3  # subnormal halves
    return x


def csr_of_index(idx):
    """(n, n_layers, starting vertex, offsets uint64[n_layers][n + 1], neighbours uint32[]) as graph_from_index"""
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
    return n, n_layers, hdr["starting_vertex"], off, np.concatenate(nbs).astype(np.uint32)


class _Case:
    def __init__(self, L, oracle, tmp, name, base, q):
        import torch
        self.L, self.oracle, self.base, self.q = L, oracle, base, q
        self.n, self.d = base.shape
        halves = base.astype(np.float16)
        assert np.array_equal(halves.astype(np.float32).view(np.uint32), base.view(np.uint32))  # the rows ARE halves
        self.idx = H.build_index_cpu(tmp, base, name=name)
        n, n_layers, sv, off, nb = csr_of_index(self.idx)
        assert n == self.n
        self.n_layers = n_layers
        self.h32, self.h16 = C.c_void_p(), C.c_void_p()
        rc = L.expann_graph_create(self.d, 0, base.ctypes.data, n, n_layers, sv, off.ctypes.data, nb.ctypes.data,
                                   C.byref(self.h32))
        assert rc == 0, L.expann_graph_last_error(None)
        rc = L.expann_graph_create_f16(self.d, 0, halves.ctypes.data, n, n_layers, sv, off.ctypes.data, nb.ctypes.data,
                                       C.byref(self.h16))
        assert rc == 0, L.expann_graph_last_error(None)
        self.og = oracle.Graph(self.idx)
        self.tq = torch.from_numpy(q).cuda()
        torch.cuda.synchronize()
        self._host, self._oracle = {}, {}

    def host(self, which, mode, ef):
        """expann_graph_search_mode on the fp32 ("h32") or binary16 ("h16") handle, unfiltered, default options; once"""
        key = (which, mode, ef)
        if key not in self._host:
            self._host[key] = _host(self.L, getattr(self, which), self.q, mode, ef)
        return self._host[key]

    def oracle_walk(self, mode, ef):
        key = (mode, ef)
        if key not in self._oracle:
            self._oracle[key] = self.og.query_k(self.q, K, ef, bool(mode))
        return self._oracle[key]


class _World:
    def __init__(self, tmp, oracle):
        from expann_amd import _lib
        self.tmp, self.oracle, self.L, self._cases = tmp, oracle, _lib.load(), {}

    def case(self, name):
        if name not in self._cases:
            kind, d = name.split("_")
            d = int(d)
            rng = np.random.RandomState(1600 + d + len(kind))
            n = 1000 if d == 1040 else H.N_ROWS
            if kind == "sift":  # integers in [0, 255]: exact in binary16, and the uint8 cast means something
                base, q = H.sift_like(rng, n, d), H.sift_like(rng, M_Q, d, frac=True)
            elif kind == "gauss":
                base, q = _gauss_f16(rng, n, d), rng.standard_normal((M_Q, d)).astype(np.float32)
            else:
                base, q = _mixed(rng, n, d), _mixed(rng, M_Q, d, rows=False)
            self._cases[name] = _Case(self.L, self.oracle, self.tmp, name, base, q)
        return self._cases[name]

    def close(self):
        for c in self._cases.values():
            self.L.expann_graph_destroy(c.h32)
            self.L.expann_graph_destroy(c.h16)


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    w = _World(tmp_path_factory.mktemp("graph_f16"), oracle)
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


def _host(L, h, q, mode, ef):
    from graph_ranged_helpers import search_mode
    rc, ids, dists, dc = search_mode(L, h, q, K, ef, mode)
    assert rc == 0, L.expann_graph_last_error(h)
    return ids, dists, dc


def _device(c, h, mode, ef, st):
    """expann_graph_search_device + expann_graph_sync; outputs pre-filled with a pattern no search writes"""
    import torch
    ids = torch.full((M_Q, K), -2, dtype=torch.int64, device="cuda")
    dists = torch.full((M_Q, K), -1.0, dtype=torch.float32, device="cuda")
    dc = torch.full((M_Q,), -3, dtype=torch.int32, device="cuda")
    st.wait_stream(torch.cuda.current_stream())
    rc = c.L.expann_graph_search_device(h, c.tq.data_ptr(), M_Q, K, ef, mode, ids.data_ptr(), dists.data_ptr(),
                                        dc.data_ptr(), st.cuda_stream)
    assert rc == 0, c.L.expann_graph_last_error(h)
    assert c.L.expann_graph_sync(h) == 0, c.L.expann_graph_last_error(h)
    return ids.cpu().numpy().view(np.uint64), dists.cpu().numpy(), dc.cpu().numpy().view(np.uint32)


def _same(got, exp, what, m=None):
    """ids, distance bits and distcomps, exactly"""
    m = got[0].shape[0] if m is None else m
    assert np.array_equal(got[0][:m], exp[0][:m]), what
    assert np.array_equal(got[1][:m].view(np.uint32), exp[1][:m].view(np.uint32)), what
    assert np.array_equal(np.asarray(got[2][:m], np.uint64), np.asarray(exp[2][:m], np.uint64)), what


# d = 128: the compiled instances (mode 0) and the run-time-dim byte walks; 144: 9 dims per lane, only the partial chunk
# of the run-time-dim loop; 192: run-time dim with byte copies built from halves; 1040: 65 dims per lane, four full
# chunks and a partial one
@pytest.mark.parametrize("name,mode", [("sift_128", 0), ("sift_128", 1), ("sift_128", 2), ("gauss_144", 0),
                                       ("sift_192", 0), ("sift_192", 1), ("sift_192", 2), ("gauss_1040", 0),
                                       ("mixed_128", 0)])
def test_f16_handle_equals_f32_handle_and_the_oracle(world, name, mode):
    c = world.case(name)
    assert c.n_layers >= 2  # the descent runs
    for ef in EFS:
        f32, f16 = c.host("h32", mode, ef), c.host("h16", mode, ef)
        _same(f16, f32, (name, mode, ef, "f16 handle against f32 handle"))
        assert (f32[0] != H.PAD).all()
        if mode in (0, 1):
            exp = c.oracle_walk(mode, ef)
            _same(f32, exp, (name, mode, ef, "f32 handle against the oracle"))
            _same(f16, exp, (name, mode, ef, "f16 handle against the oracle"))
        else:  # the restatement, on the first queries
            g = H.IndexGraph(c.idx)
            Df = H.dist_f32_matrix(c.oracle, c.base, c.q[:M_WALK])
            Db = H.bottom_matrix(c.oracle, c.base, c.q[:M_WALK], 2, Df)
            exp = H.walk(g, Df, Db, None, K, ef, 2)
            _same(f16, exp, (name, mode, ef, "f16 handle against the restatement"), m=M_WALK)


def test_mixed_case_is_decided_by_subnormals(world):
    """the case means something: queries that are all subnormal find all-subnormal rows at distances far below the
    smallest normal half squared, and flushing the rows' subnormals would change those distances"""
    c = world.case("mixed_128")
    ids, dists, _ = c.host("h16", 0, 40)
    tiny_q = np.arange(M_Q) % 3 == 0
    assert (dists[tiny_q] < 128 * 6.2e-5 ** 2 * 4).all() and (dists[tiny_q] > 0).all()
    assert (ids[tiny_q] % 3 == 0).all()
    flushed = (c.q[tiny_q][:, None, :] ** 2).sum(-1)  # the distance to a row of zeros
    assert not np.array_equal(np.broadcast_to(flushed, dists[tiny_q].shape).astype(np.float32), dists[tiny_q])


@pytest.mark.parametrize("name", ["sift_128", "sift_192"])
def test_ranged_params_are_the_f32_handles_bits(world, name):
    c = world.case(name)
    got = []
    for h in (c.h32, c.h16):
        s, o = C.c_float(), C.c_float()
        assert c.L.expann_graph_ranged_params(h, C.byref(s), C.byref(o)) == 0, c.L.expann_graph_last_error(h)
        got.append((np.float32(s.value).view(np.uint32), np.float32(o.value).view(np.uint32)))
    assert got[0] == got[1]
    from graph_ranged_helpers import oracle_ranged_q8
    scale, offset, _ = oracle_ranged_q8(c.oracle, c.base)
    assert got[1] == (scale.view(np.uint32), offset.view(np.uint32))


@pytest.mark.parametrize("name", ["sift_128", "gauss_144"])
def test_row_filter_f16_equals_f32(world, name):
    """`ones`, `every_second`, `random_10` walk ("filter_flat_rows" = 1); `block` (300 allowed rows) is scanned"""
    c = world.case(name)
    L = c.L
    ends = np.zeros(1, np.int64)
    filters = H.make_filters(c.n, ends, 0)
    try:
        for fname, flat_rows in (("ones", 1), ("every_second", 1), ("random_10", 1), ("block", 0)):
            allow, words = filters[fname]
            got = {}
            for which in ("h32", "h16"):
                h = getattr(c, which)
                assert L.expann_graph_set_option(h, b"filter_flat_rows", flat_rows) == 0
                assert L.expann_graph_set_row_filter(h, words.ctypes.data, words.size) == 0, L.expann_graph_last_error(h)
                flat = _stat(L, h, "flat_searches")
                got[which] = [_host(L, h, c.q, 0, ef) for ef in EFS]
                assert _stat(L, h, "flat_searches") - flat == (len(EFS) if fname == "block" else 0), (fname, which)
            for ef, a, b in zip(EFS, got["h16"], got["h32"]):
                _same(a, b, (name, fname, ef))
                kept = a[0][a[0] != H.PAD].astype(np.int64)
                assert allow[kept].all(), (name, fname, ef)
                if fname == "ones":
                    _same(a, c.host("h16", 0, ef), (name, "ones against no filter", ef))
                if fname == "block":
                    assert (a[2] == 300).all()
    finally:
        for h in (c.h32, c.h16):
            assert L.expann_graph_clear_row_filter(h) == 0
            assert L.expann_graph_set_option(h, b"filter_flat_rows", 0) == 0


def test_redo_launch_f16_equals_f32(world, stream):
    """"cand_capacity" = 8: the first launch overflows for some queries, the redo launch walks them again"""
    c = world.case("sift_128")
    L = c.L
    try:
        got = {}
        for which in ("h32", "h16"):
            h = getattr(c, which)
            assert L.expann_graph_set_option(h, b"cand_capacity", 8) == 0
            got[which] = _device(c, h, 0, 40, stream)
            assert _stat(L, h, "redo_queries") > 0, which
            got[which + "_redo"] = _stat(L, h, "redo_queries")
        assert got["h16_redo"] == got["h32_redo"]
        _same(got["h16"], got["h32"], "redo, f16 against f32")
        _same(got["h16"], c.host("h16", 0, 40), "redo against the default capacity")
    finally:
        for h in (c.h32, c.h16):
            assert L.expann_graph_set_option(h, b"cand_capacity", 0) == 0


@pytest.mark.parametrize("mode", [0, 2])
def test_device_entry_equals_host_entry(world, stream, mode):
    c = world.case("sift_128")
    for ef in EFS:
        _same(_device(c, c.h16, mode, ef, stream), c.host("h16", mode, ef), (mode, ef))


def test_vector_bytes(world):
    c = world.case("gauss_144")
    assert _stat(c.L, c.h16, "vector_bytes") == c.n * c.d * 2
    assert _stat(c.L, c.h32, "vector_bytes") == c.n * c.d * 4


# ---- the engine ------------------------------------------------------------------------------------
def test_engine_rows_f16_equals_a_plain_engine_over_its_file(tmp_path):
    from expann_amd import AntitopoEngine
    from graph_helpers import read_index_edges
    rng = np.random.RandomState(1616)
    base = rng.standard_normal((3000, 128)).astype(np.float32)
    q = rng.standard_normal((M_Q, 128)).astype(np.float32)
    eng = AntitopoEngine(16, 80, 1, 0, False, dim=128, rows="f16")
    eng.store_many_vectors(base[:2000], False)
    eng.store_many_vectors_batched(base[2000:], False)  # (2000 rows are stored: these go through the batched builder)
    eng.build()
    assert eng.param_list()["rows"] == "f16"
    idx = str(tmp_path / "f16_engine.index")
    eng.save_index(idx)
    plain = AntitopoEngine(16, 80, 1, 0, False, dim=128)
    plain.load_index(idx)
    for ef in EFS:
        eng.set_ef_search(ef)
        plain.set_ef_search(ef)
        a, b = eng.query_many(q, K), plain.query_many(q, K)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), ef
    # the file holds the rounded rows, and loads back into an engine that keeps halves
    from oracle_ctypes import Graph
    og = Graph(idx)
    assert np.array_equal(og.vectors().view(np.uint32), base.astype(np.float16).astype(np.float32).view(np.uint32))
    again = AntitopoEngine(16, 80, 1, 0, False, dim=128, rows="f16")
    again.load_index(idx)
    again.set_ef_search(40)
    c = again.query_many(q, K)
    assert np.array_equal(c[0], a[0]) and np.array_equal(c[1].view(np.uint32), a[1].view(np.uint32))
    assert read_index_edges(idx)[0]["n"] == 3000
    for e in (eng, plain, again):
        e.close()


def test_antitopo_rows_f16_c_abi(tmp_path, oracle):
    """expann_antitopo_set_rows_f16 and the store / save / load rules through the C ABI (n = 500, d = 64, serial)"""
    from expann_amd import _lib
    L = _lib.load()
    n, d = 500, 64
    rng = np.random.RandomState(64)
    base = rng.standard_normal((n, d)).astype(np.float32)
    e = C.c_void_p()
    assert L.expann_antitopo_create(d, 0, 16, 80, 1, 0, 0, C.byref(e)) == 0
    assert L.expann_antitopo_set_rows_f16(e, 1) == 0
    for poison in (np.nan, 70000.0):  # refused before any row of the call is inserted
        bad = base[:3].copy()
        bad[2, 5] = poison
        assert L.expann_antitopo_store(e, bad.ctypes.data, 3) == INVALID_ARG
        assert L.expann_antitopo_store_batched(e, bad.ctypes.data, 3, 0) == INVALID_ARG
        assert L.expann_antitopo_size(e) == 0
    assert L.expann_antitopo_store(e, base.ctypes.data, n) == 0
    assert L.expann_antitopo_size(e) == n
    assert L.expann_antitopo_set_rows_f16(e, 0) == INVALID_ARG  # the engine holds rows
    assert L.expann_antitopo_set_rows_f16(e, 1) == INVALID_ARG
    idx = str(tmp_path / "c_abi_f16.index")
    assert L.expann_antitopo_build(e) == 0, L.expann_antitopo_last_error(e)
    assert L.expann_antitopo_save(e, idx.encode()) == 0
    rounded = base.astype(np.float16).astype(np.float32)
    og = oracle.Graph(idx)
    assert np.array_equal(og.vectors().view(np.uint32), rounded.view(np.uint32))
    # the engine answers what the oracle's walk of its file answers
    q = rng.standard_normal((50, d)).astype(np.float32)
    ids, dists = np.zeros((50, K), np.uint64), np.zeros((50, K), np.float32)
    assert L.expann_antitopo_set_ef_search(e, 40) == 0
    assert L.expann_antitopo_query(e, q.ctypes.data, 50, K, ids.ctypes.data, dists.ctypes.data) == 0
    oids, od, _ = og.query_k(q, K, 40, False)
    assert np.array_equal(ids, oids) and np.array_equal(dists.view(np.uint32), od.view(np.uint32))
    L.expann_antitopo_destroy(e)
    # rows that are not binary16 values: an fp32 engine's file is refused by an engine that keeps halves
    plain_idx = H.build_index_cpu(tmp_path, base[:100], name="plain")
    e2 = C.c_void_p()
    assert L.expann_antitopo_create(d, 0, 16, 80, 1, 0, 0, C.byref(e2)) == 0
    assert L.expann_antitopo_set_rows_f16(e2, 1) == 0
    assert L.expann_antitopo_load(e2, plain_idx.encode()) == INVALID_ARG
    assert b"binary16" in L.expann_antitopo_last_error(e2)
    assert L.expann_antitopo_query(e2, q.ctypes.data, 50, K, ids.ctypes.data, dists.ctypes.data) != 0  # nothing uploaded
    L.expann_antitopo_destroy(e2)
    e3 = C.c_void_p()
    assert L.expann_antitopo_create(d, 0, 16, 80, 1, 0, 0, C.byref(e3)) == 0
    assert L.expann_antitopo_set_rows_f16(e3, 1) == 0
    assert L.expann_antitopo_load(e3, idx.encode()) == 0, L.expann_antitopo_last_error(e3)
    L.expann_antitopo_destroy(e3)
