"""CPU-side checks of the graph engine's row filter.  The yardstick of tests/test_gpu_graph_filter.py is the Python
restatement of THE FILTER RULE in tests/graph_filter_helpers.py; it is pinned here before anything is compared
with it: its heap functions against the image's std::priority_queue (tests/golden/heap_ref.json), its fp32
distances against oracle.l2_f32, and -- with every bit set -- the whole walk against oracle.Graph.query_k in ids,
distance bits and distcomps.  Then the properties of a filtered walk that need no device, and the argument errors
of the new entry points that are defined before the device is touched."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import graph_filter_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EFS = (10, 40)


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


class _World:
    """one serial host build per dim (n = 3000, M = 16, ef_construction = 80), its index file, the oracle's graph of
    it, and the distance matrices of the 300 queries, each made once"""

    def __init__(self, tmp, oracle):
        self.tmp, self.oracle, self._dims = tmp, oracle, {}

    def dim(self, d):
        if d not in self._dims:
            rng = np.random.RandomState(1000 + d)
            base = H.sift_like(rng, H.N_ROWS, d)
            q = H.sift_like(rng, H.M_ALL, d, frac=True)
            idx = H.build_index_cpu(self.tmp, base)
            g = H.IndexGraph(idx)
            assert g.n_layers >= 2  # several layers: the descent runs
            og = self.oracle.Graph(idx)
            assert (og.n, og.dim) == base.shape
            Df = H.dist_f32_matrix(self.oracle, base, q)
            self._dims[d] = dict(base=base, q=q, g=g, og=og, Df=Df, Db={0: Df})
        return self._dims[d]

    def bottom(self, d, mode):
        w = self.dim(d)
        if mode not in w["Db"]:
            w["Db"][mode] = H.bottom_matrix(self.oracle, w["base"], w["q"], mode, w["Df"])
        return w["Db"][mode]


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    return _World(tmp_path_factory.mktemp("graph_filter_cpu"), oracle)


def test_heap_functions_replay_the_golden_traces():
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "heap_ref.json")))["cases"]
    assert len(cases) >= 20
    for c in cases:
        states, drain = H.heap_trace(c["max_heap"], c["init"], c["ops"])
        assert states == [tuple(s) for s in c["states"]], c["name"]
        assert drain == [tuple(x) for x in c["drain"]], c["name"]


def test_distance_matrices_are_the_oracles(world, oracle):
    w = world.dim(128)
    rng = np.random.RandomState(5)
    for i, v in zip(rng.randint(0, H.M_ALL, 200), rng.randint(0, H.N_ROWS, 200)):
        assert w["Df"][i, v].view(np.uint32) == oracle.l2_f32(w["q"][i], w["base"][v]).view(np.uint32)
    # the byte distances against the plain definition
    Db = world.bottom(128, 1)
    q8, r8 = np.trunc(w["q"]).astype(np.uint8), np.trunc(w["base"]).astype(np.uint8)
    assert not np.array_equal(q8.astype(np.float32), w["q"])  # the cast truncates something
    for i, v in zip(rng.randint(0, H.M_ALL, 50), rng.randint(0, H.N_ROWS, 50)):
        assert Db[i, v] == np.float32(((q8[i].astype(np.int64) - r8[v].astype(np.int64)) ** 2).sum())


@pytest.mark.parametrize("d,mode", [(128, 0), (128, 1), (48, 0)])
def test_all_ones_restatement_is_the_oracles_walk(world, d, mode):
    w = world.dim(d)
    Db = world.bottom(d, mode)
    allow = np.ones(H.N_ROWS, bool)
    for ef in EFS:
        oids, od, odc = w["og"].query_k(w["q"], H.K, ef, bool(mode))
        for a in (None, allow):  # no filter, and a filter with every bit set
            ids, dists, dc, _ = H.walk(w["g"], w["Df"], Db, a, H.K, ef, mode)
            assert np.array_equal(ids, oids), (ef, a is None)
            assert np.array_equal(dists.view(np.uint32), od.view(np.uint32)), (ef, a is None)
            assert np.array_equal(dc, odc), (ef, a is None)


def test_filtered_walks_keep_only_allowed_rows(world):
    """every case of the GPU test: only allowed ids, exactly min(k, allowed reachable) of them, ascending, with the
    oracle's distances; the peak candidates sizes the redo test uses"""
    w = world.dim(128)
    g, Df, m = w["g"], w["Df"][:H.M_FILTER], H.M_FILTER
    ends = H.descent_ends(g, Df)
    filters = H.make_filters(H.N_ROWS, ends, g.sv)
    assert set(filters) == set(H.FILTER_NAMES)
    peaks = {}
    for name, (allow, words) in filters.items():
        assert words.size == (H.N_ROWS + 31) // 32
        ids, dists, dc, peak = H.walk(g, Df, Df, allow, H.K, 40, 0)
        peaks[name] = peak
        got = ids != H.PAD
        assert allow[ids[got].astype(np.int64)].all(), name
        for i in range(m):
            want = min(H.K, H.reachable_allowed(g, allow, int(ends[i])))
            assert got[i].sum() == want and got[i, :want].all(), (name, i)
            assert (np.diff(dists[i, :want]) >= 0).all(), (name, i)
            assert np.array_equal(dists[i, :want], Df[i, ids[i, :want].astype(np.int64)]), (name, i)
    assert not filters["no_entry"][0][ends].any() and not filters["no_entry"][0][g.sv]
    assert (filters["last_word_set"][1][-1] == 0xFFFFFFFF) and H.N_ROWS % 32 != 0
    # sparser filters walk further: the frontier the candidates heap has to hold grows
    assert peaks["random_10"].min() > peaks["ones"].max()
    # the redo test's capacity -- the largest power of two below the 10 % filter's peak at ef = 10 -- splits the queries
    peak10 = H.walk(g, Df, Df, filters["random_10"][0], H.K, 10, 0)[3]
    cap = 1 << (int(peak10.max() - 1).bit_length() - 1)
    assert cap < peak10.max() and 0 < int((peak10 > cap).sum()) < m, (cap, sorted(peak10))


def test_new_symbols_and_signatures(lib):
    from expann_amd import _lib
    vp, sz = C.c_void_p, C.c_size_t
    want = {"expann_graph_set_row_filter": [vp, vp, sz],
            "expann_graph_set_row_filter_device": [vp, vp, sz, vp],
            "expann_graph_clear_row_filter": [vp],
            "expann_antitopo_set_row_filter": [vp, vp, sz],
            "expann_antitopo_set_row_filter_device": [vp, vp, sz, vp]}
    for name, argtypes in want.items():
        assert name in _lib.ABI_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "expann_hip.h")).read(), flags=re.S)
    text = " ".join(text.split())
    assert "int expann_graph_set_row_filter(expann_graph* g, const uint32_t* allow_bits, size_t n_words);" in text
    assert ("int expann_graph_set_row_filter_device(expann_graph* g, const uint32_t* d_allow_bits, size_t n_words, "
            "void* stream);") in text
    assert "int expann_graph_clear_row_filter(expann_graph* g);" in text
    assert ("int expann_antitopo_set_row_filter(expann_antitopo* e, const uint32_t* allow_bits_or_NULL, "
            "size_t n_words);") in text
    assert "#define EXPANN_ABI_VERSION 2" in text
    assert lib.expann_abi_version() == 2
    # the header no longer says the graph engine has no filter, and states the rule
    raw = open(os.path.join(ROOT, "include", "expann_hip.h")).read()
    assert "the graph engine are not offered" not in raw and "THE FILTER RULE" in raw


def test_null_arguments_are_refused_before_the_device(lib):
    from expann_amd import _lib
    words = (C.c_uint32 * 4)(1, 2, 3, 4)
    assert lib.expann_graph_set_row_filter(None, words, 4) == _lib.ERR_INVALID_ARG
    assert lib.expann_graph_set_row_filter(None, None, 0) == _lib.ERR_INVALID_ARG
    assert lib.expann_graph_set_row_filter_device(None, words, 4, None) == _lib.ERR_INVALID_ARG
    assert lib.expann_graph_clear_row_filter(None) == _lib.ERR_INVALID_ARG
    assert lib.expann_antitopo_set_row_filter(None, words, 4) == _lib.ERR_INVALID_ARG
    assert lib.expann_antitopo_set_row_filter(None, None, 0) == _lib.ERR_INVALID_ARG
    assert lib.expann_antitopo_set_row_filter_device(None, words, 4, None) == _lib.ERR_INVALID_ARG
    out = C.c_uint64(7)
    for name in (b"filter_active", b"filter_rows", b"flat_searches"):
        assert lib.expann_graph_get_stat(None, name, C.byref(out)) == _lib.ERR_INVALID_ARG
    assert out.value == 7
    assert lib.expann_graph_set_option(None, b"filter_flat_rows", 1) == _lib.ERR_INVALID_ARG


def test_python_surface():
    from expann_amd import AntitopoEngine, _lib
    assert callable(AntitopoEngine.set_row_filter) and callable(AntitopoEngine.set_row_filter_device)
    eng = AntitopoEngine(16, 80, 1, 0, False)  # (no dim yet: nothing is opened, no device is asked for)
    for call in (lambda: eng.set_row_filter(np.ones(4, bool)), lambda: eng.set_row_filter(None),
                 lambda: eng.set_row_filter_device(0, 1)):
        with pytest.raises(_lib.ExpannError) as ei:
            call()
        assert ei.value.code == _lib.ERR_NOT_BUILT
