"""CPU-side checks of the graph engine's range search (THE RANGE WALK RULE, include/expann_hip.h): the four new
symbols, their argtypes and the header text, the refusal of a NULL handle, the Python surface, and the properties of
the yardstick in tests/graph_range_helpers.py that need no device -- with a radius in range of nothing the restated
walk is H.walk_one; with r = +inf and R <= ef it is H.walk_one(k = R, ef); and its pre-drop form is its plain form."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import graph_filter_helpers as H
import graph_range_helpers as Rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M_CPU = 40  # queries the restatement's own properties are checked on


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    """the n = 3000 serial host build at d = 128 and the oracle's distances of 40 queries"""
    tmp = tmp_path_factory.mktemp("graph_range_cpu")
    rng = np.random.RandomState(1128)
    base = H.sift_like(rng, Rg.N_ROWS, 128)
    q = H.sift_like(rng, M_CPU, 128, frac=True)
    g = H.IndexGraph(H.build_index_cpu(tmp, base))
    assert g.n_layers >= 2
    return dict(g=g, Df=H.dist_f32_matrix(oracle, base, q))


def test_new_symbols_and_signatures(lib):
    from expann_amd import _lib
    vp, sz = C.c_void_p, C.c_size_t
    want = {"expann_graph_range_search": [vp, vp, vp, sz, sz, sz, vp, vp, vp, vp],
            "expann_graph_range_search_device": [vp, vp, vp, sz, sz, sz, vp, vp, vp, vp, vp],
            "expann_antitopo_range_query": [vp, vp, vp, sz, sz, vp, vp, vp],
            "expann_antitopo_range_query_device": [vp, vp, vp, sz, sz, vp, vp, vp, vp]}
    for name, argtypes in want.items():
        assert name in _lib.ABI_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
    raw = open(os.path.join(ROOT, "include", "expann_hip.h")).read()
    text = " ".join(re.sub(r"/\*.*?\*/", " ", raw, flags=re.S).split())
    for decl in (
            "int expann_graph_range_search(expann_graph* g, const float* queries, const float* radii, size_t m, "
            "size_t max_results, size_t ef_search, uint64_t* ids, float* dists, uint32_t* counts, uint32_t* distcomps);",
            "int expann_graph_range_search_device(expann_graph* g, const float* d_queries, const float* d_radii, size_t m, "
            "size_t max_results, size_t ef_search, uint64_t* d_ids, float* d_dists, uint32_t* d_counts, "
            "uint32_t* d_distcomps, void* stream);",
            "int expann_antitopo_range_query(expann_antitopo* e, const float* queries, const float* radii, size_t m, "
            "size_t max_results, uint64_t* ids, float* dists, uint32_t* counts);",
            "int expann_antitopo_range_query_device(expann_antitopo* e, const float* d_queries, const float* d_radii, "
            "size_t m, size_t max_results, uint64_t* d_ids, float* d_dists, uint32_t* d_counts, void* stream);",
            "#define EXPANN_ABI_VERSION 2"):
        assert decl in text, decl
    assert lib.expann_abi_version() == 2
    # the rule is stated, and the brute-force range search no longer lists the graph engine as not offered
    flat = " ".join(raw.replace("*", " ").split())
    assert "THE RANGE WALK RULE" in raw
    for phrase in ("cap = max(ef, R)", "(cur.d > r || nearest.size() >= cap)", "(dn <= r && nearest.size() < cap)",
                   "(nearest.top().d > r || nearest.size() > cap)", "full0 && !(dn < worst0) && !(dn <= r && n0 < cap)",
                   "\"range_searches\""):
        assert phrase in flat, phrase
    assert "on the sharded handles, in the graph engine" not in flat


def test_a_null_handle_is_refused_before_the_device(lib):
    from expann_amd import _lib
    f = (C.c_float * 16)()
    r = (C.c_float * 1)(1.0)
    ids = (C.c_uint64 * 4)()
    cnt = (C.c_uint32 * 1)(7)
    INV = _lib.ERR_INVALID_ARG
    assert lib.expann_graph_range_search(None, f, r, 1, 4, 10, ids, None, cnt, None) == INV
    assert lib.expann_graph_range_search(None, f, r, 0, 4, 10, ids, None, cnt, None) == INV  # (before m == 0)
    assert lib.expann_graph_range_search_device(None, f, r, 1, 4, 10, ids, None, cnt, None, None) == INV
    assert lib.expann_antitopo_range_query(None, f, r, 1, 4, ids, None, cnt) == INV
    assert lib.expann_antitopo_range_query_device(None, f, r, 1, 4, ids, None, cnt, None) == INV
    out = C.c_uint64(7)
    assert lib.expann_graph_get_stat(None, b"range_searches", C.byref(out)) == INV
    assert cnt[0] == 7 and out.value == 7


def test_python_surface():
    from expann_amd import AntitopoEngine, _lib
    for name in ("range_search", "range_search_device"):
        assert callable(getattr(AntitopoEngine, name))
    eng = AntitopoEngine(16, 80, 1, 0, False)  # (no dim yet: nothing is opened, no device is asked for)
    for call in (lambda: eng.range_search(np.zeros((1, 16), np.float32), 1.0, 4),
                 lambda: eng.range_search_device(8, 8, 1, 4, 8, 0, 8)):
        with pytest.raises(_lib.ExpannError) as ei:
            call()
        assert ei.value.code == _lib.ERR_NOT_BUILT


def _plain(g, Df, k, ef):
    """H.walk_one over every query: (ids, dists, distcomps) as range_walk pads them"""
    ids, dists, dc, _ = H.walk(g, Df, Df, None, k, ef, 0)
    return ids, dists, dc.astype(np.uint32)


@pytest.mark.parametrize("ef,R", Rg.EF_R)
@pytest.mark.parametrize("r", [-1.0, float("nan")])
def test_a_radius_in_range_of_nothing_gives_the_plain_walk(world, ef, R, r):
    """r < 0 or NaN, at any R: the distcomps of walk_one at that ef, counts 0, padding"""
    g, Df = world["g"], world["Df"]
    ids, dists, counts, dc, _, peak_n = Rg.range_walk(g, Df, np.full(M_CPU, r, np.float32), R, ef)
    assert np.array_equal(dc, _plain(g, Df, 1, ef)[2])
    assert not counts.any() and (ids == H.PAD).all() and np.isinf(dists).all() and peak_n.max() <= ef + 1


@pytest.mark.parametrize("ef,R", [(10, 8), (60, 16), (60, 60)])
def test_an_infinite_radius_with_R_up_to_ef_gives_the_plain_walk(world, ef, R):
    """r = +inf, R <= ef: walk_one(k = R, ef) bit for bit; counts = every vertex the bottom layer scored"""
    g, Df = world["g"], world["Df"]
    ids, dists, counts, dc, _, _ = Rg.range_walk(g, Df, np.full(M_CPU, np.inf, np.float32), R, ef)
    pi, pd, pdc = _plain(g, Df, R, ef)
    assert np.array_equal(ids, pi) and np.array_equal(dists.view(np.uint32), pd.view(np.uint32))
    assert np.array_equal(dc, pdc)
    descent = np.array([H._descend(g, Df[i])[1] for i in range(M_CPU)], np.uint32)
    assert np.array_equal(counts, dc - descent)


@pytest.mark.parametrize("ef,R", [(10, 8), (60, 16)])
def test_with_R_up_to_ef_a_finite_radius_only_cuts_the_plain_walk(world, ef, R):
    g, Df = world["g"], world["Df"]
    radii = Rg.radii_at_rank(Df, 5)
    ids, dists, counts, dc, _, _ = Rg.range_walk(g, Df, radii, R, ef)
    pi, pd, pdc = _plain(g, Df, R, ef)
    cut = pd <= radii[:, None]
    assert np.array_equal(dc, pdc) and np.array_equal(ids, np.where(cut, pi, H.PAD))
    assert np.array_equal(dists.view(np.uint32), np.where(cut, pd, np.float32(np.inf)).view(np.uint32))


@pytest.mark.parametrize("ef,R", Rg.EF_R)
def test_the_pre_drop_changes_nothing(world, ef, R):
    """the kernel's pre-drop against the rule without it: ids, distance bits, counts, distcomps and both peaks"""
    g, Df = world["g"], world["Df"]
    grew = False
    for rank in Rg.RANKS:
        radii = Rg.radii_at_rank(Df, rank)
        a = Rg.range_walk(g, Df, radii, R, ef, predrop=False)
        b = Rg.range_walk(g, Df, radii, R, ef, predrop=True)
        assert Rg.same(a, b) and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]), rank
        true = (Df <= radii[:, None]).sum(1)
        assert (a[2] <= true).all() and (a[2] >= 1).sum() >= M_CPU // 2, rank
        # an in-range vertex is refused or popped only once `nearest` holds cap >= R in-range entries
        assert np.array_equal((a[0] != H.PAD).sum(1), np.minimum(a[2], R)), rank
        grew = grew or a[5].max() > ef + 1
    assert grew == (R > ef)  # `nearest` passes ef exactly where cap does
