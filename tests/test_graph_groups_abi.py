"""CPU-side checks of the graph engine's row groups: the new symbols, their argtypes and the header text, the
refusals that are defined before the device is touched, the Python surface, and the properties of the yardstick in
tests/graph_groups_helpers.py that need no device -- per query the grouped restatement is the bitmap restatement of
(labels == group), an ANY query is oracle.Graph.query_k, and a walked 7-row group returns 7 ids and 3 pads."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import graph_filter_helpers as H
import graph_groups_helpers as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    """the n = 3000 serial host build at d = 128, the oracle's graph of it, and the restatement over 48 queries"""
    tmp = tmp_path_factory.mktemp("graph_groups_cpu")
    rng = np.random.RandomState(1128)
    base = H.sift_like(rng, G.N_ROWS, 128)
    q = H.sift_like(rng, G.M, 128, frac=True)
    idx = H.build_index_cpu(tmp, base)
    g = H.IndexGraph(idx)
    assert g.n_layers >= 2
    Df = H.dist_f32_matrix(oracle, base, q)
    Db = {0: Df}

    def Db_of_mode(mode):
        if mode not in Db:
            Db[mode] = H.bottom_matrix(oracle, base, q, mode, Df)
        return Db[mode]
    labels, qg = G.make_labels(), G.query_groups()
    sizes = G.check_classes(labels, qg, H.descent_ends(g, Df))
    return dict(base=base, q=q, g=g, og=oracle.Graph(idx), Df=Df, Db=Db_of_mode, labels=labels, qg=qg, sizes=sizes,
                R=G.Restatement(g, Df, Db_of_mode))


def test_new_symbols_and_signatures(lib):
    from expann_amd import _lib
    vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
    want = {"expann_graph_set_row_groups": [vp, vp, sz],
            "expann_graph_set_row_groups_device": [vp, vp, sz, vp],
            "expann_graph_clear_row_groups": [vp],
            "expann_graph_search_grouped": [vp, vp, vp, sz, sz, sz, ci, vp, vp, vp],
            "expann_graph_search_grouped_device": [vp, vp, vp, sz, sz, sz, ci, vp, vp, vp, vp],
            "expann_antitopo_set_row_groups": [vp, vp, sz],
            "expann_antitopo_set_row_groups_device": [vp, vp, sz, vp],
            "expann_antitopo_query_grouped": [vp, vp, vp, sz, sz, vp, vp],
            "expann_antitopo_query_grouped_device": [vp, vp, vp, sz, sz, vp, vp, vp]}
    for name, argtypes in want.items():
        assert name in _lib.ABI_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
    assert _lib.GROUP_ANY == 0xFFFFFFFF == G.ANY
    raw = open(os.path.join(ROOT, "include", "expann_hip.h")).read()
    text = " ".join(re.sub(r"/\*.*?\*/", " ", raw, flags=re.S).split())
    for decl in (
            "#define EXPANN_GROUP_ANY 0xFFFFFFFFu",
            "int expann_graph_set_row_groups(expann_graph* g, const uint32_t* groups, size_t n);",
            "int expann_graph_set_row_groups_device(expann_graph* g, const uint32_t* d_groups, size_t n, void* stream);",
            "int expann_graph_clear_row_groups(expann_graph* g);",
            "int expann_graph_search_grouped(expann_graph* g, const float* queries, const uint32_t* query_groups, "
            "size_t m, size_t k, size_t ef_search, int mode, uint64_t* ids, float* dists, uint32_t* distcomps);",
            "int expann_graph_search_grouped_device(expann_graph* g, const float* d_queries, "
            "const uint32_t* d_query_groups, size_t m, size_t k, size_t ef_search, int mode, uint64_t* d_ids, "
            "float* d_dists, uint32_t* d_distcomps, void* stream);",
            "int expann_antitopo_set_row_groups(expann_antitopo* e, const uint32_t* groups_or_NULL, size_t n);",
            "int expann_antitopo_query_grouped(expann_antitopo* e, const float* queries, const uint32_t* query_groups, "
            "size_t m, size_t k, uint64_t* ids, float* dists);",
            "int expann_antitopo_query_grouped_device(expann_antitopo* e, const float* d_queries, "
            "const uint32_t* d_query_groups, size_t m, size_t k, uint64_t* d_ids, float* d_dists, void* stream);",
            "#define EXPANN_ABI_VERSION 2"):
        assert decl in text, decl
    assert lib.expann_abi_version() == 2
    # the rule, its three serve classes and what is still not offered
    assert "THE GROUP RULE" in raw and "THE FILTER RULE" in raw
    flat = " ".join(raw.replace("*", " ").split())
    for phrase in ("s_i == 0", "(scan)", "(walk)", "bitmap x groups", "Not offered: per-query filters"):
        assert (phrase in flat) == (phrase != "Not offered: per-query filters"), phrase


def test_null_arguments_are_refused_before_the_device(lib):
    from expann_amd import _lib
    arr = (C.c_uint32 * 4)(1, 2, 3, 4)
    f = (C.c_float * 4)()
    ids = (C.c_uint64 * 4)()
    INV = _lib.ERR_INVALID_ARG
    assert lib.expann_graph_set_row_groups(None, arr, 4) == INV
    assert lib.expann_graph_set_row_groups(None, None, 0) == INV
    assert lib.expann_graph_set_row_groups_device(None, arr, 4, None) == INV
    assert lib.expann_graph_clear_row_groups(None) == INV
    assert lib.expann_graph_search_grouped(None, f, arr, 1, 1, 1, 0, ids, f, None) == INV
    assert lib.expann_graph_search_grouped_device(None, f, arr, 1, 1, 1, 0, ids, f, None, None) == INV
    assert lib.expann_antitopo_set_row_groups(None, arr, 4) == INV
    assert lib.expann_antitopo_set_row_groups(None, None, 0) == INV
    assert lib.expann_antitopo_set_row_groups_device(None, arr, 4, None) == INV
    assert lib.expann_antitopo_query_grouped(None, f, arr, 1, 1, ids, f) == INV
    assert lib.expann_antitopo_query_grouped_device(None, f, arr, 1, 1, ids, f, None) == INV
    out = C.c_uint64(7)
    for name in (b"groups_active", b"group_count", b"group_walk_queries", b"group_scan_queries", b"group_pad_queries"):
        assert lib.expann_graph_get_stat(None, name, C.byref(out)) == INV
    assert out.value == 7


def test_python_surface():
    from expann_amd import AntitopoEngine, _lib
    for name in ("set_row_groups", "set_row_groups_device", "query_many", "query_many_device"):
        assert callable(getattr(AntitopoEngine, name))
    eng = AntitopoEngine(16, 80, 1, 0, False)  # (no dim yet: nothing is opened, no device is asked for)
    for call in (lambda: eng.set_row_groups(np.ones(4, np.uint32)), lambda: eng.set_row_groups(None),
                 lambda: eng.set_row_groups_device(0, 1),
                 lambda: eng.query_many(np.zeros((1, 16), np.float32), 1, groups=np.zeros(1, np.uint32)),
                 lambda: eng.query_many_device(0, 1, 1, 0, 0, groups_ptr=8)):
        with pytest.raises(_lib.ExpannError) as ei:
            call()
        assert ei.value.code == _lib.ERR_NOT_BUILT


def test_serve_restates_the_rule():
    assert G.serve(0, 10, 0) == G.PAD and G.serve(0, 10, 1) == G.PAD
    assert G.serve(1, 10, 1) == G.SCAN and G.serve(2, 10, 1) == G.WALK
    assert G.serve(400, 10, 400) == G.SCAN and G.serve(401, 10, 400) == G.WALK
    assert G.serve(128000, 10, 0) == G.SCAN and G.serve(128001, 10, 0) == G.WALK
    assert G.serve(2000, 1024, 0) == G.SCAN and G.serve(2000, 1025, 0) == G.WALK and G.serve(1025, 2000, 0) == G.WALK
    assert G.serve(1024, 2000, 0) == G.SCAN


@pytest.mark.parametrize("mode", [0, 1])
def test_grouped_restatement_is_the_bitmap_restatement_per_query(world, mode):
    """every query of the mixed batch, walked ("filter_flat_rows" = 1): H.walk under the bitmap (labels == group)"""
    w = world
    labels, qg, R = w["labels"], w["qg"], w["R"]
    for ef in G.EFS:
        ids, dists, dc, classes, _ = R.expected(labels, qg, G.K, ef, mode, 1)
        assert classes.count(G.PAD) == 6 and classes.count(G.SCAN) == 6  # the absent group; the 1-row group
        for X in set(G.QUERY_CYCLE) - {G.ANY, G.ABSENT, 9}:
            bi, bd, bdc, _ = H.walk(w["g"], w["Df"], w["Db"](mode), labels == np.uint32(X), G.K, ef, mode)
            rows = np.flatnonzero(qg == np.uint32(X))
            assert np.array_equal(ids[rows], bi[rows]), (ef, X)
            assert np.array_equal(dists[rows].view(np.uint32), bd[rows].view(np.uint32)), (ef, X)
            assert np.array_equal(dc[rows], bdc[rows]), (ef, X)
        # ANY is the oracle's unfiltered walk
        oi, od, odc = w["og"].query_k(w["q"], G.K, ef, bool(mode))
        rows = np.flatnonzero(qg == np.uint32(G.ANY))
        assert rows.size == 6
        assert np.array_equal(ids[rows], oi[rows]) and np.array_equal(dc[rows], odc[rows]), ef
        assert np.array_equal(dists[rows].view(np.uint32), od[rows].view(np.uint32)), ef
        # the 7-row group, walked: 7 ids of the group and 3 pads; the absent group: pads and no distcomps
        rows3 = np.flatnonzero(qg == 3)
        assert (ids[rows3, :7] != H.PAD).all() and (ids[rows3, 7:] == H.PAD).all() and np.isinf(dists[rows3, 7:]).all()
        assert (labels[ids[rows3, :7].astype(np.int64)] == 3).all()
        rows_abs = np.flatnonzero(qg == G.ABSENT)
        assert (ids[rows_abs] == H.PAD).all() and np.isinf(dists[rows_abs]).all() and (dc[rows_abs] == 0).all()


def test_scanned_queries_are_the_brute_force_over_the_group(world, oracle):
    """"filter_flat_rows" = 0: everything but ANY is scanned; the answer is oracle.brute_force over the group's rows"""
    w = world
    labels, qg = w["labels"], w["qg"]
    ids, dists, dc, classes, _ = w["R"].expected(labels, qg, G.K, 40, 0, 0)
    assert classes.count(G.SCAN) == 36 and classes.count(G.WALK) == 6 and classes.count(G.PAD) == 6
    for X in (5, 2, 1, G.TOP, 3, 9):
        rows = np.flatnonzero(labels == np.uint32(X))
        qi = np.flatnonzero(qg == np.uint32(X))
        kk = min(G.K, rows.size)
        bi, bd = oracle.brute_force(w["base"][rows], w["q"][qi], kk, oracle.METRIC_L2_F32, n_threads=4)
        assert np.array_equal(ids[qi, :kk], rows[bi.astype(np.int64)].astype(np.uint64)), X
        assert np.array_equal(dists[qi, :kk].view(np.uint32), bd.view(np.uint32)), X
        assert (ids[qi, kk:] == H.PAD).all() and (dc[qi] == rows.size).all(), X
    # the peak of a candidates heap never reaches the redo capacity: no walk of these tests can overflow for good
    peaks = w["R"].expected(labels, qg, G.K, 10, 0, 1)[4]
    assert 64 < max(peaks.values()) <= G.N_ROWS < 8192
