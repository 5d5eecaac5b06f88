"""expann_graph_append / expann_graph_remove at the handle, where their kernels chunk: the gather's
streaming, the task chunks, keep_cap at M0 / at a row's exact candidate count / at 1 024, graph_grow_upper, the
reopened top, the carried scan over more than 2^20 offsets, and the refusals that need a device.

Every case drives a handle from NumPy (tests/graph_handle_helpers.py): created from flatten() of a graph the oracle
built, adopted with the case's parameters.  After every device call the state read back is compared exactly with the
CPU reference -- a remove with the NumPy restatement of THE GRAPH REMOVE RULE (ids in order and length bits), an
append with oracle_graph_build_batched from the state before it by graph_build_helpers.compare_run's rule -- the walk
over 32 queries at ef 10 and 40 with a fresh handle created from flatten(read()): ids, distance bits, distcomps; and
the stats with the reference's numbers.  Every case first asserts, from the reference alone, that its input reaches
the path it is named after.  No tolerances."""
import ctypes as C

import numpy as np
import pytest

import graph_handle_helpers as hh
from graph_build_helpers import Params, compare_run

pytestmark = pytest.mark.gpu


def searches_match(h, st, q):
    """the handle's walk == the walk of a fresh handle created from flatten(st): ids, distance bits, distcomps"""
    with hh.Handle(st, adopt=False) as fresh:
        for ef in (10, 40):
            got, want = h.search(q, 10, ef), fresh.search(q, 10, ef)
            for a, b, what in zip(got, want, ("ids", "distance bits", "distcomps")):
                assert np.array_equal(a, b), (ef, what, np.flatnonzero((a != b).reshape(len(q), -1).any(axis=1))[:8])
            assert (got[0][:, 0] != hh.PAD).all()


def check_remove(h, ref, ids, keep_cap, p, q, only=None):
    """one expann_graph_remove against the restatement applied to `ref`, the state before.  Returns (the state read
    back, the restatement's dict)."""
    before = [h.stat(s) for s in ("remove_calls", "remove_rows", "remove_touched_rows", "remove_truncated_rows",
                                  "capacity_rows", "graph_reallocs")]
    _, want = hh.strided_remove(ref, ids, keep_cap, p, only=only)
    rc, done = h.remove(ids)
    assert (rc, done) == (0, len(np.unique(ids))), (rc, h.error())
    got = h.read()
    hh.assert_state_is(got, want)
    now = [h.stat(s) for s in ("remove_calls", "remove_rows", "remove_touched_rows", "remove_truncated_rows",
                               "capacity_rows", "graph_reallocs")]
    assert now == [before[0] + 1, before[1] + done, before[2] + want["touched"], before[3] + want["truncated"],
                   before[4], before[5]], (before, now, want["touched"], want["truncated"])
    assert (h.max_layer, h.sv) == (want["max_layer"], want["starting_vertex"])
    searches_match(h, got, q)
    return got, want


def check_append(h, ref, rows, levels, p, q, reallocs=0):
    """one expann_graph_append against the oracle's build from `ref`, the state before.  Returns the state read back
    (the order of the reverse edges in a row that was not re-pruned is the device's: the next reference starts here)."""
    levels = np.asarray(levels, np.uint8)
    ext = hh.extended(ref, rows, levels)
    ro = ext.oracle_build(ext.n, ref.n, p)
    before = [h.stat(s) for s in ("append_calls", "append_rows", "append_batches", "graph_reallocs")]
    rc, done = h.append(rows, levels)
    assert (rc, done) == (0, len(rows)), (rc, h.error())
    got = h.read()
    assert np.array_equal(got.levels, ext.levels) and np.array_equal(got.upper_idx, ext.upper_idx) and got.U == ext.U
    compare_run(got, ext, dict(max_layer=h.max_layer, starting_vertex=h.sv), ro, stat_ids=())
    n_batches = hh.batches(ext.levels, ext.n, ref.n, ref.max_layer)
    assert n_batches == int(ro["stats"][0])
    now = [h.stat(s) for s in ("append_calls", "append_rows", "append_batches", "graph_reallocs")]
    assert now == [before[0] + 1, before[1] + len(rows), before[2] + n_batches, before[3] + reallocs], (before, now)
    assert h.stat("append_edges") == hh.edge_count(ext) == hh.edge_count(got)
    searches_match(h, got, q)
    return got


@pytest.fixture(scope="module")
def streamed():
    """the streamed-gather input and its profile, made once"""
    st, ids, q = hh.streamed_case()
    prof = hh.pending_profile(hh.to_layers(st), hh.gone_mask(st.n, ids))
    return st, ids, q, prof


def test_streamed_gather(streamed):
    """800 rows, M0 = 64 full rows, 320 removed, cap 80: 475 layer-0 rows take 2 or more chunks, 22 take 3, in 475 a
    vertex is adopted in two chunks.  Full restatement.  Measured on an MI355X host: 0.8 s, 0.3 s of it the shared input."""
    st, ids, q, prof = streamed
    assert sum(1 for (v, l), x in prof.items() if l == 0 and x[0] >= 2) >= 20
    assert sum(1 for x in prof.values() if x[0] >= 3) >= 1
    assert sum(1 for x in prof.values() if x[2]) >= 5
    with hh.Handle(st, ef_construction=80) as h:
        _, want = check_remove(h, st, ids, 80, Params(80), q)
        assert want["truncated"] > 0


@pytest.mark.parametrize("which", ["cap_is_M0", "cap_is_a_rows_count", "cap_1024"])
def test_the_caps_edges(streamed, which):
    """The streamed input adopted with ef_construction = 16 (cap = M0 = 64 > ef_construction), = c, the distinct
    candidates of the median streamed row (one row holds exactly c and is not truncated, others hold more and are),
    and = 1 024 (cap == the chunk: nothing is truncated, 46 rows have more than 1 024 pending candidates).  c = 390 here:
    11 rows hold exactly 390 candidates, 235 hold more.  Full restatement in all three: a streamed row has at most 441
    distinct candidates, so the 1 024 case needs no sample.  Measured on an MI355X host: 0.4 s each."""
    st, ids, q, prof = streamed
    counts = sorted(x[1] for x in prof.values() if x[0] >= 2)
    c = counts[len(counts) // 2]
    efc = dict(cap_is_M0=16, cap_is_a_rows_count=c, cap_1024=1024)[which]
    cap = max(efc, st.M0)
    exact = sum(1 for x in prof.values() if x[0] >= 2 and x[1] == cap)
    more = sum(1 for x in prof.values() if x[0] >= 2 and x[1] > cap)
    if which == "cap_is_M0":
        assert cap == 64 > efc
    elif which == "cap_is_a_rows_count":
        assert 64 < c <= 1024 and exact >= 1 and more >= 1
    else:
        assert more == 0 and max(counts) < 1024 and sum(1 for x in prof.values() if x[3] > 1024) >= 1
    with hh.Handle(st, ef_construction=efc) as h:
        _, want = check_remove(h, st, ids, cap, Params(efc), q)
        assert want["truncated"] == sum(1 for x in prof.values() if x[1] > cap)
        assert which != "cap_1024" or want["truncated"] == 0


def test_task_chunks():
    """38 000 rows, d = 48 (the smallest dim the builder's exact tests use), M = 4, M0 = 8, ef 8, 9 500 removed: 18 765
    touched rows = 16 384 + 2 381, so the tasks go through gather + prune in two chunks over one list buffer.  Full
    restatement, one oracle distance call per candidate list: 3.2 s of CPU where it was written (a third chunk needs
    twice the rows and twice the time: left out).  Measured on an MI355X host: 2.1 s."""
    st, ids, q = hh.task_chunk_case()
    with hh.Handle(st, ef_construction=8) as h:
        _, want = check_remove(h, st, ids, 8, Params(8), q)
    assert want["touched"] > 16384 and want["touched"] % 16384 != 0


def test_upper_growth_by_chosen_levels():
    """600 rows, M = 8, ef 40, drawn levels (U = 73, top level 3: U_cap = 237, L_cap = 5).  400 rows of which 300 have
    level >= 1 (U_new = 373 > U_cap); three rows of level top + 4 = 7 first in their call (L_need = 7 > L_cap), the
    first becomes the starting vertex; a reserve and an append within it; an append past capacity_rows, which grows by
    half.  Measured on an MI355X host: 0.3 s."""
    st, rng, q = hh.drawn_case()
    p = Params(40)
    top = st.max_layer - 1
    U_cap, L_cap = st.U + st.U // 2 + 128, top + 2
    with hh.Handle(st, ef_construction=40) as h:
        assert h.stat("capacity_rows") == 600
        lv = np.zeros(400, np.uint8)
        lv[rng.choice(400, 300, replace=False)] = 1 + (rng.randint(0, 4, 300) == 0)
        assert st.U + int((lv >= 1).sum()) > U_cap and int(lv.max()) <= top
        cur = check_append(h, st, rng.standard_normal((400, 64)).astype(np.float32), lv, p, q, reallocs=1)
        assert h.stat("capacity_rows") == 1000
        lv = hh.draw_levels(rng, 30, 8)
        lv[[0, 7, 19]] = top + 4
        assert top + 4 > L_cap
        cur = check_append(h, cur, rng.standard_normal((30, 64)).astype(np.float32), lv, p, q, reallocs=1)
        assert (h.sv, h.max_layer) == (1000, top + 5)
        # (the first raises the top in a batch of its own; the other two join in one batch and do not see each other)
        assert [int(cur.degu[cur.urow(top + 4, v)]) for v in (1000, 1007, 1019)] == [2, 1, 1]
        assert h.stat("capacity_rows") == 1500
        assert h.reserve(2000) == 0 and h.stat("capacity_rows") == 2000
        searches_match(h, cur, q)
        held = h.stat("graph_reallocs")
        cur = check_append(h, cur, rng.standard_normal((200, 64)).astype(np.float32), hh.draw_levels(rng, 200, 8), p, q)
        assert (h.stat("graph_reallocs"), h.stat("capacity_rows")) == (held, 2000)
        cur = check_append(h, cur, rng.standard_normal((800, 64)).astype(np.float32), hh.draw_levels(rng, 800, 8), p, q,
                           reallocs=1)
        assert cur.n == 2030 and h.stat("capacity_rows") == 3000


def test_remove_the_top_then_reopen_it():
    """700 rows, M = 8, ef 40, drawn levels.  Every vertex of level >= 2 is removed (max_layer drops by 2 or more); 60
    rows are appended whose levels reopen those layers and one more; a tenth is removed again.  The append starts from
    the restated arrays: what the remove built aside holds zero degrees above the survivors.  Measured on an MI355X
    host: 0.3 s."""
    st, rng, q = hh.drawn_case(6004, 700)
    p = Params(40)
    top = st.max_layer - 1
    with hh.Handle(st, ef_construction=40) as h:
        ids = np.flatnonzero(st.levels >= 2)
        assert top >= 3 and len(ids) >= 3
        after, want = check_remove(h, st, ids, 40, p, q)
        assert want["max_layer"] == 2 <= st.max_layer - 2
        lv = hh.draw_levels(rng, 60, 8)
        lv[[3, 11, 40, 41]] = (top + 1, top, top + 1, 2)
        assert after.n + 60 > 700   # (the capacity stayed 700 through the remove: this append grows it)
        cur = check_append(h, after, rng.standard_normal((60, 64)).astype(np.float32), lv, p, q, reallocs=1)
        assert (h.max_layer, h.sv) == (top + 2, after.n + 3)
        assert int(cur.degu[cur.urow(top + 1, after.n + 3)]) == 1 and int(cur.degu[cur.urow(top, after.n + 11)]) >= 1
        check_remove(h, cur, hh.random_ids(rng, cur.n, cur.n // 10), 40, p, q)


def test_many_layers():
    """4 300 rows, M = 8, ef 40, drawn levels, then three rows of level 250: 251 x 4 304 = 1 080 304 offsets, 528 tiles
    (more than 2 x 256: append_scan_sums_kernel carries twice), not a multiple of 2 048; the first holds the
    other two, and they it, in 245 layers and more.  Then 430 rows and one of the three are removed: the touch and the compact kernel run
    over more than 10^6 entries.  Measured on an MI355X host: 1.1 s."""
    st, rng, q = hh.drawn_case(6002, 4300)
    p = Params(40)
    with hh.Handle(st, ef_construction=40) as h:
        entries = 251 * (st.n + 3 + 1)
        assert entries > 1048576 and entries % 2048 != 0 and (entries + 2047) // 2048 > 512
        cur = check_append(h, st, rng.standard_normal((3, 64)).astype(np.float32), [250, 250, 250], p, q, reallocs=1)
        assert (h.max_layer, h.sv) == (251, 4300)
        assert sum(int(cur.degu[cur.urow(l, 4300)]) == 2 and int(cur.degu[cur.urow(l, 4302)]) == 1 for l in range(1, 251)) >= 245
        ids = np.concatenate([hh.random_ids(rng, 4300, 430), [4301]]).astype(np.uint64)
        _, want = check_remove(h, cur, ids, 40, p, q)
        assert want["max_layer"] == 251 and 251 * 4303 > 10 ** 6


def _raw(st):
    return [a.copy() for a in (st.levels, st.upper_idx, st.ids0, st.d0.view(np.uint32), st.deg0, st.idsu,
                               st.du.view(np.uint32), st.degu)]


def test_the_two_upper_layouts():
    """600 rows, M = 8, ef 40, drawn levels (U = 73, no multiple of 64; top level >= 2).  The host's [layer][U] upper rows
    adopted into the handle's [L_cap][U_cap] = [top + 2][237] and read back: the eight arrays are the input.  Then 400
    rows, 300 of level 1 and the first of level top + 4, so that the upper arrays are laid out again in both dimensions:
    every upper row of an earlier vertex that the oracle's build left as it was is bit-equal to before, the whole row;
    and every degree of the raw [layers][U_stride] array that no vertex owns -- slots from U on, and the slots of the
    layers above the old top that the tall vertex did not take -- is zero."""
    st, rng, q = hh.drawn_case()
    p = Params(40)
    top = st.max_layer - 1
    U_cap, L_cap = st.U + st.U // 2 + 128, top + 2
    assert top >= 2 and st.U % 64 != 0 and st.L == top
    lv = np.zeros(400, np.uint8)
    lv[rng.choice(400, 300, replace=False)] = 1
    lv[0] = top + 4
    assert st.U + int((lv >= 1).sum()) > U_cap and top + 4 > L_cap
    rows = rng.standard_normal((400, 64)).astype(np.float32)
    ext = hh.extended(st, rows, lv)
    ext.oracle_build(ext.n, st.n, p)
    u32 = np.uint32
    same = [(l, v) for v in np.flatnonzero(st.levels >= 1) for l in range(1, int(st.levels[v]) + 1)
            if int(ext.degu[ext.urow(l, v)]) == int(st.degu[st.urow(l, v)]) and
            np.array_equal(ext.idsu[ext.urow(l, v), :st.degu[st.urow(l, v)]], st.idsu[st.urow(l, v), :st.degu[st.urow(l, v)]]) and
            np.array_equal(ext.du[ext.urow(l, v), :st.degu[st.urow(l, v)]].view(u32), st.du[st.urow(l, v), :st.degu[st.urow(l, v)]].view(u32))]
    assert len(same) >= 3 and {l for l, _ in same} >= {1, 2}
    with hh.Handle(st, ef_construction=40) as h:
        assert h.read_raw()[1] == U_cap
        before = h.read()
        assert all(np.array_equal(a, b) for a, b in zip(_raw(before), _raw(st)))
        after = check_append(h, before, rows, lv, p, q, reallocs=1)
        for l, v in same:
            a, b = after.urow(l, v), st.urow(l, v)
            assert after.degu[a] == st.degu[b] and np.array_equal(after.idsu[a], st.idsu[b]) and \
                np.array_equal(after.du[a].view(u32), st.du[b].view(u32)), (l, v)
        (levels, upper_idx, _, _, _, _, _, degu), ustride, L, U = h.read_raw()
        assert (U, L) == (st.U + int((lv >= 1).sum()), top + 4) and ustride > max(U, U_cap) and L > L_cap
        owned = np.zeros((L, ustride), bool)
        for l in range(1, L + 1):
            owned[l - 1, upper_idx[levels >= l]] = True
        assert (degu.reshape(L, ustride)[~owned] == 0).all()
        assert owned[top:].sum() == 4 and not owned[:, U:].any()


def test_refusals_at_the_handle():
    """600 rows.  Before adoption an append and a remove are EXPANN_ERR_NOT_BUILT; on the adopted handle an id >= n, a
    remove of every row, and an adoption with M0 + 1 ids in a row or an id >= n are EXPANN_ERR_INVALID_ARG; a binary16
    handle refuses adoption.  After each the state read back is the state before, bit for bit.  Measured on an MI355X
    host: 0.3 s."""
    from expann_amd import _lib
    st, rng, q = hh.drawn_case()
    one = rng.standard_normal((1, 64)).astype(np.float32)
    with hh.Handle(st, adopt=False) as h:
        want = h.search(q, 10, 40)
        assert h.append(one, [0]) == (_lib.ERR_NOT_BUILT, 0)
        assert h.remove([3]) == (_lib.ERR_NOT_BUILT, 0)
        shape = (C.c_size_t * 6)()
        assert h.L.expann_graph_build_state_shape(h.h, shape) == _lib.ERR_NOT_BUILT
        assert all(np.array_equal(a, b) for a, b in zip(h.search(q, 10, 40), want))
        assert h.adopt(st, 40) == 0
        before = _raw(h.read())

        def unchanged():
            now = _raw(h.read())
            assert all(np.array_equal(a, b) for a, b in zip(before, now))
            assert all(np.array_equal(a, b) for a, b in zip(h.search(q, 10, 40), want))
            assert (h.stat("remove_calls"), h.stat("append_calls")) == (0, 0)
        unchanged()
        for bad in ([5, 600], [2 ** 40], np.arange(600)):
            assert h.remove(bad) == (_lib.ERR_INVALID_ARG, 0)
            unchanged()
        long_row = st.copy()
        long_row.deg0[17] = st.M0 + 1
        far_id = st.copy()
        far_id.ids0[17, 0] = 600
        far_upper = st.copy()
        far_upper.idsu[next(r for r in range(st.U) if st.degu[r] > 0), 0] = 600   # (a layer-1 row that holds an edge)
        for bad in (long_row, far_id, far_upper):
            assert h.adopt(bad, 40) == _lib.ERR_INVALID_ARG
            unchanged()
        assert h.adopt(st, 1025) == _lib.ERR_INVALID_ARG
        unchanged()
        assert h.remove([5]) == (0, 1)   # ... and the handle is usable
    half = st.vec.astype(np.float16)
    off, nb = hh.flatten(st, st.max_layer)
    g = C.c_void_p()
    L = _lib.load()
    assert L.expann_graph_create_f16(64, 0, half.ctypes.data, st.n, st.max_layer, st.sv, off.ctypes.data, nb.ctypes.data,
                                     C.byref(g)) == 0
    h16 = hh.Handle.__new__(hh.Handle)
    h16.L, h16.h, h16.M, h16.M0 = L, g, st.M, st.M0
    assert h16.adopt(st, 40) == _lib.ERR_UNSUPPORTED
    h16.close()
