"""The inputs of tests/test_gpu_graph_handle_mutations.py decide something: from the CPU references alone, on the same
generators and seeds, every precondition of the GPU cases holds, plausible wrong variants of the gather's streaming
give another graph than THE GRAPH REMOVE RULE on the streamed input, flatten() does not depend on the row strides,
and offsets that forget the scan's carry past entry 524 288 change what a walk over the many-layer graph does.

No device.  Every measured value is printed (pytest -s shows them) and stands in DESIGN.md 4.9m."""
import numpy as np
import pytest

import graph_handle_helpers as hh
from graph_build_helpers import Params, restride


@pytest.fixture(scope="module")
def streamed():
    st, ids, q = hh.streamed_case()
    layers = hh.to_layers(st)
    return st, ids, layers, hh.pending_profile(layers, hh.gone_mask(st.n, ids))


@pytest.fixture(scope="module")
def many():
    """the many-layer graph after its append, by the oracle"""
    st, rng, q = hh.drawn_case(6002, 4300)
    ext = hh.extended(st, rng.standard_normal((3, 64)).astype(np.float32), [250, 250, 250])
    ext.oracle_build(ext.n, st.n, Params(40))
    return ext, q


def test_streamed_gather_preconditions(streamed):
    st, ids, layers, prof = streamed
    two = sum(1 for (v, l), x in prof.items() if l == 0 and x[0] >= 2)
    three = sum(1 for x in prof.values() if x[0] >= 3)
    twice = sum(1 for x in prof.values() if x[2])
    print("streamed gather: touched rows %d, layer-0 rows with >= 2 chunks %d, rows with >= 3 chunks %d, rows with a vertex "
          "adopted in two chunks %d" % (len(prof), two, three, twice))
    assert two >= 20 and three >= 1 and twice >= 5
    assert int(st.deg0.min()) == st.M0 == 64   # (why prune_overflow = 64 builds the before graph)


def test_cap_edge_preconditions(streamed):
    st, ids, layers, prof = streamed
    counts = sorted(x[1] for x in prof.values() if x[0] >= 2)
    c = counts[len(counts) // 2]
    exact = sum(1 for x in prof.values() if x[0] >= 2 and x[1] == c)
    more = sum(1 for x in prof.values() if x[0] >= 2 and x[1] > c)
    long_pending = sum(1 for x in prof.values() if x[3] > 1024)
    print("cap edges: distinct candidates of streamed rows %d .. %d, c = %d held by %d rows, exceeded by %d; rows with "
          "more than 1 024 pending candidates %d" % (counts[0], counts[-1], c, exact, more, long_pending))
    assert 64 < c <= 1024 and exact >= 1 and more >= 1
    assert counts[-1] < 1024 and long_pending >= 1 and counts[0] > 64
    # the boundary decides the counter: the rule counts > cap, a row with exactly c candidates is not truncated
    _, at_c = hh.strided_remove(st, ids, c, Params(c), only=set())
    assert at_c["truncated"] == sum(1 for x in prof.values() if x[1] > c) < sum(1 for x in prof.values() if x[1] >= c)


def test_task_chunk_preconditions():
    st, ids, _ = hh.task_chunk_case()
    touched = len(hh.pending_profile(hh.to_layers(st), hh.gone_mask(st.n, ids)))
    print("task chunks: touched rows %d = 16 384 + %d" % (touched, touched - 16384))
    assert 16384 < touched < 32768 and touched % 16384 != 0


def test_upper_growth_and_reopen_preconditions():
    st, rng, _ = hh.drawn_case()
    top = st.max_layer - 1
    U_cap, L_cap = st.U + st.U // 2 + 128, top + 2
    print("upper growth: U %d, U_cap %d, U_new %d; top level %d, L_cap %d, L_need %d" % (st.U, U_cap, st.U + 300, top, L_cap, top + 4))
    assert st.U + 300 > U_cap and top + 4 > L_cap
    st, rng, _ = hh.drawn_case(6004, 700)
    high = int((st.levels >= 2).sum())
    print("reopen: max_layer %d, %d vertices of level >= 2 go, max_layer 2 stays" % (st.max_layer, high))
    assert st.max_layer - 2 >= 2 and high >= 3 and int((st.levels == 1).sum()) > 0


def test_many_layer_preconditions(many):
    ext, _ = many
    off, nb = hh.flatten(ext, ext.max_layer)
    tiles = (off.size + 2047) // 2048
    print("many layers: %d x %d = %d offsets, %d tiles of 2 048, %d edges; the remove's kernels run over %d entries"
          % (off.shape[0], off.shape[1], off.size, tiles, len(nb), ext.max_layer * ext.n))
    assert off.size > 1048576 and off.size % 2048 != 0 and tiles > 512 and ext.max_layer * ext.n > 10 ** 6
    assert hh.batches(ext.levels, ext.n, 4300, 5) == 2 and len(nb) == hh.edge_count(ext)


# ---- wrong variants of the gather's streaming, as remove_core's select= ------------------------------------------------
def _merge(best, new, cap):
    lst = sorted(best + new)
    return lst[:cap], len(lst) > cap


def dedup_within_a_chunk_only(own, chunks, cap):
    best, cut = sorted(own), False
    for ch in chunks:
        best, c = _merge(best, sorted(set(ch)), cap)
        cut = cut or c
    return best, cut


def no_merge_with_the_best_so_far(own, chunks, cap):
    best, cut = sorted(own), False
    for ch in chunks:   # each chunk's cap smallest join the own entries alone: what earlier chunks gave is forgotten
        best, c = _merge(sorted(own), sorted(set(ch)), cap)
        cut = cut or c
    return best, cut


def cut_at_cap_minus_one(own, chunks, cap):
    lst = sorted(set(own) | {x for ch in chunks for x in ch})
    return lst[:cap - 1], len(lst) > cap


def count_at_cap_as_truncated(own, chunks, cap):
    lst = sorted(set(own) | {x for ch in chunks for x in ch})
    return lst[:cap], len(lst) >= cap


def _differing_rows(a, b):
    return sum(1 for x, y in zip(a["layers"], b["layers"]) for (xi, xd), (yi, yd) in zip(x, y)
               if not (np.array_equal(xi, yi) and np.array_equal(xd.view(np.uint32), yd.view(np.uint32))))


def test_wrong_variants_give_another_graph(streamed):
    st, ids, layers, prof = streamed
    p = Params(80)
    _, true = hh.strided_remove(st, ids, 80, p)
    _, again = hh.strided_remove(st, ids, 80, p, select=lambda own, chunks, cap: (sorted(set(own) | {x for ch in chunks for x in ch})[:cap],
                                                                                    len(set(own) | {x for ch in chunks for x in ch}) > cap))
    assert _differing_rows(true, again) == 0 and true["truncated"] == again["truncated"]   # (select= restates the rule)
    for variant in (dedup_within_a_chunk_only, no_merge_with_the_best_so_far, cut_at_cap_minus_one):
        _, wrong = hh.strided_remove(st, ids, 80, p, select=variant)
        rows = _differing_rows(true, wrong)
        print("wrong variant %s: %d of %d touched rows differ" % (variant.__name__, rows, true["touched"]))
        assert rows > 0
    # `>= cap` changes no row, only the counter -- on the input whose cap is a row's exact count
    counts = sorted(x[1] for x in prof.values() if x[0] >= 2)
    c = counts[len(counts) // 2]
    rows_at_c = {k for k, x in prof.items() if x[1] == c}
    _, true_c = hh.strided_remove(st, ids, c, Params(c), only=rows_at_c)
    _, wrong_c = hh.strided_remove(st, ids, c, Params(c), only=rows_at_c, select=count_at_cap_as_truncated)
    print("wrong variant count_at_cap_as_truncated: the counter reads %d against %d" % (wrong_c["truncated"] + 0, true_c["truncated"]))
    assert wrong_c["truncated"] == true_c["truncated"] + len(rows_at_c) > true_c["truncated"]


def test_flatten_does_not_depend_on_the_strides(streamed, many):
    for st in (streamed[0], many[0]):
        a, b = hh.flatten(st, st.max_layer), hh.flatten(restride(st, st.stride0 + 12, st.strideu + 4), st.max_layer)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[0].dtype == np.uint64 and a[1].dtype == np.uint32 and int(a[0][-1, -1]) == len(a[1]) == hh.edge_count(st)


def _descend(off, nb, vec, sv, q):
    """greedy descent through the layers above the bottom: (the vertex it enters layer 0 at, distance evaluations)"""
    cur, evals = sv, 1
    d_cur = float(((vec[cur] - q) ** 2).sum())
    for l in range(off.shape[0] - 1, 0, -1):
        moved = True
        while moved:
            moved = False
            row = nb[int(off[l, cur]):int(off[l, cur + 1])].astype(np.int64)
            evals += len(row)
            if len(row):
                d = ((vec[row] - q) ** 2).sum(axis=1)
                j = int(np.argmin(d))
                if d[j] < d_cur:
                    cur, d_cur, moved = int(row[j]), float(d[j]), True
    return cur, evals


def test_offsets_that_forget_the_carry_change_the_walk(many):
    ext, q = many
    off, nb = hh.flatten(ext, ext.max_layer)
    flat = off.reshape(-1).copy()
    flat[524288:] -= flat[524288]   # what append_scan_sums_kernel would leave without its carry into the third round
    broken = flat.reshape(off.shape)
    assert (broken[123:] != off[123:]).all()
    differ = sum(_descend(off, nb, ext.vec, ext.sv, x) != _descend(broken, nb, ext.vec, ext.sv, x) for x in q)
    print("forgotten carry: %d of 32 queries enter layer 0 elsewhere or after another count of evaluations" % differ)
    assert differ >= 1


def test_the_array_prune_is_prune_edges(streamed):
    """prune_list (one oracle call per list or per pick, float32 arrays) against prune_edges, the pair-by-pair
    statement it replaced inside apply_remove: the same edges in the same order, on both of its paths"""
    import graph_remove_helpers as grh
    st = streamed[0]
    dist = grh._Dist(st.vec)
    for v in range(0, 800, 67):
        order = np.lexsort((st.ids0[v, :64], st.d0[v, :64]))
        d, ids = st.d0[v, :64][order], st.ids0[v, :64][order].astype(np.int64)
        for limit, po in ((16, 0), (16, 1), (40, 0), (64, 2)):   # (64 candidates: above 2 * limit the rows come per pick)
            want = grh.prune_edges(list(zip(d, ids.tolist())), limit, dist, np.float32(0.5), np.float32(0.0), po)
            got = grh.prune_list(d, ids, limit, st.vec, 0.5, 0.0, po)
            assert [(x.view(np.uint32), i) for x, i in got] == [(np.float32(x).view(np.uint32), i) for x, i in want]
            assert 0 < len(got) <= limit
