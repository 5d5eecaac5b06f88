"""The batched GPU builder (expann_graph_build_batched: build_search_kernel, build_prune_kernel,
build_reverse_kernel, build_clamp_kernel and the host's batch loop) against the oracle's CPU restatement of
the same contract (oracle_graph_build_batched), bit for bit: ids, distance bits, degrees, max_layer,
starting_vertex and the counters.  No tolerances.

The build is driven one batch per call; both sides start every batch from the same arrays (the oracle's state
after the previous batch).  Within one batch only the order in which reverse edges land in a row is left open,
and nothing reads it before the row is sorted, so new rows and re-pruned rows are compared in order and every
other row as its old prefix plus a sorted list of appended (id, distance bits) pairs
(graph_build_helpers.compare_batch).  One test makes whole multi-batch calls, where that order can matter
through distance ties only; it asserts that the oracle met none."""
import functools

import numpy as np
import pytest

from graph_build_helpers import (Params, Strided, compare_run, contraction_case, draw_levels, drive_batches, restride,
                                 seed_graph, sift_like)

pytestmark = pytest.mark.gpu

# data seed of test_host_batch_loop_in_one_call
HOST_LOOP_SEED = 2   # (tie_hazards at max_batch 0 / 7 -- seed 0: 1 / 0; seeds 1 to 5: 0 / 0)


def _gauss(seed, n, d, M):
    rng = np.random.RandomState(seed)
    return rng.standard_normal((n, d)).astype(np.float32), draw_levels(rng, n, M)


@functools.lru_cache(maxsize=None)
def _seed_gauss64():
    """d 64, M 8 / M0 16, the first 256 of 1200 rows built (shared, never written)"""
    vec, levels = _gauss(64, 1200, 64, 8)
    return seed_graph(vec, levels, 8, 16, 256, Params(40))


def test_gaussian_rows_compiled_dim():
    """the plain path: 256 -> 1200 rows, d 64 (a compiled instance), upper layers, re-pruned rows"""
    st = _seed_gauss64()
    st, batches, repruned, _ = drive_batches(st, 1200, 256, Params(40))
    assert batches > 20 and repruned > 1000
    assert st.max_layer >= 3 and (st.degu[:st.U] > 0).sum() > 50


def test_integer_rows_with_ties():
    """SIFT-like integer rows, 5 % exact duplicates of earlier rows, prune_overflow 1: equal distances in the
    queues, in the descent and in the prune's sort (first of equals), co == basic, edges of length 0"""
    rng = np.random.RandomState(128)
    n, d, M = 700, 128, 6
    vec = sift_like(rng, n, d)
    dup = rng.choice(np.arange(50, n), n // 20, replace=False)
    vec[dup] = vec[rng.randint(0, 50, dup.size)]
    levels = draw_levels(rng, n, M)
    p = Params(32, prune_overflow=1)
    st = seed_graph(vec, levels, M, 2 * M, 200, p)
    seen = {"hazards": 0, "zero": 0}

    def look(bef, orc, ro, b0, b1):
        seen["hazards"] += ro["tie_hazards"]
        for v in range(b0, b1):
            seen["zero"] += int((orc.d0[v, :orc.deg0[v]] == 0).sum())
    st, batches, repruned, _ = drive_batches(st, n, 200, p, on_batch=look)
    assert seen["hazards"] > 20 and seen["zero"] > 5 and repruned > 100, seen


@pytest.mark.parametrize("d,n_built,n", [(48, 200, 700), (1040, 150, 400)])
def test_run_time_dims(d, n_built, n):
    """the D = 0 instances of the search and prune kernels (row in dynamic LDS)"""
    vec, levels = _gauss(d, n, d, 8)
    p = Params(40)
    st = seed_graph(vec, levels, 8, 16, n_built, p)
    st, batches, repruned, _ = drive_batches(st, n, n_built, p)
    assert repruned > 50 and st.max_layer >= 2


def test_long_rows():
    """M 70 / M0 140, stride0 204, ef 150 and a prune that kills nobody (prune_overflow 200): rows longer than
    128 entries (the second half of the search's neighbour loop), more than 64 reverse edges per new row,
    prune lists above 128"""
    vec, levels = _gauss(140, 900, 64, 70)
    levels[[3, 40, 90, 200, 333, 450, 600, 777]] = 1   # (M = 70 draws almost no upper rows)
    p = Params(150, prune_overflow=200)
    st = seed_graph(vec, levels, 70, 140, 400, p, slack=64)
    assert st.stride0 == 204 and st.deg0[:400].max() > 128
    st, batches, repruned, _ = drive_batches(st, 900, 400, p)
    assert st.deg0[400:].min() > 64 and st.deg0.max() == 140 and repruned > 1000


@functools.lru_cache(maxsize=None)
def _seed_1500():
    vec, levels = _gauss(1500, 1532, 64, 8)
    return seed_graph(vec, levels, 8, 16, 1500, Params(40))


@pytest.mark.parametrize("ef,stride0", [(300, None), (1024, None), (300, 1024)])
def test_prune_capacity(ef, stride0):
    """one batch of 32 on 1500 rows: candidate lists spread over 2 and 4 per thread of the prune kernel, a
    length that is no power of two, the 1024-candidate bound, and rows of the longest stride allowed"""
    st = _seed_1500()
    if stride0:
        st = restride(st, stride0=stride0)
    seen = []
    st, batches, repruned, _ = drive_batches(st, 1532, 1500, Params(ef), max_batch=32,
                                             on_batch=lambda bef, orc, ro, b0, b1: seen.append((b0, b1)))
    assert seen == [(1500, 1532)] and repruned > 20


def test_from_nothing():
    """n_built = 1: the first search meets one vertex with empty rows (C = 1), batches of one up to 32 rows"""
    vec, levels = _gauss(1, 40, 64, 8)
    levels[:] = 0
    levels[[0, 6, 21, 35]] = 1
    levels[12] = 2
    st = Strided(vec, levels, 8, 16)
    assert st.max_layer == 2
    st, batches, _, _ = drive_batches(st, 40, 1, Params(40))
    assert (batches, st.max_layer, st.sv) == (35, 3, 12)   # (31 batches of one, then four of two)


def test_layer_openers():
    """hand-set levels: a vertex at max_layer (70, in the middle of what would be a batch), one two layers
    further up (80), two openers in a row (90, 91): each goes alone, the layers skipped are opened one by one,
    max_layer_io / starting_vertex_io and stats[0] as the oracle's -- per batch, and in one call over all"""
    vec, levels = _gauss(7, 200, 64, 8)
    levels = np.minimum(levels, 1)
    levels[0] = 1
    levels[[70, 80, 90, 91]] = [2, 5, 6, 7]
    p = Params(40)
    seed = seed_graph(vec, levels, 8, 16, 64, p)
    assert seed.max_layer == 2
    cuts, tops = [], []

    def look(bef, orc, ro, b0, b1):
        cuts.append((b0, b1))
        tops.append((orc.max_layer, orc.sv))
    st, batches, _, _ = drive_batches(seed, 200, 64, p, on_batch=look)
    for v in (70, 80, 90, 91):
        assert (v, v + 1) in cuts and not any(a < v < b for a, b in cuts)
    assert tops[cuts.index((70, 71))] == (3, 70) and tops[cuts.index((80, 81))] == (6, 80)
    assert tops[cuts.index((90, 91))] == (7, 90) and tops[-1] == (8, 91)
    gpu, orc = seed.copy(), seed.copy()
    rg = gpu.gpu_build(200, 64, p)
    ro = orc.oracle_build(200, 64, p)
    assert ro["tie_hazards"] == 0 and int(ro["stats"][0]) == batches
    compare_run(gpu, orc, rg, ro)


@pytest.mark.parametrize("ortho_bias", [0.0, 0.25, 0.1])
@pytest.mark.parametrize("ortho_factor", [0.0, 0.5, 1.5])
def test_score_parameters(ortho_factor, ortho_bias):
    """ortho_factor x ortho_bias x prune_overflow {0, 1, 3}, 256 -> 600 rows: the score arithmetic.  The rule is
    the unfused form, each operation rounded: factor * (basic - co), then + bias, then res +="""
    for po in (0, 1, 3):
        p = Params(40, po, ortho_factor, ortho_bias)
        _, batches, repruned, _ = drive_batches(_seed_gauss64(), 600, 256, p)
        assert repruned > 100, po


def test_no_slack():
    """slack 2 and one batch of 64 new rows in one tight cluster: rows receive more reverse edges than they
    have room for.  stats[1] equals the oracle's count; rows that took all their edges compare exactly, the
    others keep the invariants (which edges were dropped depends on the order of the atomics)"""
    rng = np.random.RandomState(2)
    n_built, n, d = 1024, 1088, 64
    centres = rng.standard_normal((8, d)).astype(np.float32)
    vec = (centres[rng.randint(0, 8, n)] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    vec[n_built:] = (centres[3] + 0.05 * rng.standard_normal((64, d))).astype(np.float32)
    levels = draw_levels(rng, n, 8)
    levels[n_built:] = np.minimum(levels[n_built:], 1)
    p = Params(40, prune_overflow=2)
    st = restride(seed_graph(vec, levels, 8, 16, n_built, p), stride0=18, strideu=10)
    dropped = []
    st, batches, repruned, n_over = drive_batches(st, n, n_built, p, overflow=True,
                                                  on_batch=lambda bef, orc, ro, b0, b1: dropped.append(int(ro["stats"][1])))
    assert batches == 1 and dropped[0] > 0 and n_over > 0 and repruned > n_over


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("d", [64, 16])
def test_score_is_not_contracted(d, which):
    """four lattice rows on which one fused multiply-add in factor * (basic - co) + bias changes the order of
    the new row (graph_build_helpers.contraction_case), through the compiled and the run-time-dim prune kernel"""
    vec, p, row = contraction_case(d, which)
    seed = seed_graph(vec, np.zeros(4, np.uint8), 4, 8, 3, p)
    st, _, _, _ = drive_batches(seed, 4, 3, p)
    assert st.ids0[3, :st.deg0[3]].tolist() == row


def test_row_counter_past_the_stride():
    """a row whose degree counter stands past the stride (as the reverse kernel leaves a row that is not
    re-pruned and runs out of slack) is read up to the stride, not further.  Two clusters without an edge
    between them, the entry point in the first, the new vertex next to the second; the one way across would be
    to read the row of vertex 9 past its stride into the row of vertex 10, which starts with three edges into
    the second cluster"""
    import oracle_ctypes as oc
    rng = np.random.RandomState(9)
    d, M0 = 64, 16
    vec = (0.1 * rng.standard_normal((21, d))).astype(np.float32)
    vec[10:] += 4.0                                   # rows 10 .. 19 and the new row 20: the second cluster
    st = Strided(vec, np.zeros(21, np.uint8), 8, M0, stride0=M0, strideu=8)
    for lo in (0, 10):                                # every cluster: all-to-all rows, true edge lengths
        for v in range(lo, lo + 10):
            nb = [u for u in range(lo, lo + 10) if u != v]
            st.ids0[v, :9] = nb
            st.d0[v, :9] = [oc.l2_f32(vec[v], vec[u]) for u in nb]
            st.deg0[v] = 9
    st.ids0[9, 9:] = st.ids0[9, 0]                    # (between degree and stride: a repeated edge)
    st.d0[9, 9:] = st.d0[9, 0]
    st.deg0[9] = M0 + 3
    assert st.ids0[10, :3].tolist() == [11, 12, 13]
    p = Params(40)   # (ef above stride0 + 3: the hop's neighbour list in LDS has room for every entry read)
    out, _, _, _ = drive_batches(st, 21, 20, p)
    row = out.ids0[20, :out.deg0[20]].tolist()
    assert row and max(row) < 9, row                  # (the first cluster only, and not vertex 9: its row is full)


def test_descent_takes_the_first_of_equal_minima():
    """two identical rows (1 and 2) on layer 1, both in the entry point's row and both nearest to the new
    vertex: the descent moves to the one that comes first in the row, and with ef_construction = 1 the new
    vertex's only edge is that one"""
    rng = np.random.RandomState(12)
    d = 64
    vec = np.round(4 * rng.standard_normal((12, d))).astype(np.float32)
    vec[2] = vec[1]
    vec[11] = vec[1]
    vec[11, 0] += 1                                   # the new vertex: 1 away from rows 1 and 2, far from the rest
    levels = np.zeros(12, np.uint8)
    levels[:3] = 1
    seed = seed_graph(vec, levels, 4, 8, 11, Params(8, prune_overflow=4))
    up0 = seed.idsu[seed.urow(1, 0), :seed.degu[seed.urow(1, 0)]].tolist()
    assert seed.sv == 0 and sorted(up0) == [1, 2]
    hazards = []
    out, _, _, _ = drive_batches(seed, 12, 11, Params(1), on_batch=lambda bef, orc, ro, b0, b1: hazards.append(ro["tie_hazards"]))
    assert hazards[0] > 0 and out.ids0[11, :out.deg0[11]].tolist() == [up0[0]]


@pytest.mark.parametrize("max_batch", [0, 7])
def test_host_batch_loop_in_one_call(max_batch):
    """64 -> 800 rows in ONE call (many batches, layer openers among them) against the oracle's full run.
    Across batches the order of a row's appended edges can matter through distance ties only, so the test
    requires that the oracle met no such tie (tie_hazards == 0; the data seed was chosen for it on the CPU)."""
    vec, levels = _gauss(HOST_LOOP_SEED, 800, 64, 6)
    p = Params(16)
    seed = seed_graph(vec, levels, 6, 12, 64, p)
    gpu, orc = seed.copy(), seed.copy()
    ro = orc.oracle_build(800, 64, p, max_batch)
    assert ro["tie_hazards"] == 0
    assert orc.max_layer > seed.max_layer and int(ro["stats"][0]) > (100 if max_batch else 40)
    rg = gpu.gpu_build(800, 64, p, max_batch)
    compare_run(gpu, orc, rg, ro)

