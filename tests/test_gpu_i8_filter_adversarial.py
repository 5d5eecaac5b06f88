"""Adversarial soundness of the int8 filter of fp32 rows (scan_gemm_i8f.hpp), forced on (i8_filter = 2, d = 128).

The filter may drop a row only when its interval [L, L + W_q + W_b] proves it outside the k best, the select may cut
a candidate only when its lower bound exceeds an exact k-th score, and the redo pass's proven tau must reach the k-th
score.  On iid, clustered, scaled or clipped data the quantisation errors are uncorrelated with the vectors and a pair
uses a few percent of that room (tests/test_i8f_model.py: at most 0.15 of the half-width).  The data here is built
(tests/i8f_model.py) so that the errors line up with the vectors -- every component half a cell off, the error
vector parallel (or anti-parallel) to the query and to the row, |e| / |x| = lambda -- and the threshold has no room
of its own: the planted rows use 0.97 - 0.99 of the half-width (measured on the host model, asserted there), so a
lambda, c, eps, M_q, floor margin or ulp(aq) term wrong by a factor of two loses neighbours here.

Every case: ids and distance bits equal the oracle's, and the int8 scan -- no retry on another form -- gave them."""
import numpy as np
import pytest

import i8f_model as im

pytestmark = pytest.mark.gpu

K = im.K
I8F = "scan_gemm_i8w<128,F32L2>"
STATS = ("redo_queries", "redo_candidates", "redo_overflows", "spec_rank", "i8_sample", "rerank_rows")


@pytest.fixture(scope="module")
def gpu():
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_device_count() >= 1, "these tests need a HIP device"
    return L


def _run(base, queries, **opts):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(base.shape[1], "l2")
    eng.store_many_vectors(base)
    eng.build()
    eng.set_option("i8_filter", 2)
    for name, val in opts.items():
        eng.set_option(name, val)
    eng.set_profiling(True)
    ids, dists = eng.query_k_batch(queries, K)
    prof = eng.get_profile()
    st = {s: eng.get_stat(s) for s in STATS}
    eng.close()
    return ids, dists, prof, st


def _exact_on_the_int8_path(ids, dists, ref, prof, st, what):
    print(what, prof["scan_kernel"], "retries", prof["retries"], "candidates", prof.get("candidates"), st)
    assert np.array_equal(ids, ref[0]), (what, prof, st)
    assert np.array_equal(dists.view(np.uint32), ref[1].view(np.uint32)), (what, prof, st)
    assert prof["scan_kernel"] == I8F and prof["retries"] == 0, (what, prof, st)


@pytest.fixture(scope="module")
def drop(oracle):
    base, q, fam, _ = im.build_drop()
    ref = oracle.brute_force(base, q, K, oracle.METRIC_L2_F32, n_threads=16)
    assert np.array_equal(np.sort(ref[0], axis=1), np.sort(fam.astype(np.uint64), axis=1))
    assert im.I8fModel(base).s == 2.0 ** im.E
    return base, q, ref


@pytest.fixture(scope="module")
def cut(oracle):
    """the (a) index plus 16 decoys per query; the model asserts, query by query, that the decoys have the smaller keys
    and the larger exact scores (so the first round re-scores decoys alone) before anything runs on the GPU"""
    base, q, fam, dec = im.build_drop(decoys=16)
    mod = im.I8fModel(base)
    assert mod.s == 2.0 ** im.E
    Q = mod.queries(q)
    rows = np.concatenate([fam, dec], axis=1)
    for i in range(len(q)):
        S_i = np.full(base.shape[0], np.inf, dtype=np.float32)
        kept, sc = oracle.filter_by_score(base, q[i], rows[i].astype(np.uint64), np.float32(np.inf), oracle.METRIC_L2_F32)
        S_i[kept.astype(np.int64)] = sc
        im.assert_cut_orderings(mod, {name: v[i:i + 1] for name, v in Q.items()}, S_i, fam[i], dec[i])
    ref = oracle.brute_force(base, q, K, oracle.METRIC_L2_F32, n_threads=16)
    assert np.array_equal(np.sort(ref[0], axis=1), np.sort(fam.astype(np.uint64), axis=1))
    return base, q, ref


@pytest.mark.parametrize("spec_rank", [K, 0])
@pytest.mark.parametrize("rounds", [2, 1])
def test_drop_direction(gpu, drop, rounds, spec_rank):
    """(a): the k best rows of every query lie 0.987 of the half-width below their centres, the fp16 sampled pass
    reads them (k residues mod 32 of one chunk) and its tau is their k-th score plus the fp16 slack alone.
    spec_rank = k: proven thresholds; 0: auto"""
    base, q, ref = drop
    ids, dists, prof, st = _run(base, q, rerank_rounds=rounds, spec_rank=spec_rank)
    _exact_on_the_int8_path(ids, dists, ref, prof, st, f"drop, rounds {rounds}, spec_rank {spec_rank}:")


@pytest.mark.parametrize("spec_rank", [K, 0])
@pytest.mark.parametrize("rounds", [2, 1])
def test_cut_direction(gpu, cut, rounds, spec_rank):
    """(b): 16 decoys per query take the first re-rank round; T is their k-th score, one cell above the k-th family
    score, and the family rows must survive kappa <= (T - tau_q) / 2s^2 with 0.986 of their half-width used (one round:
    kappa <= kth(kappa + w_b) + w_q).  Every list holds the 16 decoys and the k family rows at least, and all of them
    are re-scored: the second round did real work"""
    base, q, ref = cut
    ids, dists, prof, st = _run(base, q, rerank_rounds=rounds, spec_rank=spec_rank, rerank_stats=1)
    _exact_on_the_int8_path(ids, dists, ref, prof, st, f"cut, rounds {rounds}, spec_rank {spec_rank}:")
    assert st["rerank_rows"] >= (16 + K) * len(q), st


@pytest.fixture(scope="module")
def sample(oracle):
    base, q, near, mid = im.build_sample()
    mod = im.I8fModel(base)
    assert mod.s == 2.0 ** im.E
    ref = oracle.brute_force(base, q, K, oracle.METRIC_L2_F32, n_threads=16)
    bites = im.sample_bites(mod, mod.queries(q), near, mid, ref)       # (asserts the construction's claims)
    assert bites.min() > 0.9724 - 0.05, bites.min()
    return base, q, ref


@pytest.mark.parametrize("redo_bound", [0, 1])
def test_proven_tau_of_the_int8_sampled_pass(gpu, sample, redo_bound):
    """(c): i8_sample = 2, spec_rank = 1.  The planted rows' errors are anti-parallel to query and row: they look a
    half-width nearer than they are.  tau_s, the best class maximum's centre, lies below every score; the speculative
    list holds the 5 near rows alone, so the redo pass filters with the proven tau made from g_k -- a row whose exact
    score is 0.972 of the way from its centre to that tau (the host model asserts tau >= S_k with that little room).
    What the GPU run adds is the path -- int8 class maxima, the failed short list, the redo pass on the proven tau,
    exact -- not a second factor-two check: a query whose error is anti-parallel to it puts every near row's score at
    or above its centre, so the rows' own lower bounds lie a half-width below any tau the maxima can give, and a
    tau short by half its room still lets them through (tried: halved slack fails (a), (b) and (d), not this)"""
    base, q, ref = sample
    assert len(q) > 64
    ids, dists, prof, st = _run(base, q, i8_sample=2, spec_rank=1, redo_bound=redo_bound)
    _exact_on_the_int8_path(ids, dists, ref, prof, st, f"proven tau, redo_bound {redo_bound}:")
    assert st["i8_sample"] == 1 and st["redo_queries"] > 0 and st["redo_overflows"] == 0, st


@pytest.mark.parametrize("kind", ["clip", "clamp"])
def test_edges_of_the_integer_range(gpu, oracle, kind):
    """(d): "clip": a query and a family row with a component beyond the clip (M_q = 2 B |e_q|); "clamp": a row whose
    bp sits at the lower clamp limit (key -inf, a candidate of every query).  The other rows stay as tight as in (a)"""
    base, q, fam = im.build_edge(kind)
    ref = oracle.brute_force(base, q, K, oracle.METRIC_L2_F32, n_threads=16)
    assert np.array_equal(np.sort(ref[0], axis=1), np.sort(fam.astype(np.uint64), axis=1))
    ids, dists, prof, st = _run(base, q)
    _exact_on_the_int8_path(ids, dists, ref, prof, st, f"edge {kind}:")
    if kind == "clamp":
        assert prof["candidates"] >= (K + 1) * len(q), prof         # the clamped row reached every list
