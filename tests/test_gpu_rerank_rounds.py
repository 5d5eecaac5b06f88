"""The select's two-round exact re-rank of the int8 filter's lists (scan_gemm_i8f.hpp "Two rounds"):
the rows of the R1 = max(16, k rounded up to 16) smallest filter keys are re-scored first, T = their k-th exact score,
and of the others only the rows whose proven lower bound tau_f + 2 s^2 kappa does not exceed T.  A dropped row scores
strictly more than T, so ids and distance bits are the oracle's in every case below, with "rerank_rounds" 2 (default)
and 1 (the single cut by interval bounds)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, K = 262_144 + 4_096, 128, 10   # (the smallest index on which the sampled pass reads 1/16 of the rows)
I8F = "scan_gemm_i8w<128,F32L2>"


@pytest.fixture(scope="module")
def gpu():
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_device_count() >= 1, "these tests need a HIP device"
    return L


@pytest.fixture(scope="module")
def iid():
    rng = np.random.RandomState(20262)
    return rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((2048, D)).astype(np.float32)


@pytest.fixture(scope="module")
def iid_ref(oracle, iid):
    base, queries = iid
    return oracle.brute_force(base, queries, K, oracle.METRIC_L2_F32, n_threads=16)


def _same(ids, dists, rids, rd, what=""):
    assert np.array_equal(ids, rids), what
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32)), what


def _run(base, queries, k, **opts):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(base.shape[1], "l2")
    eng.store_many_vectors(base)
    eng.build()
    eng.set_option("i8_filter", 2)
    for name, val in opts.items():
        eng.set_option(name, val)
    eng.set_profiling(True)
    ids, dists = eng.query_k_batch(queries, k)
    prof = eng.get_profile()
    st = {s: eng.get_stat(s) for s in ("redo_queries", "redo_candidates", "redo_overflows", "spec_rank", "rerank_rows")}
    eng.close()
    return ids, dists, prof, st


def test_two_rounds_rescore_fewer_rows_than_one(gpu, iid, iid_ref):
    """iid rows, 2 048 queries: both settings are exact and the two rounds re-score strictly fewer rows in all.  (A
    numpy model of the header's formulas, profiles/rerank_rounds_model.py, puts the ratio near 0.33 at 1 M rows x
    10 000 queries; printed here, not asserted.  Measured on MI355X on this batch: 33.9 rows per query against
    103.3, ratio 0.328, of 438 candidates per query -- proven thresholds at 2 048 queries.)"""
    base, queries = iid
    rows = {}
    for rounds in (2, 1):
        ids, dists, prof, st = _run(base, queries, K, rerank_rounds=rounds, rerank_stats=1)
        _same(ids, dists, iid_ref[0], iid_ref[1], (rounds, prof, st))
        assert prof["scan_kernel"] == I8F and prof["retries"] == 0, (rounds, prof, st)
        rows[rounds] = st["rerank_rows"]
        print(f"rerank_rounds {rounds}: {st['rerank_rows']} rows re-scored, {st['rerank_rows'] / len(queries):.1f} per query, "
              f"{prof['candidates'] / len(queries):.1f} candidates per query, {st}")
    print(f"rows re-scored, two rounds / one round: {rows[2] / max(1, rows[1]):.3f}")
    assert 0 < rows[2] < rows[1], rows


def test_without_the_option_nothing_is_counted(gpu, iid, iid_ref):
    base, queries = iid
    ids, dists, prof, st = _run(base, queries[:300], K)
    _same(ids, dists, iid_ref[0][:300], iid_ref[1][:300], (prof, st))
    assert prof["retries"] == 0 and st["rerank_rows"] == 0, (prof, st)


@pytest.fixture(scope="module")
def tied(oracle):
    """every row twice (all scores -- and all filter keys -- come in equal pairs), and for the first 40 queries the
    row of the 5th pair a third time: their 9th, 10th and 11th best are byte-identical rows, so the first round's T
    is a score that a row outside the k best ties with exactly, and the k-th place goes to the lower id"""
    rng = np.random.RandomState(78)
    half = rng.standard_normal((N // 2, D)).astype(np.float32)
    queries = rng.standard_normal((600, D)).astype(np.float32)
    h5 = oracle.brute_force(half, queries[:40], 5, oracle.METRIC_L2_F32, n_threads=16)[0][:, 4].astype(np.int64)
    assert len(set(h5.tolist())) == 40
    base = np.concatenate([half, half[h5], half], 0)
    rids, rd = oracle.brute_force(base, queries, K + 1, oracle.METRIC_L2_F32, n_threads=16)
    # the cases are what they are meant to be (checked here, on the CPU): places 9-11 tie bit for bit, the oracle
    # ranks them by id, and the 10th place is the third copy -- the lower id of the 10th / 11th
    r11 = rd.view(np.uint32)
    good = [i for i in range(40)
            if r11[i, 8] == r11[i, 9] == r11[i, 10] and rids[i, 8] == h5[i] and rids[i, 9] == N // 2 + i
            and rids[i, 10] == N // 2 + 40 + h5[i]]
    assert len(good) >= 35, good
    return base, queries, np.ascontiguousarray(rids[:, :K]), np.ascontiguousarray(rd[:, :K])


@pytest.mark.parametrize("rank", [0, 2])
def test_ties_across_the_second_rounds_cut(gpu, tied, rank):
    """rank 0 (auto): the main select serves the tied queries; rank 2: ~10 % of the batch fails the check and the
    redo select (the same wave body, by query slot, tau_f = the slot's tau_r) serves those"""
    base, queries, rids, rd = tied
    ids, dists, prof, st = _run(base, queries, K, spec_rank=rank, rerank_stats=1)
    print(f"j = {rank}: {st}")
    _same(ids, dists, rids, rd, (prof, st))
    assert prof["scan_kernel"] == I8F and prof["retries"] == 0 and st["rerank_rows"] > 0, (prof, st)
    if rank == 2:
        assert st["spec_rank"] == 2 and st["redo_queries"] > 0, st


def test_fewer_than_k_rows_in_a_list(gpu, oracle, iid):
    """j = 1 on 300 queries, 100 of them next to five planted near copies: where the sample holds a copy the list
    holds the five copies and nothing else -- one round, T = +inf, everything is re-scored, the check fails and the
    query goes to the redo pass"""
    base, queries = iid
    rng = np.random.RandomState(4)
    base = base.copy()
    q = queries[:300].copy()
    rows = rng.choice(N, 500, replace=False).reshape(100, 5)
    for i in range(100):
        base[rows[i]] = q[i] + np.float32(0.01) * rng.standard_normal((5, D)).astype(np.float32)
    rids, rd = oracle.brute_force(base, q, K, oracle.METRIC_L2_F32, n_threads=16)
    ids, dists, prof, st = _run(base, q, K, spec_rank=1)
    print(f"j = 1: {st}")
    _same(ids, dists, rids, rd, (prof, st))
    assert prof["scan_kernel"] == I8F and prof["retries"] == 0 and st["redo_overflows"] == 0, (prof, st)
    assert st["redo_queries"] >= 20, st   # (~28 planted + ~90 iid)


def test_k_100_first_round_of_112_rows(gpu, oracle, iid, capfd, monkeypatch):
    """k = 100 on 512 queries: R1 = 112, the first round's keys come from the bisection, and the lists exceed 512
    keys -- the <16,2> / <32,1> stages' instances (read from the library's own report of the list lengths;
    measured: 1 457 candidates per query, longest list 1 852, rows re-scored two rounds / one 0.399)"""
    import re
    base, queries = iid
    m = 512
    rids, rd = oracle.brute_force(base, queries[:m], 100, oracle.METRIC_L2_F32, n_threads=16)
    monkeypatch.setenv("EXPANN_DEBUG_LISTS", "1")
    rows = {}
    for rounds in (2, 1):
        capfd.readouterr()
        ids, dists, prof, st = _run(base, queries[:m], 100, rerank_rounds=rounds, rerank_stats=1)
        longest = [int(x) for x in re.findall(r"\[lists\] attempt 0 .* max (\d+),", capfd.readouterr().err)]
        print(f"rerank_rounds {rounds}: longest list {longest}, {prof['candidates'] / m:.1f} candidates per query, {st}")
        _same(ids, dists, rids, rd, (rounds, prof, st))
        assert prof["scan_kernel"] == I8F and prof["retries"] == 0, (rounds, prof, st)
        assert longest and longest[0] > 512, longest
        rows[rounds] = st["rerank_rows"]
    print(f"k = 100, rows re-scored, two rounds / one round: {rows[2] / max(1, rows[1]):.3f}")
    assert 0 < rows[2] <= rows[1], rows


def test_batch_of_48_queries(gpu, iid, iid_ref):
    """48 queries: no wave stages, wave 0 of select_topk_kernel's workgroup orders the short lists"""
    base, queries = iid
    rows = {}
    for rounds in (2, 1):
        ids, dists, prof, st = _run(base, queries[:48], K, rerank_rounds=rounds, rerank_stats=1)
        print(f"rerank_rounds {rounds}: {st}, {prof['candidates'] / 48:.1f} candidates per query")
        _same(ids, dists, iid_ref[0][:48], iid_ref[1][:48], (rounds, prof, st))
        assert prof["scan_kernel"] == I8F and prof["retries"] == 0, (rounds, prof, st)
        rows[rounds] = st["rerank_rows"]
    assert 0 < rows[2] <= rows[1], rows


def test_a_row_whose_integer_term_is_clamped(gpu, oracle, iid):
    """one row scaled by 50: its integer row term leaves the int32 range the filter keeps (checked below on the
    CPU with scan_gemm_i8f.hpp's formula), bp is clamped, the row passes every query's filter with the key -inf,
    sorts first in every list and is re-scored in the first round.  255 ordinary queries: exact, no retry.  With a
    256th query EQUAL to that row -- it finds the row at place 1, distance 0 -- the batch is exact as well; that
    query's own quantisation error (it lies 50 x beyond the clip) lets every row pass its filter, so its list
    overflows and the batch is repeated on the fp16 form, as tests/test_gpu_i8_filter.py's
    test_queries_far_beyond_the_clip_fall_back shows for any such query: the retry is the library's answer there
    and is not asserted away."""
    base, queries = iid
    base = base.copy()
    r = 123_457
    base[r] *= np.float32(50.0)
    # the header's formula in fp64: s = min(max |x|, 5.5 rms) / 127, lambda = 1.4 s / (sqrt(12) rms),
    # A_b = N_b (1 - lambda - eps) - (1 + 1 / lambda) V_b,  clamped when A_b / 2 s^2 leaves [-2^29 - 2^22, 2^29 - 2^22]
    b64 = base.astype(np.float64)
    rms = float(np.sqrt(np.mean(b64 ** 2)))
    s = float(np.float32(min(float(np.abs(base).max()), 5.5 * rms)) / np.float32(127.0))
    lam = 1.4 * s / (np.sqrt(12.0) * float(np.float32(rms)))
    eps = (D / 8.0 + 16.0) * 2.0 ** -24
    bq = np.clip(np.rint(base[r] * (np.float32(1.0) / np.float32(s))), -127, 127).astype(np.float64)
    n_b, v_b = float((b64[r] ** 2).sum()), float(((b64[r] - s * bq) ** 2).sum())
    x_b = (n_b * (1.0 - lam - eps) - (1.0 + 1.0 / lam) * v_b) / (2.0 * s * s)
    print(f"rms {rms:.4f}, s {s:.5f}, lambda {lam:.5f}: A_b / 2s^2 = {x_b:.4g} (limit -2^29 - 2^22 = {-(2 ** 29 + 2 ** 22)})")
    assert x_b < -4.0 * 2 ** 29, x_b   # (far beyond the limit: no rounding of this restatement matters)
    q = np.concatenate([queries[:255], base[r:r + 1]], 0)
    rids, rd = oracle.brute_force(base, q, K, oracle.METRIC_L2_F32, n_threads=16)
    assert rids[255, 0] == r and rd[255, 0] == 0.0
    ids, dists, prof, st = _run(base, q[:255], K, rerank_stats=1)
    _same(ids, dists, rids[:255], rd[:255], (prof, st))
    assert prof["scan_kernel"] == I8F and prof["retries"] == 0, (prof, st)
    assert st["rerank_rows"] >= 255, st   # (the clamped row alone is one per query)
    ids, dists, prof, st = _run(base, q, K)
    print(f"with the query equal to the clamped row: retries {prof['retries']}, {prof['scan_kernel']}, {st}")
    _same(ids, dists, rids, rd, (prof, st))
    assert ids[255, 0] == r and dists[255, 0] == 0.0
