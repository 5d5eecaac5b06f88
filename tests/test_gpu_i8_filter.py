"""The int8 filter of fp32 L2 rows (expann_amd/csrc/scan_gemm_i8f.hpp): rows and queries quantised to int8
with one per-index scale, scanned on the int8 matrix cores with a rigorous slack, candidates re-scored
exactly in fp32.  Forced on (option i8_filter = 2) it must give the oracle's ids and distance bits on every
kind of data the bound has to survive; the auto planner must pick it above the crossover only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I8F = "scan_gemm_i8w<128,F32L2>"
F16 = "scan_gemm_f16x<128, false>"


@pytest.fixture(scope="module")
def gpu():
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_device_count() >= 1, "these tests need a HIP device"
    return L


def _engine(base, i8_filter=2, **opts):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(base.shape[1], "l2")
    eng.store_many_vectors(base)
    eng.build()
    eng.set_option("i8_filter", i8_filter)
    for name, val in opts.items():
        eng.set_option(name, val)
    eng.set_profiling(True)
    return eng


def _check_forced(oracle, base, queries, k, path="i8f", **opts):
    """forced int8 filter: ids and distance bits equal the oracle's, and the path the test is about ran --
    "i8f": the int8 scan produced the results, no retry; "fallback": its lists overflowed (or the queries left
    the fp16 range the prelude needs) and a retry on the exact kernels of the other forms produced them (the
    intended behaviour where the one int8 scale cannot separate the rows)"""
    eng = _engine(base, 2, **opts)
    ids, dists = eng.query_k_batch(queries, k)
    prof = eng.get_profile()
    eng.close()
    rids, rd = oracle.brute_force(base, queries, k, oracle.METRIC_L2_F32, n_threads=16)
    assert np.array_equal(ids, rids), prof
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32)), prof
    if path == "i8f":
        assert prof["scan_kernel"] == I8F and prof["retries"] == 0, prof
    else:
        assert prof["scan_kernel"] != I8F and prof["retries"] >= 1, prof
    return prof


def _iid(rng, n, m, d=128):
    return rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)


@pytest.mark.parametrize("n,m,k", [(65536, 256, 10), (70001, 300, 1), (100003, 513, 10), (65600, 97, 100)])
def test_iid_rows(gpu, oracle, n, m, k):
    rng = np.random.RandomState(n + m + k)
    base, queries = _iid(rng, n, m)
    _check_forced(oracle, base, queries, k)


def test_row_magnitudes_over_24_decades_fall_back(gpu, oracle):
    """rows and queries spread over 24 decades: the one scale is set by the largest rows, every smaller row and
    query quantises to 0 and passes the filter -- the lists overflow and the batch is redone on the fp16 form"""
    rng = np.random.RandomState(7)
    n, m = 66000, 200
    base, queries = _iid(rng, n, m)
    base *= (10.0 ** rng.uniform(-12, 12, size=(n, 1))).astype(np.float32)
    queries *= (10.0 ** rng.uniform(-12, 12, size=(m, 1))).astype(np.float32)
    queries[:50] = base[rng.randint(0, n, 50)] * np.float32(1.0 + 1e-6)   # queries among the rows' scales
    _check_forced(oracle, base, queries, 10, path="fallback")


def test_tiny_rows_and_queries_in_an_ordinary_index(gpu, oracle):
    """0.5 % of the rows and 10 % of the queries at magnitudes 1e-12 .. 1: they quantise to (nearly) 0, their
    error is their whole value, and the int8 filter still serves the batch"""
    rng = np.random.RandomState(8)
    n, m = 66000, 200
    base, queries = _iid(rng, n, m)
    tiny = rng.randint(0, n, n // 200)
    base[tiny] *= (10.0 ** rng.uniform(-12, 0, size=(len(tiny), 1))).astype(np.float32)
    queries[:20] *= (10.0 ** rng.uniform(-12, 0, size=(20, 1))).astype(np.float32)
    queries[20:30] = base[tiny[:10]] * np.float32(1.0 + 1e-5)
    _check_forced(oracle, base, queries, 10)


def test_clipped_outliers_and_queries_just_outside_the_clip_range(gpu, oracle):
    """rows with components far beyond the clip (their integer row term is clamped: key -inf, always re-scored)
    and queries with one component just beyond it: the int8 filter serves the batch"""
    rng = np.random.RandomState(11)
    n, m = 40000, 300
    base, queries = _iid(rng, n, m)
    rows = rng.choice(n, 210, replace=False)
    base[rows[10:], rng.randint(0, 128, 200)] = rng.choice([-1, 1], 200) * rng.uniform(6, 200, 200)  # clipped components
    base[rows[:10]] *= 50.0                                     # whole rows far out: their row term is clamped
    # (both on the SAME rows -- components up to 10 000 -- would set the rms, hence the one scale, ~5 x too
    # coarse for every other row: that index overflows the lists and falls back, as the 24-decade case)
    rms = float(np.sqrt(np.mean(base.astype(np.float64) ** 2)))
    queries[:40, 7] = np.float32(5.6 * rms)                                                        # just beyond the clip
    _check_forced(oracle, base, queries, 10)


def test_queries_far_beyond_the_clip_fall_back(gpu, oracle):
    """queries 30 x the rows' scale: their quantisation error covers every row, the lists overflow, and the
    retry on the fp16 form gives the exact results"""
    rng = np.random.RandomState(12)
    n, m = 40000, 100
    base, queries = _iid(rng, n, m)
    queries[:30] *= 30.0
    _check_forced(oracle, base, queries, 10, path="fallback")


def test_duplicates_and_near_ties_at_the_kth(gpu, oracle):
    rng = np.random.RandomState(13)
    n, m, k = 70000, 128, 10
    base, queries = _iid(rng, n, m)
    base[1000:1040] = base[5]                        # 40 copies: ties across the k-th
    queries[:16] = base[5] + np.float32(1e-3) * queries[:16]
    for j in range(20):                              # rows one ulp apart around one query's k-th
        base[2000 + j] = np.nextafter(base[3000], np.float32(np.inf)) if j % 2 else base[3000]
    queries[16:32] = base[3000] + np.float32(0.05) * queries[16:32]
    _check_forced(oracle, base, queries, k)


@pytest.mark.parametrize("k", [1, 10, 100])
def test_clustered_rows(gpu, oracle, k):
    rng = np.random.RandomState(17 + k)
    n, m, c = 72000, 260, 60
    centres = rng.standard_normal((c, 128)).astype(np.float32)
    base = (centres[np.arange(n) * c // n] + 0.3 * rng.standard_normal((n, 128))).astype(np.float32)
    queries = (centres[rng.randint(0, c, m)] + 0.3 * rng.standard_normal((m, 128))).astype(np.float32)
    _check_forced(oracle, base, queries, k)


def test_seeded_sweep(gpu, oracle):
    """~200 random cases: sizes off the tile grid, k from 1 to 128, offsets, scales, clusters, spikes.  Every
    case is exact, and each ran one of the two paths: the int8 filter without a retry, or its overflow and the
    fp16 form; most of them the first"""
    paths = {"i8f": 0, "fallback": 0}
    for seed in range(200):
        rng = np.random.RandomState(90000 + seed)
        n = int(rng.randint(33000, 90000))
        m = int(rng.randint(1, 320))
        k = int(rng.choice([1, 2, 5, 10, 16, 32, 64, 100, 128]))
        base, queries = _iid(rng, n, m)
        kind = seed % 5
        if kind == 1:
            scale = np.float32(10.0 ** rng.uniform(-6, 6))
            base *= scale
            queries *= scale
            base += np.float32(rng.uniform(-3, 3)) * scale
            queries += np.float32(rng.uniform(-3, 3)) * scale
        elif kind == 2:
            c = int(rng.randint(2, 200))
            centres = rng.standard_normal((c, 128)).astype(np.float32)
            base = (centres[rng.randint(0, c, n)] + 0.2 * base).astype(np.float32)
            queries = (centres[rng.randint(0, c, m)] + 0.2 * queries).astype(np.float32)
        elif kind == 3:
            sp = rng.randint(0, n, 50)
            base[sp, rng.randint(0, 128, 50)] *= np.float32(20.0)
            queries[: max(1, m // 4)] *= np.float32(1.5)
        elif kind == 4:
            base[rng.randint(0, n, 64)] = base[0]
            queries[: max(1, m // 3)] = base[0] + np.float32(1e-4) * queries[: max(1, m // 3)]
        eng = _engine(base, 2)
        ids, dists = eng.query_k_batch(queries, k)
        prof = eng.get_profile()
        kernel = prof["scan_kernel"]
        eng.close()
        rids, rd = oracle.brute_force(base, queries, k, oracle.METRIC_L2_F32, n_threads=16)
        assert np.array_equal(ids, rids), (seed, n, m, k, kind, kernel)
        assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32)), (seed, n, m, k, kind, kernel)
        if kernel == I8F and prof["retries"] == 0:
            paths["i8f"] += 1
        else:
            assert kernel != I8F and prof["retries"] >= 1, (seed, n, m, k, kind, prof)
            paths["fallback"] += 1
    assert paths["i8f"] >= 150, paths


def test_auto_above_the_crossover_runs_the_int8_filter(gpu, oracle):
    rng = np.random.RandomState(23)
    n, m, k = 1 << 20, 4096, 10
    base, queries = _iid(rng, n, m)
    eng = _engine(base, 1)
    ids, dists = eng.query_k_batch(queries, k)
    prof = eng.get_profile()
    assert prof["scan_kernel"] == I8F and prof["retries"] == 0, prof
    eng.set_option("i8_filter", 0)                    # the fp16 form on the same engine: identical results
    ids0, d0 = eng.query_k_batch(queries, k)
    assert eng.get_profile()["scan_kernel"] == "scan_gemm_f16x<128, false>"
    eng.close()
    assert np.array_equal(ids, ids0)
    assert np.array_equal(dists.view(np.uint32), d0.view(np.uint32))
    rids, rd = oracle.brute_force(base, queries[:48], k, oracle.METRIC_L2_F32, n_threads=16)
    assert np.array_equal(ids[:48], rids)
    assert np.array_equal(dists[:48].view(np.uint32), rd.view(np.uint32))


@pytest.mark.parametrize("n,m,k", [(300000, 2000, 10), (200000, 300, 10), (131072, 700, 10), (70000, 140, 10),
                                   (65536, 97, 10), (65536, 40, 10), (1 << 20, 2048, 10), (1 << 20, 4096, 32)])
def test_auto_below_the_crossover_keeps_the_fp16_form(gpu, n, m, k):
    rng = np.random.RandomState(29)
    base, queries = _iid(rng, n, m)
    eng = _engine(base, 1)
    eng.query_k_batch(queries, k)
    assert eng.get_profile()["scan_kernel"] == "scan_gemm_f16x<128, false>", eng.get_profile()
    eng.close()


def test_overflow_retries_on_the_fp16_form(gpu, oracle):
    rng = np.random.RandomState(31)
    n, m, k = 100000, 300, 10
    base, queries = _iid(rng, n, m)
    _check_forced(oracle, base, queries, k, path="fallback", cand_capacity=64)


def test_option_and_environment_switch(gpu):
    import os
    import subprocess
    import sys
    rng = np.random.RandomState(37)
    base, queries = _iid(rng, 65536, 64)
    eng = _engine(base, 0)
    eng.query_k_batch(queries, 10)
    assert eng.get_profile()["scan_kernel"].startswith("scan_gemm_f16x"), eng.get_profile()
    eng.set_option("i8_filter", 2)
    eng.query_k_batch(queries, 10)
    assert eng.get_profile()["scan_kernel"] == I8F, eng.get_profile()
    eng.close()
    # EXPANN_I8_FILTER sets the option's starting value of every engine the process creates
    code = ("import numpy as np; from expann_amd import GpuBruteForceEngine as E; r = np.random.RandomState(1); "
            "b = r.standard_normal((65536, 128)).astype(np.float32); e = E(128, 'l2'); e.store_many_vectors(b); "
            "e.build(); e.set_profiling(True); e.query_k_batch(b[:64].copy(), 10); print(e.get_profile()['scan_kernel'])")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, EXPANN_I8_FILTER="2"), cwd=root,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == I8F, out.stdout


def test_auto_turns_itself_off_on_tightly_clustered_rows(gpu, oracle):
    """rows in tight clusters give the int8 filter lists far longer than on iid rows (i8f_cand_limit): after one
    such search the auto planner keeps the index on the fp16 form; results are exact either way"""
    rng = np.random.RandomState(41)
    n, m, k, c = 1 << 20, 4096, 10, 1000
    centres = rng.standard_normal((c, 128)).astype(np.float32)
    base = (centres[np.arange(n) * c // n] + 0.3 * rng.standard_normal((n, 128))).astype(np.float32)
    queries = (centres[rng.randint(0, c, m)] + 0.3 * rng.standard_normal((m, 128))).astype(np.float32)
    eng = _engine(base, 1)
    ids, dists = eng.query_k_batch(queries, k)
    first = eng.get_profile()
    ids2, d2 = eng.query_k_batch(queries, k)
    second = eng.get_profile()
    eng.close()
    assert first["scan_kernel"] == I8F, first
    assert second["scan_kernel"] == "scan_gemm_f16x<128, false>", second
    assert np.array_equal(ids, ids2) and np.array_equal(dists.view(np.uint32), d2.view(np.uint32))
    rids, rd = oracle.brute_force(base, queries[:64], k, oracle.METRIC_L2_F32, n_threads=16)
    assert np.array_equal(ids[:64], rids)
    assert np.array_equal(dists[:64].view(np.uint32), rd.view(np.uint32))
