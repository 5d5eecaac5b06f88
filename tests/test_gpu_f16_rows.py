"""Brute force over IEEE binary16 rows (EXPANN_DTYPE_F16, dtype="f16"): every entry point must return, bit for bit,
what the reference's arithmetic gives on the exactly upcast rows -- the expected answers are the oracle's over
rows16.astype(np.float32), ids equal, distances equal as uint32 -- while the rows stay 2 bytes per element on the device.
Shapes are those at which test_gpu_any_dim.py and test_gpu_row_filter.py reach each path."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = np.uint64(2 ** 64 - 1)
N_BIG, M_BIG = 65_536, 97


def _rows16(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32).astype(np.float16)


def _gauss(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32)


def _engine(rows, metric="l2", dtype="f16", **opts):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(rows.shape[1], metric, dtype)
    eng.store_many_vectors(rows)
    eng.build()
    for name, val in opts.items():
        eng.set_option(name, val)
    eng.set_profiling(True)
    return eng


def _om(oracle, metric):
    return oracle.METRIC_L2_F32 if metric == "l2" else oracle.METRIC_IP_F32


def _ref(oracle, rows16, queries, k, metric="l2"):
    """THE reference: the oracle over the exactly upcast rows"""
    assert rows16.dtype == np.float16
    return oracle.brute_force(rows16.astype(np.float32), queries, k, _om(oracle, metric), n_threads=16)


def _same(got, want, what=""):
    ids, dists = got
    rids, rd = want
    assert np.array_equal(ids, rids), what
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32)), what


@functools.lru_cache(maxsize=None)
def _big(d):
    """rows and queries of the matrix-core cases at dim d (shared, never written to)"""
    rows, queries = _rows16(10 * d, N_BIG, d), _gauss(10 * d + 1, M_BIG, d)
    rows.setflags(write=False)
    queries.setflags(write=False)
    return rows, queries


_REFS = {}


def _big_ref(oracle, d, metric, k=100):
    key = (d, metric, k)
    if key not in _REFS:
        _REFS[key] = _ref(oracle, *_big(d), k, metric)
    return _REFS[key]


# 1. exact scan, small index -----------------------------------------------------------------------------------------
def _special_rows(rows):
    """d = 128: fp16 subnormals (integer multiples of 2^-24), +-65504 and exact zeros among the rows"""
    rng = np.random.default_rng(1)
    rows[0:40] = (rng.integers(-1023, 1024, (40, 128)) * 2.0 ** -24).astype(np.float16)
    rows[40:60] = (rng.choice([-65504.0, 65504.0], (20, 128))).astype(np.float16)
    rows[60:70] = 0
    assert (np.abs(rows[0:40].astype(np.float32)) < 2.0 ** -14).all() and np.isfinite(rows[40:60]).all()


def _special_queries(queries, rows):
    rng = np.random.default_rng(2)
    queries[0] = rng.integers(-1023, 1024, 128) * 2.0 ** -24 + 2.0 ** -26      # the subnormal rows' magnitude
    queries[1] = rows[45].astype(np.float32) * np.float32(0.9)                 # the +-65504 rows' magnitude
    queries[2] = rows[7].astype(np.float32) + np.float32(2.0 ** -27)           # next to one subnormal row


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", [16, 48, 128, 400, 4096])
def test_small_index_exact_scan(oracle, d, metric):
    n, m, k = 3000, 9, 10
    rows, queries = _rows16(d, n, d), _gauss(d + 1, m, d)
    if d == 128:
        _special_rows(rows)
        _special_queries(queries, rows)
    want = _ref(oracle, rows, queries, k, metric)
    if d == 128:
        # every expected distance is a normal fp32 number, and the special rows are among the answers
        assert np.isfinite(want[1]).all() and (np.abs(want[1]) >= np.finfo(np.float32).tiny).all()
        if metric == "l2":
            assert (want[0][0] < 70).all() and want[0][2][0] == 7 and want[0][1][0] == 45
        else:
            assert want[0][1][0] == 45 and (want[0][1][:5] >= 40).all() and (want[0][1][:5] < 60).all()
    eng = _engine(rows, metric)
    assert eng.get_stat("base_bytes") == n * d * 2
    assert eng.param_list()["dtype"] == "f16"
    got = eng.query_k_batch(queries, k)
    prof = eng.get_profile()
    eng.close()
    assert prof["scan_kernel"].startswith("scan_filter_f32_any") and "F16" in prof["scan_kernel"], prof
    _same(got, want)


def test_base_bytes_of_the_other_dtypes():
    from expann_amd import GpuBruteForceEngine
    for dtype, npdt, size in (("f32", np.float32, 4), ("u8", np.uint8, 1)):
        eng = GpuBruteForceEngine(128, "l2", dtype)
        assert eng.get_stat("base_bytes") == 0
        eng.store_many_vectors(np.ones((300, 128), npdt))
        assert eng.get_stat("base_bytes") == 0                     # staged, not on the device yet
        eng.build()
        assert eng.get_stat("base_bytes") == 300 * 128 * size
        eng.close()


def _nonfinite_case(metric):
    """a small index with a +inf, a -inf and (L2) a NaN element in three rows, past the first k rows"""
    n, d, m = 3000, 128, 9
    rows, queries = _rows16(77, n, d), _gauss(78, m, d)
    queries[:, 5] = np.abs(queries[:, 5]) + 0.5            # inner product: +inf * positive = +inf, score -inf, rank 0
    rows[100, 5] = np.inf
    rows[200, 5] = -np.inf
    if metric == "l2":                                     # (a NaN score's sign decides where it sorts under -dot: L2 only)
        rows[300, 9] = np.nan
    return rows, queries


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_rows_with_inf_and_nan_behave_as_in_an_f32_index(oracle, metric):
    """the header's sentence, on the exact scan and on score_ids: the oracle over the upcast rows, and the F32 index"""
    rows, queries = _nonfinite_case(metric)
    k = 10
    want = _ref(oracle, rows, queries, k, metric)
    if metric == "ip":
        assert (want[0][:, 0] == 100).all() and np.isneginf(want[1][:, 0]).all()
    assert np.isfinite(want[1][:, 1:]).all()
    ids = np.array([100, 200, 300, 7, 2999], np.uint64)
    out = {}
    for dtype, r in (("f16", rows), ("f32", rows.astype(np.float32))):
        eng = _engine(r, metric, dtype)
        out[dtype] = (eng.query_k_batch(queries, k), eng.score_ids(queries[0], ids))
        eng.close()
    _same(out["f16"][0], want, "oracle")
    _same(out["f16"][0], out["f32"][0], "f32 index")
    # score_ids keeps `score < cutoff`: never a NaN or a +inf score, always a -inf one
    rk, rs = oracle.filter_by_score(rows.astype(np.float32), queries[0], ids, float("inf"), _om(oracle, metric))
    assert list(rk) == ([7, 2999] if metric == "l2" else [100, 300, 7, 2999])
    for kept, sc in (out["f16"][1], out["f32"][1]):
        assert np.array_equal(kept, rk) and np.array_equal(sc.view(np.uint32), rs.view(np.uint32))


# 2. matrix-core filter, re-rank over the fp16 rows -----------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", [128, 256, 768, 208, 1536])
def test_gemm_size(oracle, d, metric):
    rows, queries = _big(d)
    rids, rd = _big_ref(oracle, d, metric)
    eng = _engine(rows, metric)
    assert eng.get_stat("base_bytes") == N_BIG * d * 2
    for k in (1, 10, 100):
        got = eng.query_k_batch(queries, k)
        prof = eng.get_profile()
        _same(got, (rids[:, :k], rd[:, :k]), k)
        assert prof["scan_kernel"].startswith("scan_gemm_f16"), prof
        assert prof["retries"] == 0, (k, prof)
    eng.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("k", [1000, 8192])
def test_long_lists_reach_the_sorting_select(oracle, k, metric):
    """all 97 queries (more than 64: the wave selects run first and leave the long lists to the sorting select),
    both metrics: the _Float16 re-rank of select_wave_kernel and of select_topk_kernel's bitonic path.  No retry at
    k = 1000 (the plan keeps at most max(2 k, cap / 6) rows per level); at k = 8192 = cap / 2 a retry is the data's
    luck, as for fp32 rows, and the kernel is asserted when there was none."""
    rows, queries = _big(128)
    rids, rd = _big_ref(oracle, 128, metric, 8192)
    eng = _engine(rows, metric)
    got = eng.query_k_batch(queries, k)
    prof = eng.get_profile()
    eng.close()
    print(k, metric, prof["scan_kernel"], "retries", prof["retries"])
    _same(got, (rids[:, :k], rd[:, :k]))
    if k == 1000:
        assert prof["retries"] == 0, prof
    if prof["retries"] == 0:
        assert prof["scan_kernel"].startswith("scan_gemm_f16"), prof


# 3. the same operands as the F32 index of the upcast rows -----------------------------------------------------------
@pytest.mark.parametrize("d", [128, 208])
def test_same_filter_operands_as_the_f32_index(oracle, d):
    rows, queries = _big(d)
    out = {}
    for dtype, r in (("f16", rows), ("f32", rows.astype(np.float32))):
        eng = _engine(r, "l2", dtype)
        got = eng.query_k_batch(queries, 10)
        out[dtype] = (got, eng.get_profile())
        eng.close()
    _same(out["f16"][0], out["f32"][0])
    assert out["f16"][1]["candidates"] == out["f32"][1]["candidates"] > 0, out
    assert out["f16"][1]["scan_kernel"] == out["f32"][1]["scan_kernel"]


# 4. integer-valued rows never take the uint8 shadow ---------------------------------------------------------------------
def test_integer_rows_do_not_take_the_uint8_shadow(oracle):
    rng = np.random.default_rng(255)
    rows = rng.integers(0, 256, (N_BIG, 128)).astype(np.float16)
    queries = rng.integers(0, 256, (M_BIG, 128)).astype(np.float32)
    eng = _engine(rows)
    got = eng.query_k_batch(queries, 10)
    prof = eng.get_profile()
    eng.close()
    assert "i8" not in prof["scan_kernel"].lower() and "u8" not in prof["scan_kernel"].lower(), prof
    _same(got, _ref(oracle, rows, queries, 10))


# 5. duplicates and fallbacks ------------------------------------------------------------------------------------------
def test_ties_duplicates_and_padding(oracle):
    d = 400
    rows = _rows16(7, 5000, d)
    rows[100:140] = rows[3]
    queries = _gauss(8, 6, d)
    queries[0] = rows[3]
    queries[1] = rows[4999]
    eng = _engine(rows)
    for k in (1, 50):
        _same(eng.query_k_batch(queries, k), _ref(oracle, rows, queries, k), k)
    eng.close()
    small = rows[:20].copy()
    eng = _engine(small)
    ids, dists = eng.query_k_batch(queries, 32)
    eng.close()
    assert (ids[:, 20:] == PAD).all() and np.isinf(dists[:, 20:]).all()
    _same((ids[:, :20], dists[:, :20]), _ref(oracle, small, queries, 20))


def test_queries_outside_the_fp16_range_fall_back(oracle):
    rows, queries = _big(128)
    queries = queries.copy()
    queries[5, 7] = 1.0e9
    eng = _engine(rows)
    got = eng.query_k_batch(queries, 10)
    prof = eng.get_profile()
    eng.close()
    assert prof["scan_kernel"].startswith("scan_filter_f32"), prof
    _same(got, _ref(oracle, rows, queries, 10))


@pytest.mark.parametrize("scan_kernel", [1, 3])
def test_forced_scan_kernels_are_exact(oracle, scan_kernel):
    """1 = the direct scan; 3 = bf16x3, which fp16 rows do not have: accepted, runs the exact direct scan"""
    rows, queries = _big(128)
    eng = _engine(rows, scan_kernel=scan_kernel)
    got = eng.query_k_batch(queries, 10)
    prof = eng.get_profile()
    eng.close()
    assert prof["scan_kernel"].startswith("scan_filter_f32_any"), prof
    rids, rd = _big_ref(oracle, 128, "l2")
    _same(got, (rids[:, :10], rd[:, :10]))


def test_shadow_and_int8_filter_options_are_accepted_and_ignored(oracle):
    rows, queries = _big(128)
    eng = _engine(rows, u8_exact=1, i8_filter=2)
    got = eng.query_k_batch(queries, 10)
    prof = eng.get_profile()
    eng.close()
    assert prof["scan_kernel"].startswith("scan_gemm_f16"), prof
    rids, rd = _big_ref(oracle, 128, "l2")
    _same(got, (rids[:, :10], rd[:, :10]))


# 6. few queries ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("m", [1, 4])
def test_few_queries(oracle, m, metric):
    rows, queries = _big(128)
    rids, rd = _big_ref(oracle, 128, metric)
    want = (rids[:m, :10], rd[:m, :10])
    eng = _engine(rows, metric)
    _same(eng.query_k_batch(queries[:m], 10), want, "latency mode")
    eng.set_option("latency_mode", 0)
    _same(eng.query_k_batch(queries[:m], 10), want, "plain copies")
    eng.close()


# 7. device rows, deferred searches --------------------------------------------------------------------------------------
def test_device_rows_and_deferred_searches(oracle):
    torch = pytest.importorskip("torch")
    from expann_amd import GpuBruteForceEngine
    rows, queries = _big(128)
    off, m, k = 10 ** 12, M_BIG, 10
    t_rows = torch.from_numpy(np.array(rows)).cuda()
    assert t_rows.dtype == torch.float16
    rids, rd = _big_ref(oracle, 128, "l2")
    want = (rids[:, :k] + np.uint64(off), rd[:, :k])
    eng = GpuBruteForceEngine(128, "l2", "f16")
    eng.set_base_device(t_rows.data_ptr(), N_BIG, off)
    assert eng.get_stat("base_bytes") == N_BIG * 128 * 2
    tq = torch.from_numpy(np.array(queries)).cuda()
    outs = [(torch.empty(m, k, dtype=torch.int64, device="cuda"), torch.empty(m, k, dtype=torch.float32, device="cuda"))
            for _ in range(4)]
    torch.cuda.synchronize()
    eng.search_device(tq.data_ptr(), m, k, outs[0][0].data_ptr(), outs[0][1].data_ptr(), 0)
    torch.cuda.synchronize()
    eng.set_option("async_search", 1)
    st = torch.cuda.Stream()
    for i, dd in outs[1:]:
        eng.search_device(tq.data_ptr(), m, k, i.data_ptr(), dd.data_ptr(), st.cuda_stream)
    eng.sync()
    torch.cuda.synchronize()
    eng.close()
    for n_out, (i, dd) in enumerate(outs):
        _same((i.cpu().numpy().view(np.uint64), dd.cpu().numpy()), want, n_out)


# 8. row filter ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filtered():
    n, d = 65_573, 128
    rows, queries = _rows16(4081, n, d), _gauss(4082, 300, d)
    eng = _engine(rows)
    yield rows, queries, eng
    eng.close()


def _expected_filtered(oracle, rows16, queries, k, allow):
    """as test_gpu_row_filter._expected: the oracle over the allowed rows only, ids mapped back"""
    idx = np.flatnonzero(allow)
    m = queries.shape[0]
    if idx.size == 0:
        return np.full((m, k), PAD, np.uint64), np.full((m, k), np.inf, np.float32)
    rids, rd = _ref(oracle, np.ascontiguousarray(rows16[idx]), queries, k)
    out = np.full(rids.shape, PAD, np.uint64)
    ok = rids != PAD
    out[ok] = idx[rids[ok].astype(np.int64)].astype(np.uint64)
    return out, rd


@pytest.mark.parametrize("which", ["0.5", "0.05", "100 rows", "none", "all"])
def test_row_filter(oracle, filtered, which):
    rows, queries, eng = filtered
    n = rows.shape[0]
    rs = np.random.RandomState(7)
    if which == "100 rows":
        allow = np.zeros(n, bool)
        allow[rs.choice(n, 100, replace=False)] = True
    elif which in ("none", "all"):
        allow = np.full(n, which == "all")
    else:
        allow = rs.rand(n) < float(which)
    eng.set_row_filter(allow)
    assert eng.get_stat("filter_active") == 1 and eng.get_stat("filter_rows") == int(allow.sum())
    eng.get_profile()
    got = eng.query_k_batch(queries, 10)
    prof = eng.get_profile()
    _same(got, _expected_filtered(oracle, rows, queries, 10, allow), which)
    if which in ("0.5", "0.05", "all"):
        assert prof["scan_kernel"].startswith("scan_gemm_f16") and prof["retries"] == 0, prof
    eng.set_row_filter(None)
    assert eng.get_stat("filter_active") == 0 and eng.get_stat("filter_rows") == n


# 9. score_ids -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", [128, 400])
def test_score_ids(oracle, d, metric):
    n = 6000
    rows = _rows16(d + 5, n, d)
    query = _gauss(d + 6, 1, d)[0]
    ids = np.random.default_rng(d).integers(0, n, 5000).astype(np.uint64)
    up, om = rows.astype(np.float32), _om(oracle, metric)
    _, all_sc = oracle.filter_by_score(up, query, ids, float("inf"), om)
    cutoff = float(np.median(all_sc))
    eng = _engine(rows, metric)
    for c in (float("inf"), cutoff):
        kept, sc = eng.score_ids(query, ids, c)
        rk, rs = oracle.filter_by_score(up, query, ids, c, om)
        assert np.array_equal(kept, rk)
        assert np.array_equal(sc.view(np.uint32), rs.view(np.uint32))
    assert 0 < rk.size < ids.size
    eng.close()


# 10. speculative thresholds ---------------------------------------------------------------------------------------------
def test_spec_rank(oracle):
    rows = _big(128)[0]
    queries = _gauss(1283, 300, 128)
    eng = _engine(rows, spec_rank=3)
    got = eng.query_k_batch(queries, 10)
    prof = eng.get_profile()
    st = {s: eng.get_stat(s) for s in ("redo_queries", "redo_overflows", "spec_rank")}
    eng.close()
    _same(got, _ref(oracle, rows, queries, 10))
    assert prof["retries"] == 0 and st["spec_rank"] == 3 and st["redo_overflows"] == 0, (prof, st)


# 11. sharded --------------------------------------------------------------------------------------------------------------
def test_sharded_in_process(oracle):
    from expann_amd import ShardedBruteForceEngine
    n, d, m, k = 20_011, 128, 150, 10
    rows, queries = _rows16(2011, n, d), _gauss(2012, m, d)
    rows[9_000:9_030] = rows[3]                  # exact ties across the shard boundaries
    queries[5] = rows[3]
    single = _engine(rows)
    want = single.query_k_batch(queries, k)
    single.close()
    eng = ShardedBruteForceEngine(d, "l2", "f16", devices=[0, 0, 0])
    eng.store_many_vectors(rows[:7_000])
    eng.store_many_vectors(rows[7_000:])
    eng.build()
    assert eng.size() == n and eng.shards() == 3 and eng.param_list()["dtype"] == "f16"
    got = eng.query_k_batch(queries, k)
    eng.close()
    _same(got, want)
    _same(got, _ref(oracle, rows, queries, k))


def test_sharded_rank_form_adopts_fp16_device_rows(oracle):
    """one rank, no communicator: the rank form's only way to receive rows is a device pointer -- here binary16"""
    torch = pytest.importorskip("torch")
    from expann_amd import ShardedBruteForceEngine
    rows, queries = _big(128)
    off, m, k = 1_000_000, M_BIG, 10
    t_rows = torch.from_numpy(np.array(rows)).cuda()
    tq = torch.from_numpy(np.array(queries)).cuda()
    eng = ShardedBruteForceEngine(128, "l2", "f16", device=0, rank=0, world=1)
    eng.set_shard_device(0, t_rows.data_ptr(), N_BIG, off)
    ids = torch.empty(m, k, dtype=torch.int64, device="cuda")
    dd = torch.empty(m, k, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.search_device(tq.data_ptr(), m, k, ids.data_ptr(), dd.data_ptr(), 0)
    eng.sync()
    torch.cuda.synchronize()
    eng.close()
    rids, rd = _big_ref(oracle, 128, "l2")
    _same((ids.cpu().numpy().view(np.uint64), dd.cpu().numpy()), (rids[:, :k] + np.uint64(off), rd[:, :k]))


# 12. the C++ surface --------------------------------------------------------------------------------------------------
def test_cpp_engine_rounds_float_rows_to_fp16(oracle, tmp_path):
    from expann_amd import _lib
    _lib.load()
    so = tmp_path / "f16_engine_hook.so"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "f16_engine_hook.cpp"), "-o", str(so),
                           "-L", libdir, "-lexpann_hip", "-Wl,-rpath," + libdir])
    hook = C.CDLL(str(so))
    hook.f16_engine_query.restype = C.c_int
    hook.f16_engine_query.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t,
                                      C.c_void_p, C.c_void_p]
    n, d, m, k = 3000, 128, 9, 10
    rows = _gauss(31, n, d)                      # float rows: the engine rounds them
    rows[5] *= 1.0e-6                            # (subnormal halves) ...
    rows[6] *= 1.0e5                             # ... and overflow to +-inf
    queries = _gauss(32, m, d)
    ids = np.empty((m, k), np.uint64)
    dists = np.empty((m, k), np.float32)
    assert hook.f16_engine_query(rows.ctypes.data, n, d, 0, queries.ctypes.data, m, k, ids.ctypes.data,
                                 dists.ctypes.data) == 0
    with np.errstate(over="ignore"):
        rows16 = rows.astype(np.float16)
    eng = _engine(rows16)
    want = eng.query_k_batch(queries, k)
    eng.close()
    _same((ids, dists), want)
    _same((ids, dists), _ref(oracle, rows16, queries, k))
