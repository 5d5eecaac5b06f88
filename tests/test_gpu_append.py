"""Appending rows to a built brute-force index (expann_append, expann_append_device, expann_reserve).

THE APPEND RULE: after an append every entry point answers, bit for bit, as a fresh handle built from all the rows
answers.  Every comparison here is exact -- ids equal, distances equal as uint32 patterns -- against the oracle over
the concatenated rows AND against a fresh engine over the same rows; "copies_digest" shows that the fp16 copy an
append extended in place IS the one the fresh engine built (sound row terms, not merely lucky ones).
m = 130 queries and k = 10 unless a case says otherwise; the row with the global max |v| sits in the initial part
unless the case is about the scale."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, K = 130, 10
F16X = "scan_gemm_f16x"
I8F = "scan_gemm_i8w<128,F32L2>"
PAD = np.uint64(2 ** 64 - 1)


@pytest.fixture(scope="module")
def gpu():
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_device_count() >= 1, "these tests need a HIP device"
    return L


def _engine(rows, metric="l2", dtype="f32", opts=(), reserve=0):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(rows.shape[1], metric, dtype)
    for name, val in opts:
        eng.set_option(name, val)
    if reserve:
        eng.reserve(reserve)
    eng.store_many_vectors(rows)
    eng.build()
    eng.set_profiling(True)
    return eng


def _same(got, want, note=None):
    ids, dists = got
    rids, rd = want
    assert np.array_equal(ids, rids), note
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32)), note


def _rows(seed, n, d, m=M, scale=1.0):
    """n rows and m queries; the row with the largest |v| is row 0, so that it lies in every initial part"""
    rng = np.random.RandomState(seed)
    rows = (rng.standard_normal((n, d)) * scale).astype(np.float32)
    queries = (rng.standard_normal((m, d)) * scale).astype(np.float32)
    top = int(np.argmax(np.abs(rows).max(axis=1)))
    rows[[0, top]] = rows[[top, 0]]
    return rows, queries


def _stats(eng, *names):
    return {n: eng.get_stat(n) for n in names}


def _append_in_steps(oracle, rows, queries, n0, steps, metric="l2", dtype="f32", opts=(), warm=False, ometric=None,
                     kernel=None):
    """build on rows[:n0], append the steps one by one, search == oracle of the rows so far after each; at the end
    the digest is the fresh engine's.  Returns (appended engine, fresh engine, digest before the first append)."""
    ometric = oracle.METRIC_L2_F32 if ometric is None else ometric
    seen = rows.astype(np.float16).astype(np.float32) if dtype == "f16" else rows
    eng = _engine(rows[:n0], metric, dtype, opts)
    if warm:  # (the fp16 copy is not made at build under a forced "scan_kernel": the first search makes it)
        eng.query_k_batch(queries, K)
    d0 = eng.get_stat("copies_digest")
    n = n0
    for s in steps:
        eng.append(rows[n:n + s])
        n += s
        assert eng.size() == n
        _same(eng.query_k_batch(queries, K), oracle.brute_force(seen[:n], queries, K, ometric, n_threads=16), (n0, s))
    assert n == rows.shape[0]
    prof = eng.get_profile()
    if kernel:
        assert prof["scan_kernel"].startswith(kernel), prof
    fresh = _engine(rows, metric, dtype, opts)
    _same(fresh.query_k_batch(queries, K), eng.query_k_batch(queries, K))
    return eng, fresh, d0


# ---- 1. tile edges ---------------------------------------------------------------------------------------------
def test_tile_edges_d128(gpu, oracle):
    steps = [1, 63, 64, 65, 200, 1000]
    n0 = 4500
    rows, queries = _rows(1, n0 + sum(steps), 128)
    eng, fresh, d0 = _append_in_steps(oracle, rows, queries, n0, steps, kernel=F16X)
    st = _stats(eng, "append_calls", "append_rows", "append_extends", "append_rebuilds", "base_bytes", "copies_digest")
    fd = fresh.get_stat("copies_digest")
    n = eng.size()
    eng.close()
    fresh.close()
    assert st["append_extends"] == 6 and st["append_rebuilds"] == 0 and st["append_calls"] == 6, st
    assert st["append_rows"] == sum(steps) and n == rows.shape[0] and st["base_bytes"] == n * 128 * 4, st
    assert st["copies_digest"] == fd and fd != 0 and d0 != 0 and st["copies_digest"] != d0, (st, fd, d0)


# ---- 2. the scale ----------------------------------------------------------------------------------------------
def test_scale_extend_then_rebuild(gpu, oracle):
    rng = np.random.RandomState(2)
    n0 = 4500
    rows = np.clip(rng.standard_normal((n0 + 2, 128)) * 0.4, -1.4, 1.4).astype(np.float32)
    queries = (rng.standard_normal((M, 128)) * 0.4).astype(np.float32)
    rows[0, 5] = 1.5      # the initial max |v|: scale 2^14
    rows[n0, 7] = -1.9    # still 2^14: extend
    rows[n0 + 1, 9] = 2.5  # 2^13: the copy is dropped and made again
    eng = _engine(rows[:n0])
    for n, want in ((n0 + 1, (1, 0)), (n0 + 2, (1, 1))):
        eng.append(rows[n - 1:n])
        _same(eng.query_k_batch(queries, K), oracle.brute_force(rows[:n], queries, K, n_threads=16), n)
        st = _stats(eng, "append_extends", "append_rebuilds", "copies_digest")
        fresh = _engine(rows[:n])
        fd = fresh.get_stat("copies_digest")
        fresh.close()
        assert (st["append_extends"], st["append_rebuilds"]) == want, st
        assert st["copies_digest"] == fd and fd != 0, (n, st, fd)
    eng.close()


# ---- 3. run-time dim, and the w8 geometry --------------------------------------------------------------------
def test_runtime_dim_144(gpu, oracle):
    steps = [100, 28, 1]
    n0 = 4200
    rows, queries = _rows(3, n0 + sum(steps), 144)
    eng, fresh, _ = _append_in_steps(oracle, rows, queries, n0, steps, opts=(("scan_kernel", 4),), warm=True,
                                     kernel="scan_gemm_f16kl")
    st = _stats(eng, "append_extends", "append_rebuilds", "copies_digest")
    fd = fresh.get_stat("copies_digest")
    eng.close()
    fresh.close()
    assert st["append_extends"] == 3 and st["append_rebuilds"] == 0, st
    assert st["copies_digest"] == fd and fd != 0, (st, fd)


def test_w8_geometry_d256(gpu, oracle):
    n0 = 4500
    rows, queries = _rows(4, n0 + 77, 256)
    eng, fresh, _ = _append_in_steps(oracle, rows, queries, n0, [77], kernel="scan_gemm_f16y")
    st = _stats(eng, "append_extends", "copies_digest")
    fd = fresh.get_stat("copies_digest")
    eng.close()
    fresh.close()
    assert st["append_extends"] == 1 and st["copies_digest"] == fd and fd != 0, (st, fd)


# ---- 4. inner product: max ||b||^2 grows -----------------------------------------------------------------------
def test_inner_product_larger_norms(gpu, oracle):
    rng = np.random.RandomState(5)
    n0, n1 = 4500, 300
    init = (rng.standard_normal((n0, 128)) * 0.25).astype(np.float32)
    init[0] = 0.0
    init[0, 3] = 3.5  # the global max |v|, in the initial part
    top = float(np.sqrt((init.astype(np.float64) ** 2).sum(axis=1).max()))
    new = rng.standard_normal((n1, 128))
    new = (new / np.sqrt((new ** 2).sum(axis=1, keepdims=True)) * (2.0 * top)).astype(np.float32)
    assert np.abs(new).max() < 3.5  # (twice the norm of any initial row, yet no new maximum: the scale stays)
    rows = np.concatenate([init, new])
    queries = rng.standard_normal((M, 128)).astype(np.float32)
    queries[::2] *= np.float32(1e-3)
    eng, fresh, _ = _append_in_steps(oracle, rows, queries, n0, [n1], metric="ip", ometric=oracle.METRIC_IP_F32, kernel=F16X)
    st = _stats(eng, "append_extends", "append_rebuilds", "copies_digest")
    fd = fresh.get_stat("copies_digest")
    eng.close()
    fresh.close()
    assert st["append_extends"] == 1 and st["append_rebuilds"] == 0, st
    assert st["copies_digest"] == fd and fd != 0, (st, fd)


# ---- 5. binary16 rows ------------------------------------------------------------------------------------------
def test_f16_rows(gpu, oracle):
    steps = [65, 700]
    n0 = 4500
    rows, queries = _rows(6, n0 + sum(steps), 128)
    rows = rows.astype(np.float16).astype(np.float32)
    eng, fresh, d0 = _append_in_steps(oracle, rows, queries, n0, steps, dtype="f16", kernel=F16X)
    st = _stats(eng, "append_extends", "append_rebuilds", "base_bytes", "copies_digest")
    fd = fresh.get_stat("copies_digest")
    eng.close()
    fresh.close()
    assert st["append_extends"] == 2 and st["append_rebuilds"] == 0 and st["base_bytes"] == rows.shape[0] * 128 * 2, st
    assert st["copies_digest"] == fd and fd != 0 and fd != d0, (st, fd, d0)


# ---- 6. the int8 filter is rebuilt -----------------------------------------------------------------------------
def test_int8_filter_runs_again_after_an_append(gpu, oracle):
    n0, n1 = 33000, 1000
    rows, queries = _rows(7, n0 + n1, 128)
    eng = _engine(rows[:n0], opts=(("i8_filter", 2),))
    _same(eng.query_k_batch(queries, K), oracle.brute_force(rows[:n0], queries, K, n_threads=16))
    p0 = eng.get_profile()
    eng.append(rows[n0:])
    _same(eng.query_k_batch(queries, K), oracle.brute_force(rows, queries, K, n_threads=16))
    p1 = eng.get_profile()
    eng.close()
    assert p0["scan_kernel"] == I8F, p0
    assert p1["scan_kernel"] == I8F, p1  # (its copy was dropped by the append and made again by this search)


# ---- 7. crossing the planner's sizes -----------------------------------------------------------------------------
def test_crossing_65536_rows(gpu, oracle):
    n0, n1 = 4500, 61500
    rows, queries = _rows(8, n0 + n1, 128)
    eng = _engine(rows[:n0])
    eng.query_k_batch(queries, K)
    eng.append(rows[n0:])
    for k in (10, 100):
        _same(eng.query_k_batch(queries, k), oracle.brute_force(rows, queries, k, n_threads=16), k)
    st = _stats(eng, "append_extends", "base_capacity_rows")
    eng.close()
    assert st["append_extends"] == 1 and st["base_capacity_rows"] >= n0 + n1, st


# ---- 8. 8-bit rows ---------------------------------------------------------------------------------------------
def test_u8_rows(gpu, oracle):
    rng = np.random.RandomState(9)
    n0, n1 = 3000, 500
    rows = rng.randint(0, 256, size=(n0 + n1, 128)).astype(np.uint8)
    queries = rng.randint(0, 256, size=(M, 128)).astype(np.float32)
    eng = _engine(rows[:n0], dtype="u8")
    _same(eng.query_k_batch(queries, K), oracle.brute_force(rows[:n0], queries, K, oracle.METRIC_L2_U8, n_threads=16))
    eng.append(rows[n0:])
    _same(eng.query_k_batch(queries, K), oracle.brute_force(rows, queries, K, oracle.METRIC_L2_U8, n_threads=16))
    st = _stats(eng, "append_extends", "append_rebuilds", "append_rows", "base_bytes", "copies_digest")
    eng.close()
    assert st == dict(append_extends=0, append_rebuilds=0, append_rows=n1, base_bytes=(n0 + n1) * 128, copies_digest=0), st


def test_i8_rows_inner_product(gpu, oracle):
    rng = np.random.RandomState(10)
    n0, n1 = 3000, 500
    rows = rng.randint(-127, 128, size=(n0 + n1, 128)).astype(np.int8)
    queries = rng.randint(-127, 128, size=(M, 128)).astype(np.int8)
    eng = _engine(rows[:n0], metric="ip", dtype="i8")
    _same(eng.query_k_batch(queries, K), oracle.brute_force(rows[:n0], queries, K, oracle.METRIC_IP_I8, n_threads=16))
    eng.append(rows[n0:])
    _same(eng.query_k_batch(queries, K), oracle.brute_force(rows, queries, K, oracle.METRIC_IP_I8, n_threads=16))
    st = _stats(eng, "append_extends", "append_rebuilds")
    eng.close()
    assert st == dict(append_extends=0, append_rebuilds=0), st


@pytest.mark.parametrize("metric,oname", [("l2", "METRIC_L2_I8"), ("ip", "METRIC_IP_I8")])
def test_i8_rows_on_the_matrix_cores_across_reserve_and_append(gpu, oracle, metric, oname):
    """65 536 int8 rows (whole 64-row tiles, from 96 queries on): the per-wave hit-queue form serves, and its int8
    operand IS the base (no copy: nothing to pad, nothing to map).  A reserve moves the base and forgets nothing, so
    that alias has to follow it; an append drops the form's row terms, which the next search makes again."""
    rng = np.random.RandomState(18)
    n0, n1 = 65536, 64
    rows = rng.randint(-127, 128, size=(n0 + n1, 128)).astype(np.int8)
    queries = rng.randint(-127, 128, size=(M, 128)).astype(np.int8)
    om = getattr(oracle, oname)
    want0 = oracle.brute_force(rows[:n0], queries, K, om, n_threads=16)
    eng = _engine(rows[:n0], metric=metric, dtype="i8")
    _same(eng.query_k_batch(queries, K), want0)
    p0 = eng.get_profile()
    eng.reserve(100000)
    r = _stats(eng, "base_reallocs", "base_capacity_rows")
    _same(eng.query_k_batch(queries, K), want0, "after the reserve")
    p1 = eng.get_profile()
    eng.append(rows[n0:])
    _same(eng.query_k_batch(queries, K), oracle.brute_force(rows, queries, K, om, n_threads=16), "after the append")
    p2 = eng.get_profile()
    st = _stats(eng, "base_reallocs", "append_extends", "append_rebuilds", "copies_digest")
    eng.close()
    for p in (p0, p1, p2):
        assert p["scan_kernel"].startswith("scan_gemm_i8w"), p
    assert r == dict(base_reallocs=1, base_capacity_rows=100000), r
    assert st == dict(base_reallocs=1, append_extends=0, append_rebuilds=0, copies_digest=0), st


# ---- 9. filter and groups are cleared --------------------------------------------------------------------------
def test_filter_and_groups_are_cleared(gpu, oracle):
    n0, n1 = 4500, 100
    rows, queries = _rows(11, n0 + n1, 128)
    rng = np.random.RandomState(12)
    eng = _engine(rows[:n0])
    eng.set_row_filter(rng.rand(n0) < 0.3)
    eng.set_row_groups(rng.randint(0, 7, n0).astype(np.uint32))
    assert _stats(eng, "filter_active", "groups_active") == dict(filter_active=1, groups_active=1)
    eng.append(rows[n0:])
    assert _stats(eng, "filter_active", "groups_active", "filter_rows") == dict(filter_active=0, groups_active=0,
                                                                             filter_rows=n0 + n1)
    _same(eng.query_k_batch(queries, K), oracle.brute_force(rows, queries, K, n_threads=16))
    allow = np.zeros(n0 + n1, dtype=bool)
    allow[n0 + 3] = True
    eng.set_row_filter(allow)
    ids, dists = eng.query_k_batch(queries, K)
    rids, rd = oracle.brute_force(rows[n0 + 3:n0 + 4], queries, K, n_threads=16)
    eng.close()
    assert np.all(ids[:, 0] == n0 + 3) and np.all(ids[:, 1:] == PAD)
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32))


# ---- 10. the other entry points ----------------------------------------------------------------------------------
def test_other_entry_points_after_an_append(gpu, oracle):
    import torch
    n0, n1 = 4500, 700
    rows, queries = _rows(13, n0 + n1, 128)
    old_ref = oracle.brute_force(rows[:n0], queries, K, n_threads=16)
    ref20 = oracle.brute_force(rows, queries, 20, n_threads=16)
    eng = _engine(rows[:n0])
    # a deferred search issued BEFORE the append answers over the old rows
    tq = torch.from_numpy(queries).cuda()
    tid = torch.empty(M, K, dtype=torch.int64, device="cuda")
    td = torch.empty(M, K, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.set_option("async_search", 1)
    eng.search_device(tq.data_ptr(), M, K, tid.data_ptr(), td.data_ptr(), st.cuda_stream)
    eng.append(rows[n0:])
    eng.sync()
    torch.cuda.synchronize()
    eng.set_option("async_search", 0)
    _same((tid.cpu().numpy().astype(np.uint64), td.cpu().numpy()), old_ref)
    # score_ids with ids of appended rows
    ids = np.concatenate([np.arange(n0 - 5, n0 + 40), [n0 + n1 - 1, 0]]).astype(np.uint64)
    cutoff = float(np.median(ref20[1][0]) * 4)
    kept, sc = eng.score_ids(queries[0], ids, cutoff)
    rkept, rsc = oracle.filter_by_score(rows, queries[0], ids, cutoff)
    assert np.array_equal(kept, rkept) and np.array_equal(sc.view(np.uint32), rsc.view(np.uint32))
    assert (kept >= n0).any()
    # range search with each query's exact 10th distance as its radius: the counts include appended rows
    radii = ref20[1][:, K - 1].copy()
    want_counts = (ref20[1] <= radii[:, None]).sum(axis=1).astype(np.uint32)
    rids, rdists, counts = eng.range_search(queries, radii, K)
    eng.close()
    assert np.array_equal(counts, want_counts) and (want_counts < 20).all()
    _same((rids, rdists), (ref20[0][:, :K], ref20[1][:, :K]))
    assert (ref20[0][:, :K] >= n0).any()  # (appended rows are among the answers)


# ---- 11. reserve -------------------------------------------------------------------------------------------------
def test_reserve(gpu, oracle):
    n0, steps = 4500, 64
    rows, queries = _rows(14, n0 + steps * 100, 128)
    want = oracle.brute_force(rows, queries, K, n_threads=16)
    for reserve in (12000, 0):
        eng = _engine(rows[:n0])
        if reserve:
            eng.reserve(reserve)
        r0 = _stats(eng, "base_reallocs", "base_capacity_rows")
        for i in range(steps):
            eng.append(rows[n0 + 100 * i:n0 + 100 * (i + 1)])
        r1 = _stats(eng, "base_reallocs", "base_capacity_rows", "append_extends")
        _same(eng.query_k_batch(queries, K), want, reserve)
        fresh_digest = None
        if reserve:
            fresh = _engine(rows)
            fresh_digest = fresh.get_stat("copies_digest")
            fresh.close()
            assert eng.get_stat("copies_digest") == fresh_digest != 0
        eng.close()
        assert r1["append_extends"] == steps, r1
        if reserve:
            assert r0 == dict(base_reallocs=1, base_capacity_rows=12000), r0
            assert r1["base_reallocs"] == 1 and r1["base_capacity_rows"] == 12000, r1
        else:
            assert r0 == dict(base_reallocs=0, base_capacity_rows=n0), r0
            assert 1 <= r1["base_reallocs"] <= 6 and r1["base_capacity_rows"] >= n0 + steps * 100, r1
    # a reserve before build() is honoured by build()
    eng = _engine(rows[:n0], reserve=9000)
    r = _stats(eng, "base_capacity_rows", "base_reallocs")
    eng.append(rows[n0:n0 + 4500])
    r2 = _stats(eng, "base_capacity_rows", "base_reallocs", "append_extends")
    _same(eng.query_k_batch(queries, K), oracle.brute_force(rows[:n0 + 4500], queries, K, n_threads=16))
    eng.close()
    assert r == dict(base_capacity_rows=9000, base_reallocs=0), r
    assert r2 == dict(base_capacity_rows=9000, base_reallocs=0, append_extends=1), r2


# ---- 12. rows from device memory, on a side stream -----------------------------------------------------------
def test_append_device_equals_the_host_append(gpu, oracle):
    import torch
    n0, n1 = 4500, 333
    rows, queries = _rows(15, n0 + n1, 128)
    host = _engine(rows[:n0])
    host.append(rows[n0:])
    dev = _engine(rows[:n0])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = torch.from_numpy(rows[n0:]).cuda()
        dev.append_device(t.data_ptr(), n1, stream=st.cuda_stream)
        t.zero_()  # (the rows were copied: the caller may reuse its buffer on return)
    torch.cuda.synchronize()
    want = oracle.brute_force(rows, queries, K, n_threads=16)
    _same(dev.query_k_batch(queries, K), want)
    _same(host.query_k_batch(queries, K), want)
    ds = _stats(dev, "append_extends", "append_rows", "copies_digest")
    hs = _stats(host, "append_extends", "append_rows", "copies_digest")
    dev.close()
    host.close()
    assert ds == hs and ds["append_extends"] == 1 and ds["copies_digest"] != 0, (ds, hs)


# ---- 13. errors --------------------------------------------------------------------------------------------------
def test_errors(gpu, oracle):
    import torch
    from expann_amd import GpuBruteForceEngine
    from expann_amd._lib import ExpannError
    n0 = 4500
    rows, queries = _rows(16, n0 + 10, 128)
    # rows adopted from the caller: refused, and the handle still searches
    t = torch.from_numpy(rows[:n0]).cuda()
    torch.cuda.synchronize()
    eng = GpuBruteForceEngine(128, "l2")
    eng.set_base_device(t.data_ptr(), n0, 0)
    with pytest.raises(ExpannError) as e:
        eng.append(rows[n0:])
    assert e.value.code == 5
    with pytest.raises(ExpannError) as e:
        eng.reserve(10000)
    assert e.value.code == 5
    _same(eng.query_k_batch(queries, K), oracle.brute_force(rows[:n0], queries, K, n_threads=16))
    assert eng.size() == n0
    eng.close()
    # before build(): expann_add's job
    eng = GpuBruteForceEngine(128, "l2")
    eng.store_many_vectors(rows[:n0])
    with pytest.raises(ExpannError) as e:
        eng.append(rows[n0:])
    assert e.value.code == 4
    with pytest.raises(ExpannError) as e:
        eng.append_device(t.data_ptr(), 5)
    assert e.value.code == 4
    eng.build()
    # n == 0: EXPANN_OK, and nothing moves but the call counter
    names = ("append_rows", "append_extends", "append_rebuilds", "base_reallocs", "base_capacity_rows", "copies_digest")
    before = _stats(eng, *names)
    eng.append(rows[:0])
    assert gpu.expann_append(eng._h, None, 0) == 0
    assert _stats(eng, *names) == before and eng.get_stat("append_calls") == 2 and eng.size() == n0
    with pytest.raises(ExpannError) as e:  # NULL rows with n > 0
        from expann_amd import _lib
        _lib.check(eng._h, gpu.expann_append(eng._h, None, 3))
    assert e.value.code == 1
    _same(eng.query_k_batch(queries, K), oracle.brute_force(rows[:n0], queries, K, n_threads=16))
    eng.close()


def test_store_after_build_appends(gpu, oracle):
    """the reference's sequence through the engine's own interface: store, build, query, store, query"""
    n0 = 4500
    rows, queries = _rows(17, n0 + 3, 128)
    eng = _engine(rows[:n0])
    eng.store_vector(rows[n0])
    eng.store_many_vectors(rows[n0 + 1:])
    assert eng.size() == n0 + 3
    _same(eng.query_k_batch(queries, K), oracle.brute_force(rows, queries, K, n_threads=16))
    assert eng.query_k(rows[n0 + 2], 1) == [n0 + 2]
    eng.close()


# ---- 14. the C++ engine ----------------------------------------------------------------------------------------
def test_cpp_engine_store_build_query_store_query():
    exe = os.path.join(ROOT, "expann_amd", "host", "expann_append_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("ok"), out.stdout
