"""Removing rows from a built brute-force index (expann_remove, expann_remove_device, expann_compact_row_filter;
DESIGN.md 4.6j).

THE REMOVE RULE: after a remove every entry point answers, bit for bit, as a fresh handle built from the surviving
rows in their old order answers.  Every comparison here is exact -- ids equal, distances equal as uint32 patterns --
against the oracle over the surviving rows AND against a fresh engine built from them; where the fp16 copy was
compacted, "copies_digest" shows that it IS the one the fresh engine built (non-zero and equal).
m = 130 queries and k = 10 unless a case says otherwise; the row with the global max |v| is among the survivors
unless the case is about the scale.  No case provokes a fault: the ids out of range are refused by a comparison."""
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
INVALID_ARG, NOT_BUILT, UNSUPPORTED = 1, 4, 5


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


def _rows(seed, n, d, keep, m=M):
    """n rows and m queries; the row with the largest |v| is row `keep`, which no case removes"""
    rng = np.random.RandomState(seed)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((m, d)).astype(np.float32)
    top = int(np.argmax(np.abs(rows).max(axis=1)))
    rows[[keep, top]] = rows[[top, keep]]
    return rows, queries


def _stats(eng, *names):
    return {n: eng.get_stat(n) for n in names}


class Live:
    """An engine and the original numbers of the rows it still holds."""

    def __init__(self, oracle, rows, queries, metric="l2", dtype="f32", opts=(), ometric=None, warm=False, reserve=0):
        self.oracle, self.rows, self.queries = oracle, rows, queries
        self.kw = dict(metric=metric, dtype=dtype, opts=opts)
        self.ometric = oracle.METRIC_L2_F32 if ometric is None else ometric
        self.alive = np.arange(rows.shape[0])
        self.eng = _engine(rows, reserve=reserve, **self.kw)
        self.warm = warm
        if warm:  # (the fp16 copy is not made at build under a forced "scan_kernel": the first search makes it)
            self.eng.query_k_batch(queries, K)

    def survivors(self):
        return self.rows[self.alive]

    def remove(self, ids, keep=None, how="host"):
        """remove the CURRENT ids `ids`; check the count, the size and the search against the oracle"""
        ids = np.asarray(ids, dtype=np.uint64)
        gone = np.unique(ids).astype(np.int64)
        if keep is not None:  # (the original number of the row that carries max |v|)
            assert keep not in self.alive[gone]
        if how == "host":
            removed = self.eng.remove(ids)
        else:
            removed = how(self.eng, ids)
        self.alive = np.delete(self.alive, gone)
        assert removed == gone.size
        assert self.eng.size() == self.alive.size
        self.check("after removing %d rows" % gone.size)

    def check(self, note=None, k=K):
        want = self.oracle.brute_force(self.survivors(), self.queries, k, self.ometric, n_threads=16)
        _same(self.eng.query_k_batch(self.queries, k), want, note)
        return want

    def check_shift(self):
        """a survivor's nearest neighbour is itself, at its NEW id (L2 over distinct float rows)"""
        n = self.alive.size
        at = np.array([0, 1, n // 3, n // 2, n - 2, n - 1])
        ids, dists = self.eng.query_k_batch(self.survivors()[at], 1)
        assert np.array_equal(ids[:, 0], at.astype(np.uint64)) and np.all(dists[:, 0] == 0)

    def fresh(self):
        eng = _engine(self.survivors(), **self.kw)
        if self.warm:
            eng.query_k_batch(self.queries, K)
        return eng

    def check_fresh(self, digest=True, k=K):
        """the same answers as an engine built from the survivors; with digest: and the same, non-zero, fp16 copy"""
        fresh = self.fresh()
        _same(self.eng.query_k_batch(self.queries, k), fresh.query_k_batch(self.queries, k))
        fd, d = fresh.get_stat("copies_digest"), self.eng.get_stat("copies_digest")
        fresh.close()
        if digest and fd == 0 and self.alive.size < 4096:
            # below 4 096 rows the direct scan serves and a fresh index makes no fp16 copy by itself, while a remove
            # carries the one it has over: the copy to compare with is made by forcing the fp16 form ("scan_kernel" 4)
            kw = dict(self.kw, opts=tuple(self.kw["opts"]) + (("scan_kernel", 4),))
            forced = _engine(self.survivors(), **kw)
            _same(self.eng.query_k_batch(self.queries, k), forced.query_k_batch(self.queries, k))
            fd = forced.get_stat("copies_digest")
            forced.close()
        if digest:
            assert d == fd and fd != 0, (d, fd)
        return d, fd

    def close(self):
        self.eng.close()


# ---- 1. tile edges ---------------------------------------------------------------------------------------------
def test_tile_edges_d128(gpu, oracle):
    n, keep = 6000, 3000
    rows, queries = _rows(1, n, 128, keep)
    live = Live(oracle, rows, queries)
    d0 = live.eng.get_stat("copies_digest")
    rng = np.random.RandomState(101)

    def random_ids():
        cur = live.alive.size
        cand = np.setdiff1d(np.arange(cur), np.flatnonzero(live.alive == keep))
        ids = rng.choice(cand, 500, replace=False)
        return np.concatenate([ids, ids[:50]])[rng.permutation(550)]  # 50 of them twice, in any order

    steps = [lambda: [0],
             lambda: [live.alive.size - 1],
             lambda: np.arange(60, 125),                       # crosses a 64-row and a 128-row tile edge
             lambda: np.arange(1000, 1400, 2),
             random_ids,
             lambda: np.arange(5000, 4700, -1)]                 # descending
    want_removed = [1, 1, 65, 200, 500, 300]
    for step, w in zip(steps, want_removed):
        before = live.alive.size
        live.remove(step(), keep=keep)
        assert before - live.alive.size == w
        live.check_shift()
        d, fd = live.check_fresh()
        assert d != d0
    prof = live.eng.get_profile()
    st = _stats(live.eng, "remove_calls", "remove_rows", "remove_compacts", "remove_rebuilds", "base_capacity_rows",
                "base_reallocs", "base_bytes")
    live.close()
    assert prof["scan_kernel"].startswith(F16X), prof
    assert st == dict(remove_calls=6, remove_rows=sum(want_removed), remove_compacts=6, remove_rebuilds=0,
                      base_capacity_rows=n, base_reallocs=0, base_bytes=(n - sum(want_removed)) * 128 * 4), st


# ---- 2. the maxima -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,oname", [("l2", "METRIC_L2_F32"), ("ip", "METRIC_IP_F32")])
def test_the_row_with_the_largest_norm_goes(gpu, oracle, metric, oname):
    """max ||b||^2 has to be recomputed: a stale one shows in the digest (and in the inner product's query scaling)"""
    rng = np.random.RandomState(2)
    n = 5000
    rows = np.clip(rng.standard_normal((n, 128)) * 0.4, -1.4, 1.4).astype(np.float32)
    queries = (rng.standard_normal((M, 128)) * 0.4).astype(np.float32)
    rows[10, 5] = 1.5      # max |v|: scale 2^14; stays
    rows[4000] = 1.2       # ||b||^2 = 184, far the largest; max |v| 1.2 < 1.5
    live = Live(oracle, rows, queries, metric=metric, ometric=getattr(oracle, oname))
    live.remove([4000], keep=10)
    live.check_fresh()
    st = _stats(live.eng, "remove_compacts", "remove_rebuilds")
    live.close()
    assert st == dict(remove_compacts=1, remove_rebuilds=0), st


def test_the_scale_changes(gpu, oracle):
    rng = np.random.RandomState(3)
    n = 5000
    rows = np.clip(rng.standard_normal((n, 128)) * 0.4, -1.4, 1.4).astype(np.float32)
    queries = (rng.standard_normal((M, 128)) * 0.4).astype(np.float32)
    rows[10, 5] = 1.5
    rows[77, 9] = -1.9     # 2^14 with or without it: compact
    rows[4000, 7] = 2.5    # 2^13 while it is there
    live = Live(oracle, rows, queries)
    live.remove([4000])
    live.check_fresh()
    assert _stats(live.eng, "remove_compacts", "remove_rebuilds") == dict(remove_compacts=0, remove_rebuilds=1)
    live.remove([77])      # 1.9 -> 1.5: the scale stays
    live.check_fresh()
    st = _stats(live.eng, "remove_compacts", "remove_rebuilds")
    live.close()
    assert st == dict(remove_compacts=1, remove_rebuilds=1), st


def test_an_unusable_mark_is_forgotten(gpu, oracle):
    n = 5000
    rows, queries = _rows(4, n, 128, 10)
    rows[2222, 3] = 1e30   # beyond every fp16 scale: no fp16 form serves
    live = Live(oracle, rows, queries)
    live.eng.query_k_batch(queries, K)   # (only its kernel is looked at: that row's distances are +inf in fp32)
    p0 = live.eng.get_profile()
    assert live.eng.get_stat("copies_digest") == 0
    live.remove([2222])
    p1 = live.eng.get_profile()
    live.check_fresh()
    st = _stats(live.eng, "remove_compacts", "remove_rebuilds")
    live.close()
    assert not p0["scan_kernel"].startswith("scan_gemm_f16"), p0   # (no fp16 form: the bf16x3 form or the direct scan)
    assert p1["scan_kernel"].startswith(F16X), p1
    assert st == dict(remove_compacts=0, remove_rebuilds=1), st


# ---- 3. geometries -----------------------------------------------------------------------------------------------
def _mixed_ids(n, keep, seed):
    """row 0, the last row, a run across a tile edge and 300 random rows, none of them `keep`"""
    rng = np.random.RandomState(seed)
    ids = np.concatenate([[0, n - 1], np.arange(120, 131), rng.choice(np.arange(200, n - 1), 300, replace=False)])
    return ids[ids != keep]


@pytest.mark.parametrize("d,opts,warm,kernel", [(144, (("scan_kernel", 4),), True, "scan_gemm_f16kl"),
                                                (256, (), False, "scan_gemm_f16y")])
def test_other_dims(gpu, oracle, d, opts, warm, kernel):
    n, keep = 5003, 2500
    rows, queries = _rows(5 + d, n, d, keep)
    live = Live(oracle, rows, queries, opts=opts, warm=warm)
    live.remove(_mixed_ids(n, keep, d), keep=keep)
    live.check_shift()
    live.check_fresh()
    prof = live.eng.get_profile()
    st = _stats(live.eng, "remove_compacts", "remove_rebuilds")
    live.close()
    assert prof["scan_kernel"].startswith(kernel), prof
    assert st == dict(remove_compacts=1, remove_rebuilds=0), st


def test_f16_rows(gpu, oracle):
    n, keep = 5003, 2500
    rows, queries = _rows(6, n, 128, keep)
    rows = rows.astype(np.float16).astype(np.float32)
    live = Live(oracle, rows, queries, dtype="f16")
    live.remove(_mixed_ids(n, keep, 6), keep=keep)
    live.check_shift()
    live.check_fresh()
    st = _stats(live.eng, "remove_compacts", "remove_rebuilds", "base_bytes")
    live.close()
    assert st == dict(remove_compacts=1, remove_rebuilds=0, base_bytes=live.alive.size * 128 * 2), st


def test_inner_product(gpu, oracle):
    n, keep = 5003, 2500
    rows, queries = _rows(7, n, 128, keep)
    queries[::2] *= np.float32(1e-3)
    live = Live(oracle, rows, queries, metric="ip", ometric=oracle.METRIC_IP_F32)
    live.remove(_mixed_ids(n, keep, 7), keep=keep)
    live.check_fresh()
    st = _stats(live.eng, "remove_compacts", "remove_rebuilds")
    live.close()
    assert st == dict(remove_compacts=1, remove_rebuilds=0), st


# ---- 4. 8-bit and int16 rows: only the base is compacted ---------------------------------------------------------
@pytest.mark.parametrize("dtype,metric,oname,d", [("u8", "l2", "METRIC_L2_U8", 128), ("i8", "ip", "METRIC_IP_I8", 128),
                                                  ("i16", "l2", "METRIC_L2_I16_REFCOMPAT", 64)])
def test_integer_rows(gpu, oracle, dtype, metric, oname, d):
    rng = np.random.RandomState(8)
    n = 5000
    if dtype == "u8":
        rows = rng.randint(0, 256, size=(n, d)).astype(np.uint8)
        queries = rng.randint(0, 256, size=(M, d)).astype(np.float32)
    elif dtype == "i8":
        rows = rng.randint(-127, 128, size=(n, d)).astype(np.int8)
        queries = rng.randint(-127, 128, size=(M, d)).astype(np.int8)
    else:
        rows = rng.randint(-90, 91, size=(n, d)).astype(np.int16)
        queries = rng.randint(-90, 91, size=(M, d)).astype(np.int16)
    live = Live(oracle, rows, queries, metric=metric, dtype=dtype, ometric=getattr(oracle, oname))
    live.check()
    live.remove(_mixed_ids(n, -1, 8))
    d_live, d_fresh = live.check_fresh(digest=False)
    st = _stats(live.eng, "remove_calls", "remove_compacts", "remove_rebuilds", "base_bytes", "base_capacity_rows")
    live.close()
    assert d_live == 0 and d_fresh == 0
    assert st == dict(remove_calls=1, remove_compacts=0, remove_rebuilds=0, base_bytes=live.alive.size * d * rows.itemsize,
                      base_capacity_rows=n), st


def test_i8_rows_on_the_matrix_cores(gpu, oracle):
    """33 000 int8 rows under "scan_kernel" 5: the hit-queue form's int8 operand IS the base, so the alias must not
    outlive the base a remove replaces; its row terms are made again by the next search"""
    rng = np.random.RandomState(9)
    n = 33000
    rows = rng.randint(-127, 128, size=(n, 128)).astype(np.int8)
    queries = rng.randint(-127, 128, size=(M, 128)).astype(np.int8)
    live = Live(oracle, rows, queries, metric="ip", dtype="i8", opts=(("scan_kernel", 5),), ometric=oracle.METRIC_IP_I8)
    live.check()
    p0 = live.eng.get_profile()
    live.remove(np.concatenate([[0, n - 1], np.arange(20000, 20150)]))   # 32 848 rows stay: above the form's minimum
    p1 = live.eng.get_profile()
    live.check_fresh(digest=False)
    live.close()
    assert p0["scan_kernel"].startswith("scan_gemm_i8w"), p0
    assert p1["scan_kernel"].startswith("scan_gemm_i8w"), p1


# ---- 5. together with the rest -----------------------------------------------------------------------------------
def test_remove_then_append_within_the_capacity(gpu, oracle):
    n, keep = 5000, 2500
    rows, queries = _rows(10, n + 400, 128, keep)
    live = Live(oracle, rows[:n], queries)
    live.remove(_mixed_ids(n, keep, 10), keep=keep)
    removed = n - live.alive.size
    assert removed > 300
    live.eng.append(rows[n:n + 300])                     # fits into the freed room
    live.rows = rows
    live.alive = np.concatenate([live.alive, np.arange(n, n + 300)])
    assert live.eng.size() == live.alive.size
    live.check("after the append")
    ids, _ = live.eng.query_k_batch(rows[n:n + 1], 1)
    assert ids[0, 0] == n - removed                      # the ids continue at the new size
    live.check_fresh()
    st = _stats(live.eng, "base_reallocs", "base_capacity_rows", "append_extends", "append_rebuilds", "remove_compacts")
    live.close()
    assert st == dict(base_reallocs=0, base_capacity_rows=n, append_extends=1, append_rebuilds=0, remove_compacts=1), st


def test_append_then_remove_old_and_new_rows(gpu, oracle):
    n, keep = 5000, 2500
    rows, queries = _rows(11, n + 700, 128, keep)
    live = Live(oracle, rows[:n], queries)
    live.eng.append(rows[n:])
    live.rows = rows
    live.alive = np.arange(n + 700)
    live.remove(np.concatenate([np.arange(n - 40, n + 90), [3, n + 699], np.arange(n + 300, n + 500, 3)]), keep=keep)
    live.check_shift()
    live.check_fresh()
    st = _stats(live.eng, "append_extends", "remove_compacts", "remove_rebuilds", "base_reallocs")
    live.close()
    assert st == dict(append_extends=1, remove_compacts=1, remove_rebuilds=0, base_reallocs=1), st


def test_other_entry_points_after_a_remove(gpu, oracle):
    n, keep = 5000, 2500
    rows, queries = _rows(12, n, 128, keep)
    live = Live(oracle, rows, queries)
    rng = np.random.RandomState(120)
    live.eng.set_row_filter(rng.rand(n) < 0.3)
    live.eng.set_row_groups(rng.randint(0, 7, n).astype(np.uint32))
    assert _stats(live.eng, "filter_active", "groups_active") == dict(filter_active=1, groups_active=1)
    live.remove(_mixed_ids(n, keep, 12), keep=keep)       # (the search inside runs unfiltered: the filter is gone)
    n1 = live.alive.size
    assert _stats(live.eng, "filter_active", "groups_active", "filter_rows") == dict(filter_active=0, groups_active=0,
                                                                                   filter_rows=n1)
    surv, eng, fresh = live.survivors(), live.eng, live.fresh()
    ref20 = oracle.brute_force(surv, queries, 20, n_threads=16)
    # score_ids: the new numbering; ids beyond the new size are refused as before
    from expann_amd._lib import ExpannError
    ids = np.concatenate([np.arange(n1 - 45, n1), [0, 5]]).astype(np.uint64)
    cutoff = float(np.median(ref20[1][0]) * 4)
    kept, sc = eng.score_ids(queries[0], ids, cutoff)
    rkept, rsc = oracle.filter_by_score(surv, queries[0], ids, cutoff)
    assert np.array_equal(kept, rkept) and np.array_equal(sc.view(np.uint32), rsc.view(np.uint32)) and kept.size
    for e in (eng, fresh):
        with pytest.raises(ExpannError):
            e.score_ids(queries[0], np.array([0, n1], dtype=np.uint64), cutoff)
    # range search with each query's exact 10th distance as its radius
    radii = ref20[1][:, K - 1].copy()
    want_counts = (ref20[1] <= radii[:, None]).sum(axis=1).astype(np.uint32)
    rids, rdists, counts = eng.range_search(queries, radii, K)
    fids, fdists, fcounts = fresh.range_search(queries, radii, K)
    assert np.array_equal(counts, want_counts) and np.array_equal(fcounts, want_counts)
    _same((rids, rdists), (ref20[0][:, :K], ref20[1][:, :K]))
    _same((fids, fdists), (rids, rdists))
    # a filter and groups set for the shorter index
    allow = rng.rand(n1) < 0.4
    labels = rng.randint(0, 5, n1).astype(np.uint32)
    qg = rng.randint(0, 5, M).astype(np.uint32)
    for e in (eng, fresh):
        e.set_row_groups(labels)
    _same(eng.query_k_batch(queries, K, groups=qg), fresh.query_k_batch(queries, K, groups=qg))
    g_ids, _ = eng.query_k_batch(queries, K, groups=qg)
    assert np.all(labels[g_ids[:, 0].astype(np.int64)] == qg)
    for e in (eng, fresh):
        e.set_row_groups(None)
        e.set_row_filter(allow)
    want = oracle.brute_force(surv[allow], queries, K, n_threads=16)
    got = eng.query_k_batch(queries, K)
    _same(got, fresh.query_k_batch(queries, K))
    assert np.array_equal(np.flatnonzero(allow)[want[0].astype(np.int64)].astype(np.uint64), got[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    fresh.close()
    live.close()


def test_int8_filter_runs_again_after_a_remove(gpu, oracle):
    """ "i8_filter" = 2 at 33 000 rows (test_gpu_append.py's shape for that copy): dropped by the remove, made again
    by the next search"""
    n, keep = 33500, 2500
    rows, queries = _rows(13, n, 128, keep)
    live = Live(oracle, rows, queries, opts=(("i8_filter", 2),))
    live.check()
    p0 = live.eng.get_profile()
    live.remove(_mixed_ids(n, keep, 13), keep=keep)
    p1 = live.eng.get_profile()
    live.check_fresh()
    live.close()
    assert p0["scan_kernel"] == I8F, p0
    assert p1["scan_kernel"] == I8F, p1


# ---- 6. compact_row_filter ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [0.5, 0.01])
def test_compact_row_filter(gpu, oracle, share):
    n, keep = 6000, 3000
    rows, queries = _rows(14, n, 128, keep)
    rng = np.random.RandomState(140)
    allow = rng.rand(n) < share
    allow[keep] = True
    live = Live(oracle, rows, queries)
    twin = Live(oracle, rows, queries)
    live.eng.set_row_filter(allow)
    under = live.eng.query_k_batch(queries, K)              # the tombstoned search: the same rows, their OLD ids
    removed = live.eng.compact_row_filter()
    live.alive = np.flatnonzero(allow)
    assert removed == n - live.alive.size and live.eng.size() == live.alive.size
    assert _stats(live.eng, "filter_active", "filter_rows") == dict(filter_active=0, filter_rows=live.alive.size)
    want = live.check()
    real = under[0] != PAD
    assert np.array_equal(live.alive[want[0][real].astype(np.int64)].astype(np.uint64), under[0][real])
    assert np.array_equal(under[1].view(np.uint32), want[1].view(np.uint32))
    twin.remove(np.flatnonzero(~allow), keep=keep)
    _same(live.eng.query_k_batch(queries, K), twin.eng.query_k_batch(queries, K))
    d, _ = live.check_fresh()
    assert d == twin.eng.get_stat("copies_digest")
    st = _stats(live.eng, "remove_calls", "remove_rows", "remove_compacts")
    live.close()
    twin.close()
    assert st == dict(remove_calls=1, remove_rows=removed, remove_compacts=1), st


def test_compact_row_filter_all_and_nothing(gpu, oracle):
    from expann_amd._lib import ExpannError
    n = 6000
    rows, queries = _rows(15, n, 128, 3000)
    live = Live(oracle, rows, queries)
    d0 = live.eng.get_stat("copies_digest")
    with pytest.raises(ExpannError) as e:                   # no filter in force
        live.eng.compact_row_filter()
    assert e.value.code == INVALID_ARG
    live.eng.set_row_filter(np.ones(n, dtype=bool))         # allows every row: removes nothing, keeps every copy
    assert live.eng.compact_row_filter() == 0
    assert live.eng.size() == n and live.eng.get_stat("copies_digest") == d0 != 0
    assert _stats(live.eng, "filter_active", "remove_rows", "remove_compacts", "remove_rebuilds") == dict(
        filter_active=0, remove_rows=0, remove_compacts=0, remove_rebuilds=0)
    live.check()
    live.eng.set_row_filter(np.zeros(n, dtype=bool))        # allows nothing: refused, and the filter stays
    with pytest.raises(ExpannError) as e:
        live.eng.compact_row_filter()
    assert e.value.code == INVALID_ARG
    assert _stats(live.eng, "filter_active", "filter_rows") == dict(filter_active=1, filter_rows=0)
    assert live.eng.size() == n and np.all(live.eng.query_k_batch(queries, K)[0] == PAD)
    live.eng.set_row_filter(None)
    live.check()
    assert live.eng.get_stat("copies_digest") == d0
    live.close()


# ---- 7. refusals leave the handle as it was ----------------------------------------------------------------------
def _device_remove(eng, ids, stream=None):
    import torch
    t = torch.from_numpy(np.asarray(ids, dtype=np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return eng.remove_device(t.data_ptr(), t.numel(), stream=0 if stream is None else stream)


def test_refusals(gpu, oracle):
    import ctypes as C
    import torch
    from expann_amd import GpuBruteForceEngine, _lib
    from expann_amd._lib import ExpannError
    n = 5000
    rows, queries = _rows(16, n, 128, 2500)
    live = Live(oracle, rows, queries)
    want = live.check()
    d0 = live.eng.get_stat("copies_digest")
    names = ("remove_calls", "remove_rows", "remove_compacts", "remove_rebuilds", "base_capacity_rows")
    s0 = _stats(live.eng, *names)

    def unchanged():
        assert live.eng.size() == n and live.eng.get_stat("copies_digest") == d0 != 0
        _same(live.eng.query_k_batch(queries, K), want)
        assert _stats(live.eng, *names) == s0

    for bad in ([n], [5, n, 7], [2 ** 63], [2 ** 64 - 1, 3], [2 ** 32 + 5]):   # (2^32 + 5: not row 5)
        with pytest.raises(ExpannError) as e:
            live.eng.remove(np.array(bad, dtype=np.uint64))
        assert e.value.code == INVALID_ARG, bad
        unchanged()
        with pytest.raises(ExpannError) as e:
            _device_remove(live.eng, bad)
        assert e.value.code == INVALID_ARG, bad
        unchanged()
    with pytest.raises(ExpannError) as e:                   # every row: an index is never empty
        live.eng.remove(np.arange(n))
    assert e.value.code == INVALID_ARG
    unchanged()
    removed = C.c_size_t(99)                                # NULL ids with n_ids > 0
    assert gpu.expann_remove(live.eng._h, None, 3, C.byref(removed)) == INVALID_ARG
    unchanged()
    # n_ids == 0: EXPANN_OK, nothing moves but the call counter; a NULL n_removed is fine
    assert live.eng.remove(np.zeros(0, dtype=np.uint64)) == 0
    assert gpu.expann_remove(live.eng._h, None, 0, None) == 0
    assert gpu.expann_remove_device(live.eng._h, None, 0, None, None) == 0
    s0["remove_calls"] = 3
    unchanged()
    ids = (C.c_uint64 * 2)(17, 17)
    assert gpu.expann_remove(live.eng._h, ids, 2, None) == 0 and live.eng.size() == n - 1
    live.close()
    # rows adopted from the caller: refused, and the handle still searches
    t = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    eng = GpuBruteForceEngine(128, "l2")
    eng.set_base_device(t.data_ptr(), n, 0)
    for call in (lambda: eng.remove([1, 2]), lambda: _device_remove(eng, [1, 2])):
        with pytest.raises(ExpannError) as e:
            call()
        assert e.value.code == UNSUPPORTED
    _same(eng.query_k_batch(queries, K), want)
    assert eng.size() == n
    eng.close()
    # before build()
    eng = GpuBruteForceEngine(128, "l2")
    eng.store_many_vectors(rows)
    for call in (lambda: eng.remove([1, 2]), lambda: _device_remove(eng, [1, 2])):
        with pytest.raises(ExpannError) as e:
            call()
        assert e.value.code == NOT_BUILT
    with pytest.raises(ExpannError) as e:
        _lib.check(eng._h, gpu.expann_remove(eng._h, None, 3, None))      # (NULL ids come first)
    assert e.value.code == INVALID_ARG
    eng.build()
    _same(eng.query_k_batch(queries, K), want)
    eng.close()


# ---- 8. device ids and streams -----------------------------------------------------------------------------------
def test_remove_device_equals_the_host_remove(gpu, oracle):
    import torch
    n, keep = 5000, 2500
    rows, queries = _rows(17, n, 128, keep)
    ids = _mixed_ids(n, keep, 17)
    host = Live(oracle, rows, queries)
    host.remove(ids, keep=keep)
    dev = Live(oracle, rows, queries)
    st = torch.cuda.Stream()

    def on_side_stream(eng, ids):
        with torch.cuda.stream(st):                         # the ids are PRODUCED on the side stream
            t = torch.from_numpy(ids.view(np.int64) - 1).cuda(non_blocking=True) + 1
            removed = eng.remove_device(t.data_ptr(), t.numel(), stream=st.cuda_stream)
            t.zero_()                                       # (they were read: the caller may reuse them on return)
        torch.cuda.synchronize()
        return removed

    dev.remove(ids, keep=keep, how=on_side_stream)
    _same(dev.eng.query_k_batch(queries, K), host.eng.query_k_batch(queries, K))
    names = ("remove_calls", "remove_rows", "remove_compacts", "remove_rebuilds", "copies_digest")
    ds, hs = _stats(dev.eng, *names), _stats(host.eng, *names)
    dev.close()
    host.close()
    assert ds == hs and ds["remove_compacts"] == 1 and ds["copies_digest"] != 0, (ds, hs)


def test_a_deferred_search_sees_the_rows_before_the_remove(gpu, oracle):
    import torch
    n, keep = 5000, 2500
    rows, queries = _rows(18, n, 128, keep)
    live = Live(oracle, rows, queries)
    old_ref = live.check()
    tq = torch.from_numpy(queries).cuda()
    tid = torch.empty(M, K, dtype=torch.int64, device="cuda")
    td = torch.empty(M, K, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    live.eng.set_option("async_search", 1)
    live.eng.search_device(tq.data_ptr(), M, K, tid.data_ptr(), td.data_ptr(), st.cuda_stream)
    gone = np.unique(old_ref[0][:, 0]).astype(np.int64)     # every query's nearest row goes
    gone = gone[gone != keep]
    live.eng.remove(gone)
    live.eng.sync()
    torch.cuda.synchronize()
    live.eng.set_option("async_search", 0)
    _same((tid.cpu().numpy().astype(np.uint64), td.cpu().numpy()), old_ref)
    live.alive = np.delete(live.alive, gone)
    live.check()
    live.check_fresh()
    live.close()


# ---- 9. fewer than k survivors -----------------------------------------------------------------------------------
def test_fewer_than_k_survivors(gpu, oracle):
    n = 300
    rows, queries = _rows(19, n, 128, 100)
    live = Live(oracle, rows, queries)
    stay = np.array([3, 64, 100, 127, 128, 255, 299])
    live.remove(np.setdiff1d(np.arange(n), stay), keep=100)
    ids, dists = live.eng.query_k_batch(queries, K)
    live.check_fresh(digest=False)
    live.close()
    assert live.alive.tolist() == stay.tolist()
    assert np.all(ids[:, 7:] == PAD) and np.all(np.isposinf(dists[:, 7:]))
    assert np.all(np.sort(ids[:, :7], axis=1) == np.arange(7, dtype=np.uint64))


# ---- 10. the C++ engine ------------------------------------------------------------------------------------------
def test_cpp_engine_store_build_query_remove_query_append_query():
    exe = os.path.join(ROOT, "expann_amd", "host", "expann_remove_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("ok"), out.stdout
