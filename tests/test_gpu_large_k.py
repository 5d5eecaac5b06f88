"""Brute-force search at k from 128 to the bound of 8192 (and one step past it): every path the host planning
switches to above k = 100 -- the int8 filters and the uint8 shadow drop out at k > 256, the sampled fp16 pass stops
there too and the threshold ladder runs level by level, the candidate lists sit at their largest capacity from
k = 257 on, the select kernels rank lists nearly as long as k, the host call stops staging at m * k > 16384.  Ids
and fp32 distances (as uint32 bit patterns) must equal the oracle's, the return code must be EXPANN_OK, and where
k exceeds the row count the tail is UINT64_MAX / +inf.

One oracle call per base at k = 8192 serves every smaller k: the oracle's order (score, then id) is total, so its
top k is the first k of its top 8192.  Rows are iid (Gaussian fp32, uniform int8, folded-Gaussian uint8); the seeds
are fixed and no two rows are equal.  Equal SCORES of different rows cannot be avoided at these k -- among the 8192
nearest of 10^5 Gaussian rows the fp32 scores lie about 400 ulps apart on average, a few dozen pairs per query
coincide, and integer scores of 8-bit rows coincide far more often; both sides order them by id.  Rows that are
equal on purpose belong to the tie test alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = np.uint64(2 ** 64 - 1)
K_MAX = 8192          # the bound on k (expann_search's comment in include/expann_hip.h)
M = 100


def _rows(kind, shape, seed):
    rng = np.random.RandomState(seed)
    if kind == "gauss":
        return rng.standard_normal(shape).astype(np.float32)
    if kind == "u8":
        return np.clip(np.round(np.abs(rng.standard_normal(shape)) * 40), 0, 255).astype(np.uint8)
    if kind == "i8":
        return rng.randint(-128, 128, size=shape).astype(np.int8)
    if kind == "ints":                             # SIFT-like: fp32 rows holding 0 .. 255
        return np.clip(np.round(np.abs(rng.standard_normal(shape)) * 40), 0, 255).astype(np.float32)
    raise ValueError(kind)


class _Bank:
    """rows, queries, oracle results and engines, each made once per module and then only read"""

    def __init__(self, oracle):
        self.oracle, self._rows, self._q, self._ref, self._eng = oracle, {}, {}, {}, {}

    def rows(self, kind, n, d):
        key = (kind, n, d)
        if key not in self._rows:
            self._rows[key] = _rows(kind, (n, d), 7_000_000 + n + d)
            self._rows[key].setflags(write=False)
        return self._rows[key]

    def queries(self, kind, d, m=M):
        key = (kind, d, m)
        if key not in self._q:
            q = _rows(kind, (m, d), 9_000_000 + d + m)
            self._q[key] = q.astype(np.float32) if kind == "u8" else q
            self._q[key].setflags(write=False)
        return self._q[key]

    def ometric(self, kind, metric):
        o = self.oracle
        return {("gauss", "l2"): o.METRIC_L2_F32, ("gauss", "ip"): o.METRIC_IP_F32, ("ints", "l2"): o.METRIC_L2_F32,
                ("u8", "l2"): o.METRIC_L2_U8, ("i8", "l2"): o.METRIC_L2_I8, ("i8", "ip"): o.METRIC_IP_I8}[(kind, metric)]

    def ref(self, kind, n, d, metric):
        """the oracle's top K_MAX of the module's M queries over rows(kind, n, d)"""
        key = (kind, n, d, metric)
        if key not in self._ref:
            ids, dd = self.oracle.brute_force(self.rows(kind, n, d), self.queries(kind, d), K_MAX,
                                              self.ometric(kind, metric), n_threads=16)
            ids.setflags(write=False)
            dd.setflags(write=False)
            self._ref[key] = (ids, dd)
        return self._ref[key]

    def engine(self, kind, n, d, metric):
        from expann_amd import GpuBruteForceEngine
        key = (kind, n, d, metric)
        if key not in self._eng:
            eng = GpuBruteForceEngine(d, metric, {"gauss": "f32", "ints": "f32", "u8": "u8", "i8": "i8"}[kind])
            eng.store_many_vectors(self.rows(kind, n, d))
            eng.build()
            eng.set_profiling(True)
            self._eng[key] = eng
        return self._eng[key]

    def close(self):
        for eng in self._eng.values():
            eng.close()
        self._eng.clear()


@pytest.fixture(scope="module")
def bank(oracle):
    from expann_amd import _lib
    assert _lib.load().expann_device_count() >= 1, "these tests need a HIP device"
    b = _Bank(oracle)
    yield b
    b.close()


def _search(eng, queries, k):
    """expann_search through the C ABI: (return code, ids, dists, profile, error text) -- no exception, so that
    the code itself can be asserted"""
    queries = np.ascontiguousarray(queries)
    m = queries.shape[0]
    ids = np.full((m, k), 12345, dtype=np.uint64)
    dists = np.full((m, k), -1.0, dtype=np.float32)
    eng.get_profile()
    rc = eng._L.expann_search(eng._h, queries.ctypes.data, m, k, ids.ctypes.data, dists.ctypes.data)
    err = eng._L.expann_last_error(eng._h).decode() if rc else ""
    return rc, ids, dists, eng.get_profile(), err


def _check(eng, queries, k, ref, n, what, gemm=False, no_retry=False):
    """the three assertions of every case; ref = the oracle's lists of these queries at any k' >= k"""
    rc, ids, dists, prof, err = _search(eng, queries, k)
    what = f"{what} k={k}: kernel {prof['scan_kernel']!r} retries {prof['retries']}"
    print(what)
    assert rc == 0, f"{what}: return code {rc}: {err}"
    rids, rd = ref[0][:queries.shape[0], :k], ref[1][:queries.shape[0], :k]
    bad = np.flatnonzero((ids != rids).any(1))
    assert bad.size == 0, f"{what}: ids of {bad.size} queries differ from the oracle's, first {bad[:5]}"
    bad = np.flatnonzero((dists.view(np.uint32) != rd.view(np.uint32)).any(1))
    assert bad.size == 0, f"{what}: distance bits of {bad.size} queries differ, first {bad[:5]}"
    if k > n:
        assert (ids[:, n:] == PAD).all() and np.isposinf(dists[:, n:]).all(), f"{what}: padding"
        assert (ids[:, :n] != PAD).all(), f"{what}: padding before position n"
    if gemm:
        assert prof["scan_kernel"].startswith("scan_gemm_"), what
    if no_retry:
        assert prof["retries"] == 0, what
    return prof


F32_KS = [128, 255, 256, 257, 1000, 2048, 4096, 6000, 8192]
F32_CASES = [(n, d, k) for n in (70001, 131072) for d, ks in ((128, F32_KS), (64, [257, 2048, 8192]), (192, [257, 2048, 8192]))
             for k in ks]


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("n,d,k", F32_CASES)
def test_f32_matrix_core_forms(bank, n, d, k, metric):
    """100 queries: the fp16 GEMM filter, with the int8 filters and the sampled pass up to k = 256 and the plain
    ladder beyond.  Up to k = 4096 a retry would mean the plan is wrong, not that the data was unlucky: a level is
    planned to keep at most max(2 k, cap / 6) <= cap / 2 rows and the spread of that count is under 100."""
    _check(bank.engine("gauss", n, d, metric), bank.queries("gauss", d), k, bank.ref("gauss", n, d, metric), n,
           f"f32 {metric} n={n} d={d} m={M}", gemm=k <= 256, no_retry=k <= 4096)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("k", [257, 2048, 8192])
@pytest.mark.parametrize("n", [20000, 70001])
def test_f32_three_queries(bank, n, k, metric):
    """m = 3: below the matrix-core forms' crossover"""
    _check(bank.engine("gauss", n, 128, metric), bank.queries("gauss", 128)[:3], k, bank.ref("gauss", n, 128, metric),
           n, f"f32 {metric} n={n} d=128 m=3")


@pytest.mark.parametrize("n,k", [(5000, 4999), (5000, 5000), (5000, 5001), (5000, 8192), (16384, 8192)])
def test_single_level_indexes_and_padding(bank, n, k):
    """n_groups <= s0: one level keeps every row, the select ranks a list as long as the index; k > n pads"""
    _check(bank.engine("gauss", n, 128, "l2"), bank.queries("gauss", 128)[:9], k, bank.ref("gauss", n, 128, "l2"), n,
           f"f32 l2 n={n} d=128 m=9")


EIGHT_BIT = [("u8", "l2"), ("i8", "l2"), ("i8", "ip")]


@pytest.mark.parametrize("k", [256, 257, 2048, 8192])
@pytest.mark.parametrize("d", [128, 192])
@pytest.mark.parametrize("kind,metric", EIGHT_BIT)
def test_8_bit_rows(bank, kind, metric, d, k):
    _check(bank.engine(kind, 70001, d, metric), bank.queries(kind, d), k, bank.ref(kind, 70001, d, metric), 70001,
           f"{kind} {metric} n=70001 d={d} m={M}")


@pytest.mark.parametrize("k", [257, 8192])
@pytest.mark.parametrize("d", [128, 192])
@pytest.mark.parametrize("kind,metric", EIGHT_BIT)
def test_8_bit_rows_three_queries(bank, kind, metric, d, k):
    _check(bank.engine(kind, 70001, d, metric), bank.queries(kind, d)[:3], k, bank.ref(kind, 70001, d, metric), 70001,
           f"{kind} {metric} n=70001 d={d} m=3")


@pytest.mark.parametrize("k", [256, 257])
def test_integer_valued_f32_rows(bank, k):
    """fp32 rows that hold integers 0 .. 255 (SIFT): k = 256 is the last the uint8 shadow serves, 257 the first
    it does not"""
    _check(bank.engine("ints", 70001, 128, "l2"), bank.queries("ints", 128), k, bank.ref("ints", 70001, 128, "l2"),
           70001, f"integer-valued f32 l2 n=70001 d=128 m={M}")


@pytest.mark.parametrize("m", [3, 130])
def test_massive_exact_ties(bank, m):
    """20 000 copies of one row among 70 001, k = 1000: ties are broken by the lower id"""
    from expann_amd import GpuBruteForceEngine
    n, d, k = 70001, 128, 1000
    rng = np.random.RandomState(77)
    base = bank.rows("gauss", n, d).copy()
    copies = np.sort(rng.choice(n, 20000, replace=False))
    base[copies] = base[copies[0]]
    queries = rng.standard_normal((m, d)).astype(np.float32)
    queries[0] = base[copies[0]]
    ref = bank.oracle.brute_force(base, queries, k, bank.oracle.METRIC_L2_F32, n_threads=16)
    assert np.array_equal(ref[0][0], copies[:k].astype(np.uint64)) and (ref[1][0] == 0).all()
    eng = GpuBruteForceEngine(d, "l2")
    eng.store_many_vectors(base)
    eng.build()
    eng.set_profiling(True)
    try:
        _check(eng, queries, k, ref, n, f"ties f32 l2 n={n} d={d} m={m}")
    finally:
        eng.close()


def test_staging_boundary_of_the_host_call(bank):
    """expann_search stages queries and results in pinned memory up to m * k = 16384 and copies plainly beyond:
    both sides of the boundary, one after the other on one handle, then k = 10 again"""
    eng, ref = bank.engine("gauss", 70001, 128, "l2"), bank.ref("gauss", 70001, 128, "l2")
    q = bank.queries("gauss", 128)
    for m, k in [(2, 8192), (4, 4096), (5, 4096), (16, 1024), (17, 1024), (17, 10), (100, 10)]:
        _check(eng, q[:m], k, ref, 70001, f"staging f32 l2 n=70001 d=128 m={m}")


def test_the_bound_on_k(bank):
    from expann_amd import _lib
    eng, ref = bank.engine("gauss", 20000, 128, "l2"), bank.ref("gauss", 20000, 128, "l2")
    q = bank.queries("gauss", 128)[:5]
    _check(eng, q, K_MAX, ref, 20000, "bound f32 l2 n=20000 d=128 m=5")
    for k in (K_MAX + 1, 2 * K_MAX):
        rc, ids, _, _, err = _search(eng, q, k)
        assert rc == _lib.ERR_UNSUPPORTED, (k, rc, err)
        assert (ids == 12345).all(), "a refused search wrote results"
        assert f"k <= {K_MAX}" in err, err
    _check(eng, q, 10, ref, 20000, "after the refusal f32 l2 n=20000 d=128 m=5")
