"""expann_set_base_device with every derived copy of the old rows alive: one handle is moved from rows A to rows B
and back, and after each move every search must answer for the rows in force -- ids equal to the CPU oracle's and
distances equal as uint32 bit patterns.  A copy of the old rows that survived the move (the fp16 copy, the bf16
planes, the int8 copies, the uint8 shadow, a filter's masked row terms, the groups' row lists) would answer for
the old rows, or with the old row count: A and B differ in both.  The workspace, the options and the profiling
state are the handle's and stay."""
import numpy as np
import pytest

from row_groups_helpers import ANY, expected, expected_grouped, same

pytestmark = pytest.mark.gpu

D, M, K = 128, 96, 10
# (option settings, in order) of the four searches: the fp16 copy, the bf16 planes, the int8 filter's copies where
# the rows support it (fp32 L2 d = 128 from 32 768 rows on), the planner's own choice
FORMS = [{"scan_kernel": 4, "i8_filter": 1}, {"scan_kernel": 3, "i8_filter": 1}, {"scan_kernel": 0, "i8_filter": 2},
         {"scan_kernel": 0, "i8_filter": 1}]
LABELS = [5, 0x80000001, 77]
I8F = "scan_gemm_i8w<128,F32L2>"


@pytest.fixture(scope="module")
def gpu():
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_device_count() >= 1, "these tests need a HIP device"
    return L


def _integer_rows(rng, n):
    return rng.randint(0, 256, size=(n, D)).astype(np.float32)


def _case(oracle, rows, queries, seed):
    """rows on the device, and what the oracle answers for them: plainly, under a filter of every third row, and
    grouped with three labels (a few queries name ANY: every row)"""
    import torch
    n = rows.shape[0]
    allow = np.arange(n) % 3 == 0
    rng = np.random.RandomState(seed)
    groups = np.asarray(LABELS, np.uint32)[rng.randint(0, 3, n)]
    qg = np.asarray(LABELS + [ANY], np.uint32)[rng.randint(0, 4, M)]
    return {"rows": rows, "n": n, "dev": torch.from_numpy(rows).to(torch.device("cuda", 0)), "queries": queries,
            "allow": allow, "groups": groups, "qg": qg,
            "plain": oracle.brute_force(rows, queries, K, oracle.METRIC_L2_F32, n_threads=8),
            "filtered": expected(oracle, rows, queries, K, allow),
            "grouped": expected_grouped(oracle, rows, groups, queries, qg, K)}


def _rebase(eng, c):
    import torch
    torch.cuda.synchronize()
    eng.set_base_device(c["dev"].data_ptr(), c["n"], 0)
    assert eng.get_stat("filter_active") == 0 and eng.get_stat("groups_active") == 0
    assert eng.get_stat("filter_rows") == c["n"] and eng.get_stat("group_count") == 0
    assert eng.get_stat("base_bytes") == c["n"] * D * 4


def _search_every_way(eng, c, what):
    """every form plainly, then grouped, then under the filter; the groups and the filter are left in force"""
    def forms():
        for opts in FORMS:
            for name, v in opts.items():
                eng.set_option(name, v)
            yield (what, opts)
    for tag in forms():
        same(eng.query_k_batch(c["queries"], K), c["plain"], ("plain",) + tag)
    eng.set_row_groups(c["groups"])
    for tag in forms():
        same(eng.query_k_batch(c["queries"], K, groups=c["qg"]), c["grouped"], ("grouped",) + tag)
    eng.set_row_filter(c["allow"])
    assert eng.get_stat("filter_active") == 1 and eng.get_stat("groups_active") == 1
    assert eng.get_stat("filter_rows") == int(c["allow"].sum())
    for tag in forms():
        same(eng.query_k_batch(c["queries"], K), c["filtered"], ("filtered",) + tag)


def test_rebase_fp32_rows_with_every_copy_alive(gpu, oracle):
    """8 192 integer-valued rows, 12 288 Gaussian rows, and back: n >= 4 096 keeps the matrix-core forms eligible"""
    from expann_amd import GpuBruteForceEngine
    rng = np.random.RandomState(4242)
    a = _case(oracle, _integer_rows(rng, 8192), _integer_rows(rng, M), 1)
    b = _case(oracle, rng.standard_normal((12288, D)).astype(np.float32),
              rng.standard_normal((M, D)).astype(np.float32), 2)
    assert not np.array_equal(a["plain"][0], b["plain"][0])
    eng = GpuBruteForceEngine(D, "l2")
    eng.set_profiling(True)
    for c, what in ((a, "A"), (b, "B"), (a, "A again")):
        _rebase(eng, c)
        _search_every_way(eng, c, what)
    # the forced forms did run (the profile names the last full scan), on the handle that was moved twice
    eng.set_row_filter(None)
    eng.set_row_groups(None)
    for kernel, name in ((4, "scan_gemm_f16"), (3, "scan_gemm_bf16x3")):
        eng.set_option("scan_kernel", kernel)
        eng.get_profile()
        same(eng.query_k_batch(a["queries"], K), a["plain"], name)
        assert eng.get_profile()["scan_kernel"].startswith(name)
    eng.close()


def test_rebase_rows_that_carry_the_uint8_shadow_and_the_int8_filter(gpu, oracle):
    """the two copies that need more rows: 65 536 integer-valued rows searched with integer queries make the uint8
    shadow handle, 69 632 Gaussian rows searched with "i8_filter" 2 the int8 filter's copies; each is alive when
    the other rows arrive"""
    from expann_amd import GpuBruteForceEngine
    rng = np.random.RandomState(4343)
    rows_a, q_a = _integer_rows(rng, 65536), _integer_rows(rng, M)
    rows_b, q_b = rng.standard_normal((69632, D)).astype(np.float32), rng.standard_normal((M, D)).astype(np.float32)
    a = {"rows": rows_a, "n": 65536, "queries": q_a, "plain": oracle.brute_force(rows_a, q_a, K, oracle.METRIC_L2_F32, n_threads=8)}
    b = {"rows": rows_b, "n": 69632, "queries": q_b, "plain": oracle.brute_force(rows_b, q_b, K, oracle.METRIC_L2_F32, n_threads=8)}
    import torch
    for c in (a, b):
        c["dev"] = torch.from_numpy(c["rows"]).to(torch.device("cuda", 0))
    eng = GpuBruteForceEngine(D, "l2")
    eng.set_profiling(True)
    eng.set_option("i8_filter", 2)
    for c, what in ((a, "A"), (b, "B"), (a, "A again"), (b, "B again")):
        _rebase(eng, c)
        eng.get_profile()
        for again in range(2):   # (the second search finds the copies built)
            same(eng.query_k_batch(c["queries"], K), c["plain"], (what, again))
            kernel = eng.get_profile()["scan_kernel"]
            if c is a:
                assert kernel.startswith(("scan_gemm_i8w", "scan_gemm_i8q")) and kernel != I8F, (what, kernel)
            else:
                assert kernel == I8F, (what, kernel)
    eng.close()


def test_rebase_uint8_rows(gpu, oracle):
    """the derived copies of an 8-bit handle (row terms, the padded int8 copy): "scan_kernel" 2 and 5 on 8 192 rows,
    then on 12 288 other rows, and back"""
    import torch
    from expann_amd import GpuBruteForceEngine
    rng = np.random.RandomState(4444)
    cases = []
    for n in (8192, 12288):
        rows = rng.randint(0, 256, size=(n, D)).astype(np.uint8)
        queries = rng.randint(0, 256, size=(M, D)).astype(np.float32)
        cases.append((rows, torch.from_numpy(rows).to(torch.device("cuda", 0)), queries,
                      oracle.brute_force(rows, queries, K, oracle.METRIC_L2_U8, n_threads=8)))
    eng = GpuBruteForceEngine(D, "l2", "u8")
    for i in (0, 1, 0):
        rows, dev, queries, want = cases[i]
        torch.cuda.synchronize()
        eng.set_base_device(dev.data_ptr(), rows.shape[0], 0)
        assert eng.get_stat("base_bytes") == rows.shape[0] * D
        for kernel in (2, 5):
            eng.set_option("scan_kernel", kernel)
            same(eng.query_k_batch(queries, K), want, (i, kernel))
    eng.close()
