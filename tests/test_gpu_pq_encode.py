"""expann_pq_encode / expann_pq_train (expann_amd/csrc/pq_encode.hpp) against THE ENCODE RULE and THE TRAIN RULE restated
in NumPy (tests/test_pq_encode_abi.py).  Every comparison is exact: codes as bytes, codebooks as float32 bits."""
import numpy as np
import pytest

from test_pq_encode_abi import encode_rule, train_rule

pytestmark = pytest.mark.gpu

N = 2 * 256 + 37  # two workgroup tiles of rows and a ragged end
# dsub 33 is the first sub-vector longer than a tile chunk (32 columns): it and 40 take the streamed path
SHAPES = [(ncent, M, dsub) for ncent, Ms in ((256, (8, 24, 128)), (16, (16, 48, 256))) for M in Ms for dsub in (1, 3, 8, 33, 40)
          if M * dsub <= 4096]


def engine(cb, metric="l2"):
    from expann_amd import GpuBruteForceEngine
    M, ncent, dsub = cb.shape
    return GpuBruteForceEngine(M * dsub, metric, "pq8" if ncent == 256 else "pq4", codebooks=cb)


def packed(codes, ncent):
    from expann_amd import pack_pq4
    return codes if ncent == 256 else pack_pq4(codes)


def encoded(cb, x):
    eng = engine(cb)
    got = eng.encode(x)
    eng.close()
    return got


def encoded_on_device(eng, x, shape):
    import torch
    tx, tc = torch.from_numpy(x).cuda(), torch.zeros(shape, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.encode_device(tx.data_ptr(), len(x), tc.data_ptr(), 0)
    return tc.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def unpacked(rows, ncent):
    from expann_amd import unpack_pq4
    return rows if ncent == 256 else unpack_pq4(rows)


@pytest.mark.parametrize("ncent,M,dsub", SHAPES)
def test_encode_against_the_rule_host_and_device(ncent, M, dsub):
    rng = np.random.default_rng(1000 * M + 10 * dsub + ncent)
    cb = rng.standard_normal((M, ncent, dsub)).astype(np.float32)
    x = rng.standard_normal((N, M * dsub)).astype(np.float32)
    want = packed(encode_rule(x, cb), ncent)
    eng = engine(cb, "ip")  # (the rule is L2 whatever the metric)
    assert np.array_equal(eng.encode(x), want)
    assert np.array_equal(eng.encode(x[:1]), want[:1]) and eng.encode(x[:0]).shape == (0, want.shape[1])
    assert np.array_equal(encoded_on_device(eng, x, want.shape), want)
    assert eng.get_stat("pq_encode_launches") == 3 and eng.size() == 0
    eng.close()


def test_the_host_form_stages_in_pieces():
    """dim 4096: a piece is 4 096 rows, 4 396 rows take two; against the device form (one launch) and, at the seam, the rule"""
    rng = np.random.default_rng(6)
    cb = rng.standard_normal((128, 256, 32)).astype(np.float32)
    x = rng.standard_normal((4396, 4096)).astype(np.float32)
    eng = engine(cb)
    got = eng.encode(x)
    assert np.array_equal(got, encoded_on_device(eng, x, got.shape)) and eng.get_stat("pq_encode_launches") == 3
    eng.close()
    assert np.array_equal(got[4092:4100], encode_rule(x[4092:4100], cb)) and np.array_equal(got[-2:], encode_rule(x[-2:], cb))


@pytest.mark.parametrize("ncent,M,dsub", [(256, 8, 18), (256, 24, 40), (16, 16, 9), (16, 48, 40)])
def test_summation_order(ncent, M, dsub):
    """values over eight decades along j, and every odd centroid its even neighbour moved by a few ulps, so the argmin
    hangs on the last bits: a tree sum, a reversed sum, an FMA or an fp64 sum each change dozens of codes (counted with
    the restatement at these seeds: at least 49 of them)"""
    rng = np.random.default_rng(M + dsub)
    scale = (10.0 ** (np.arange(dsub) % 9 - 4)).astype(np.float32)
    cb = rng.standard_normal((M, ncent, dsub)).astype(np.float32) * scale
    cb[:, 1::2] = cb[:, 0::2] * (1 + rng.standard_normal((M, ncent // 2, dsub)).astype(np.float32) * np.float32(3e-7))
    x = (rng.standard_normal((N, M, dsub)).astype(np.float32) * scale).reshape(N, M * dsub)
    assert np.array_equal(encoded(cb, x), packed(encode_rule(x, cb), ncent))


@pytest.mark.parametrize("ncent,M,dsub", [(256, 8, 3), (16, 16, 8), (256, 8, 40)])
def test_ties_go_to_the_lower_centroid(ncent, M, dsub):
    rng = np.random.default_rng(3)
    cb = rng.standard_normal((M, ncent, dsub)).astype(np.float32)
    cb[:, ncent // 2:] = cb[:, :ncent // 2]
    pick = rng.integers(0, ncent, (N, M))
    x = cb[np.arange(M), pick].reshape(N, M * dsub)  # every row sits on a centroid, which exists twice
    assert np.array_equal(unpacked(encoded(cb, x), ncent), pick % (ncent // 2))


@pytest.mark.parametrize("ncent,M", [(256, 8), (16, 16)])
def test_ties_of_signed_zeros_and_of_a_midpoint(ncent, M):
    """dsub = 1.  Centroids 0 and 1 are -0.0 and +0.0: a zero row of either sign is at distance 0 from both and takes
    centroid 0.  Centroids 2 and 3 are 2 and 4 (the others far away): the row 3 is at distance 1 from both and takes 2."""
    cb = np.full((M, ncent, 1), 100.0, np.float32) + np.arange(ncent, dtype=np.float32)[None, :, None]
    cb[:, :4, 0] = [-0.0, 0.0, 2.0, 4.0]
    x = np.tile(np.array([[0.0], [-0.0], [3.0]], np.float32), (1, M))
    got = unpacked(encoded(cb, x), ncent)
    assert got.tolist() == [[0] * M, [0] * M, [2] * M] and np.array_equal(got, encode_rule(x, cb))


def test_pq4_packing():
    """M = 48: code 2 j in the low nibble of byte j; a swapped nibble or a shifted byte shows at every row"""
    from expann_amd import pack_pq4
    rng = np.random.default_rng(4)
    cb = rng.standard_normal((48, 16, 2)).astype(np.float32)
    x = rng.standard_normal((N, 96)).astype(np.float32)
    assert np.array_equal(encoded(cb, x), pack_pq4(encode_rule(x, cb)))


@pytest.mark.parametrize("iters", [0, 1, 4])
@pytest.mark.parametrize("ncent,M,dsub,n", [(256, 8, 1, 805), (256, 8, 3, 805), (256, 16, 8, 2085), (16, 16, 1, 805), (16, 32, 4, 805),
                                            (16, 16, 8, 2085)])
def test_train_against_the_rule(ncent, M, dsub, n, iters):
    from expann_amd import train_pq_codebooks
    X = np.random.default_rng(100 * M + dsub + n).standard_normal((n, M * dsub)).astype(np.float32)
    got = train_pq_codebooks(X, M, 8 if ncent == 256 else 4, iters)
    assert got.shape == (M, ncent, dsub) and np.array_equal(bits(got), bits(train_rule(X, M, ncent, iters)))


@pytest.mark.parametrize("ncent,M,dsub", [(256, 8, 2), (16, 16, 3)])
def test_empty_clusters_and_duplicate_initial_centroids(ncent, M, dsub):
    """three distinct vectors: duplicate initial centroids tie, the upper copies stay empty and keep their bits"""
    from expann_amd import train_pq_codebooks
    rng = np.random.default_rng(9)
    X = rng.standard_normal((3, M * dsub)).astype(np.float32)[rng.integers(0, 3, 900)]
    start, want = train_rule(X, M, ncent, 0), train_rule(X, M, ncent, 3)
    codes = encode_rule(X, want)
    empty = np.array([[not (codes[:, i] == c).any() for c in range(ncent)] for i in range(M)])
    assert empty.sum() >= M * (ncent - 3) and np.array_equal(bits(want[empty]), bits(start[empty]))
    assert np.array_equal(bits(train_pq_codebooks(X, M, 8 if ncent == 256 else 4, 3)), bits(want))


def test_sum_order_in_the_update():
    """16 centroids over 5 000 rows that span eight decades: a sequential float64 sum of hundreds of rows each.  (A float32
    sum shows here; another ORDER of the float64 sum shows only where the cast to float32 sits on a rounding boundary.)"""
    from expann_amd import train_pq_codebooks
    rng = np.random.default_rng(12)
    X = (rng.standard_normal((5000, 32)) * 10.0 ** rng.uniform(-4, 4, (5000, 1))).astype(np.float32)
    assert np.array_equal(bits(train_pq_codebooks(X, 16, 4, 2)), bits(train_rule(X, 16, 16, 2)))


@pytest.mark.parametrize("dtype,ncent,M,dsub", [("pq8", 256, 16, 8), ("pq4", 16, 32, 4)])
def test_end_to_end_from_fp32_rows(dtype, ncent, M, dsub):
    import test_gpu_pq
    import test_gpu_pq4
    from expann_amd import GpuBruteForceEngine, train_pq_codebooks
    rng = np.random.default_rng(21)
    rows = rng.standard_normal((2085, M * dsub)).astype(np.float32)
    queries = rng.standard_normal((9, M * dsub)).astype(np.float32)
    eng = GpuBruteForceEngine(M * dsub, "l2", dtype, codebooks=train_pq_codebooks(rows, M, 8 if ncent == 256 else 4, 4))
    eng.store_many_vectors(eng.encode(rows))
    eng.build()
    got = eng.query_k_batch(queries, 10)
    eng.close()
    cb = train_rule(rows, M, ncent, 4)
    codes = encode_rule(rows, cb)
    test_gpu_pq.same(got, (test_gpu_pq if ncent == 256 else test_gpu_pq4).reference(cb, codes, queries, 10, "l2"))

    def error(books):
        return float(((rows.reshape(-1, M, dsub) - books[np.arange(M), encode_rule(rows, books)]) ** 2).sum(axis=(1, 2)).mean())
    assert error(cb) < error(train_rule(rows, M, ncent, 0))
