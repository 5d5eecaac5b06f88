"""THE ENCODE RULE and THE TRAIN RULE of include/expann_hip.h restated in NumPy (what tests/test_gpu_pq_encode.py
compares the kernels with), and what needs no device: the refusals of expann_pq_train and the restatement itself on
an example worked by hand."""
import numpy as np
import pytest

INVALID_ARG = 1


def encode_rule(x, cb):
    """codes [n, M]: per (row, i, c) one float32 chain over j in order, then the first minimum."""
    M, ncent, dsub = cb.shape
    xs = np.asarray(x, np.float32).reshape(len(x), M, 1, dsub)
    D = np.zeros((len(x), M, ncent), np.float32)
    for j in range(dsub):
        t = xs[..., j] - cb[None, :, :, j]
        D = D + t * t
    return D.argmin(axis=2).astype(np.uint8)


def train_rule(X, M, ncent, iters):
    """codebooks [M, ncent, dsub]: rows floor(c n / ncent) first; then assignment and float64 means in row order
    (np.cumsum is the sequential sum), empty clusters left alone."""
    n, dim = X.shape
    dsub = dim // M
    cb = X[np.arange(ncent, dtype=np.int64) * n // ncent].reshape(ncent, M, dsub).transpose(1, 0, 2).copy()
    for _ in range(iters):
        codes = encode_rule(X, cb)
        for i in range(M):
            sub = X[:, i * dsub:(i + 1) * dsub].astype(np.float64)
            for c in range(ncent):
                mine = sub[codes[:, i] == c]
                if len(mine):
                    cb[i, c] = (np.cumsum(mine, axis=0)[-1] / np.float64(len(mine))).astype(np.float32)
    return cb


def test_the_rules_on_four_rows_worked_by_hand():
    """M = 2, dsub = 1, three centroids, rows (0, 1), (4, 1), (4, 5), (10, 5).  Init takes rows 0, 1, 2: centroids
    0, 4, 4 and 1, 1, 5.  Sub-quantiser 0: the 4s tie between centroids 1 and 2 and go to 1; so does 10 (36 = 36);
    centroid 2 is empty and stays 4; centroid 1 becomes (4 + 4 + 10) / 3 = 6.  Second round: the 4s are nearest to
    centroid 2 now, 10 stays with centroid 1, which becomes 10.  Sub-quantiser 1: the 1s tie between centroids 0 and 1
    and go to 0, centroid 1 stays empty, nothing moves."""
    X = np.array([[0, 1], [4, 1], [4, 5], [10, 5]], np.float32)
    assert train_rule(X, 2, 3, 0)[:, :, 0].tolist() == [[0, 4, 4], [1, 1, 5]]
    one = train_rule(X, 2, 3, 1)
    assert one[:, :, 0].tolist() == [[0, 6, 4], [1, 1, 5]]
    assert encode_rule(X, train_rule(X, 2, 3, 0)).tolist() == [[0, 0], [1, 0], [1, 2], [1, 2]]
    assert encode_rule(X, one).tolist() == [[0, 0], [2, 0], [2, 2], [1, 2]]
    assert train_rule(X, 2, 3, 2)[:, :, 0].tolist() == [[0, 10, 4], [1, 1, 5]]


@pytest.mark.parametrize("n,dim,M,bits,iters,null", [
    (1000, 128, 16, 5, 1, ""), (1000, 128, 16, 0, 1, ""),      # code_bits
    (1000, 100, 8, 8, 1, ""), (1000, 128, 24, 8, 1, ""),       # M does not divide dim
    (1000, 128, 8, 4, 1, ""), (1000, 8192, 8, 8, 1, ""),       # the limits of the dtype
    (255, 128, 16, 8, 1, ""), (15, 128, 16, 4, 1, ""),         # n < ncent
    (2 ** 24 + 1, 128, 16, 8, 1, ""), (1000, 128, 16, 8, 1001, ""),
    (1000, 128, 16, 8, 1, "rows"), (1000, 128, 16, 8, 1, "codebooks")])
def test_train_refuses_before_the_device(n, dim, M, bits, iters, null):
    from expann_amd import _lib
    L = _lib.load()
    buf = np.zeros(16, np.float32)  # (never read: every case is refused by value)
    rows, cb = (None if null == "rows" else buf.ctypes.data), (None if null == "codebooks" else buf.ctypes.data)
    assert L.expann_pq_train(0, rows, n, dim, M, bits, iters, cb) == INVALID_ARG
    assert b"expann_pq_train" in L.expann_last_error(None)
