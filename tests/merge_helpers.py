"""Helpers of the k-way merge tests (expann_merge_topk_device / _strided_device): a generator of synthetic
per-shard result lists and the numpy statement of what the merge must return.  Imported by the CPU test of the
helpers themselves and by the GPU test that drives the kernel."""
import numpy as np

PAD_ID = np.uint64(2 ** 64 - 1)


def make_lists(rng, n_lists, m, k, scores="gauss", n_real=None, id_base=0, id_step=7, dup=None, inf_tail=0):
    """(ids[n_lists, m, k] uint64, dists[n_lists, m, k] float32): every list ascending by (score, id) and padded at
    the tail with (+inf, UINT64_MAX), as a search leaves it.

    scores    "gauss" (both signs), "neg" (all negative, as inner product scores them) or "eight" (drawn from eight
              distinct values: equal scores with different ids within and across lists)
    n_real    real entries per list: an int, or an array that broadcasts to [n_lists, m]; default k (no padding)
    id_base   ids are id_base + id_step * (a permutation of 0 .. n_lists * k - 1 per query): distinct across lists
    dup       (count, lists): `count` of the real (score, id) pairs of list lists[0] -- any of them, drawn before
              the lists are sorted -- replace as many pairs of each other list named: the same pair present in
              several lists
    inf_tail  the last `inf_tail` real entries of every list score +inf (real ids, ahead of the padding)

    Two inputs are never generated, because a search cannot produce them and the kernel's order and numpy's differ
    on them: NaN scores, and zeros of mixed sign (the kernel orders by the float's bits, -0.0 before +0.0; numpy
    orders by value and takes them for equal).  Everywhere else the two orders agree.  Every zero is +0.0."""
    shape = (n_lists, m, k)
    if scores == "gauss":
        d = rng.standard_normal(shape) * 100.0
    elif scores == "neg":
        d = -np.abs(rng.standard_normal(shape) * 100.0) - 1.0
    elif scores == "eight":
        d = rng.choice(np.array([-3.5, -1.0, 0.0, 0.25, 1.0, 2.0, 1e10, 3e38]), size=shape)
    else:
        raise ValueError(scores)
    d = d.astype(np.float32) + np.float32(0.0)            # (-0.0 + 0.0 = +0.0)
    perm = np.argsort(rng.rand(m, n_lists * k), axis=1).astype(np.uint64)
    ids = (np.uint64(id_base) + np.uint64(id_step) * perm).reshape(m, n_lists, k).transpose(1, 0, 2).copy()
    real = np.asarray(k if n_real is None else n_real, dtype=np.int64)
    if real.ndim == 1:                                     # one count per list
        real = real[:, None]
    real = np.broadcast_to(real, (n_lists, m))
    assert real.min() >= 0 and real.max() <= k
    if dup is not None:
        count, lists = dup
        assert count <= min(int(real[g].min()) for g in lists)
        for g in lists[1:]:
            ids[g, :, :count] = ids[lists[0], :, :count]
            d[g, :, :count] = d[lists[0], :, :count]
    pos = np.arange(k)[None, None, :]
    if inf_tail:
        d[(pos < real[:, :, None]) & (pos >= real[:, :, None] - inf_tail)] = np.inf
    pad = pos >= real[:, :, None]
    d[pad] = np.inf
    ids[pad] = PAD_ID
    order = np.lexsort((ids, d), axis=-1)
    return np.take_along_axis(ids, order, -1), np.take_along_axis(d, order, -1)


def lists_are_well_formed(ids, dists):
    """every list ascending by (score, id), padding (+inf, UINT64_MAX) only at the tail, no NaN, no -0.0"""
    if np.isnan(dists).any() or (np.signbit(dists) & (dists == 0)).any():
        return False
    pad = ids == PAD_ID
    if not np.isinf(dists[pad]).all() or (dists[pad] < 0).any():
        return False
    if (pad[..., :-1] & ~pad[..., 1:]).any():              # a real entry behind a padding one
        return False
    a_d, b_d, a_i, b_i = dists[..., :-1], dists[..., 1:], ids[..., :-1], ids[..., 1:]
    return bool(((a_d < b_d) | ((a_d == b_d) & (a_i <= b_i))).all())


def merge_reference(ids, dists):
    """the k smallest (score, id) of the n_lists * k entries of every query: numpy's lexsort((ids, scores))[:k]"""
    n_lists, m, k = ids.shape
    fi = ids.transpose(1, 0, 2).reshape(m, n_lists * k)
    fd = dists.transpose(1, 0, 2).reshape(m, n_lists * k)
    order = np.lexsort((fi, fd), axis=-1)[:, :k]
    return np.take_along_axis(fi, order, -1), np.take_along_axis(fd, order, -1)


def staged(n_lists, k):
    """which instance of merge_topk_kernel a call launches: the lists of a query are staged in LDS while their
    12-byte entries fit 48 KiB"""
    return n_lists * k * 12 <= 49152
