"""CPU-side checks of the k-way merge's boundary: the argument checks of expann_merge_topk_device /
expann_merge_topk_strided_device that return before any device call, and the generator and the numpy reference
(tests/merge_helpers.py) that the GPU test of the kernel relies on."""
import os

import numpy as np
import pytest

from merge_helpers import PAD_ID, lists_are_well_formed, make_lists, merge_reference, staged


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_argument_checks_return_before_any_device_call(lib):
    from expann_amd import _lib
    buf = np.zeros(64, np.uint64)                  # (host memory: a call that got past the checks would not see it)
    p = buf.ctypes.data
    plain, strided = lib.expann_merge_topk_device, lib.expann_merge_topk_strided_device
    for n_lists, m, k in [(0, 1, 1), (65, 1, 1), (1, 1, 0), (0, 0, 1), (2, 0, 0)]:
        assert plain(0, p, p, n_lists, m, k, p, p, None) == _lib.ERR_INVALID_ARG, (n_lists, m, k)
        assert strided(0, p, p, 8, 8, n_lists, m, k, p, p, None) == _lib.ERR_INVALID_ARG, (n_lists, m, k)
    assert b"1 <= n_lists <= 64" in lib.expann_last_error(None)
    for null in range(4):
        a = [p] * 4
        a[null] = None
        assert plain(0, a[0], a[1], 2, 1, 1, a[2], a[3], None) == _lib.ERR_INVALID_ARG, null
        assert strided(0, a[0], a[1], 8, 8, 2, 1, 1, a[2], a[3], None) == _lib.ERR_INVALID_ARG, null
    # no queries: nothing to do, whatever the device
    assert plain(0, p, p, 1, 0, 1, p, p, None) == _lib.OK
    assert plain(0, p, p, 64, 0, 1000, p, p, None) == _lib.OK
    assert strided(0, p, p, 8, 16, 64, 0, 8, p, p, None) == _lib.OK


@pytest.mark.parametrize("scores", ["gauss", "neg", "eight"])
def test_generated_lists_are_ascending_with_padding_at_the_tail(scores):
    rng = np.random.RandomState(3)
    n_real = rng.randint(0, 18, size=(5, 9))
    n_real[2] = 0                                  # a list that is all padding
    for kwargs in [{}, {"n_real": n_real}, {"n_real": 11, "inf_tail": 3}, {"dup": (6, [0, 2, 4])},
                   {"n_real": np.array([17, 0, 3, 17, 1])}, {"id_base": 2 ** 40, "id_step": 2 ** 20}]:
        ids, d = make_lists(rng, 5, 9, 17, scores=scores, **kwargs)
        assert ids.shape == d.shape == (5, 9, 17) and ids.dtype == np.uint64 and d.dtype == np.float32
        assert lists_are_well_formed(ids, d), kwargs
        want = np.broadcast_to(kwargs["n_real"][:, None] if np.ndim(kwargs.get("n_real")) == 1
                               else kwargs.get("n_real", 17), (5, 9))
        assert np.array_equal((ids != PAD_ID).sum(-1), want), kwargs
        if "dup" in kwargs:                        # the shared pairs are in each of the lists named
            for q in range(9):
                pairs = [set(zip(ids[g, q].tolist(), d[g, q].tolist())) for g in (0, 2, 4)]
                assert len(pairs[0] & pairs[1] & pairs[2]) == 6
        if "inf_tail" in kwargs:
            assert (np.isinf(d) & (ids != PAD_ID)).sum() == 5 * 9 * 3
    if scores == "eight":
        assert len(np.unique(d[ids != PAD_ID])) <= 8


def test_the_checker_rejects_what_the_generator_avoids():
    rng = np.random.RandomState(4)
    ids, d = make_lists(rng, 2, 3, 8, n_real=6)
    assert lists_are_well_formed(ids, d)
    for poke in (lambda i, x: x.__setitem__((0, 0, 0), np.nan), lambda i, x: x.__setitem__((0, 0, 0), -0.0),
                 lambda i, x: x.__setitem__((1, 2, 3), -1e30),                  # descending
                 lambda i, x: i.__setitem__((1, 1, 2), PAD_ID),                 # padding in the middle
                 lambda i, x: x.__setitem__((0, 1, 7), 1.0)):                   # a padding id with a finite score
        i2, d2 = ids.copy(), d.copy()
        poke(i2, d2)
        assert not lists_are_well_formed(i2, d2)


@pytest.mark.parametrize("n_lists,m,k", [(1, 4, 9), (3, 7, 10), (8, 5, 64), (64, 2, 65)])
def test_reference_agrees_with_the_sharded_tests_merge(n_lists, m, k):
    """tests/test_sharded_gloo.py's _merge_np, query by query, on lists without duplicates"""
    from test_sharded_gloo import _merge_np
    rng = np.random.RandomState(n_lists)
    n_real = rng.randint(0, k + 1, size=(n_lists, m))
    for scores in ("gauss", "neg", "eight"):
        ids, d = make_lists(rng, n_lists, m, k, scores=scores, n_real=n_real)
        ri, rd = merge_reference(ids, d)
        oi, od = _merge_np(ids, d)
        assert np.array_equal(ri, oi.view(np.uint64)) and np.array_equal(rd.view(np.uint32), od.view(np.uint32))
        # the result is itself a well-formed list holding min(k, real entries) of them
        assert lists_are_well_formed(ri[None], rd[None])
        assert np.array_equal((ri != PAD_ID).sum(-1), np.minimum(k, n_real.sum(0)))


def test_launch_condition():
    assert staged(64, 64) and staged(8, 512) and staged(1, 4096)
    assert not staged(64, 65) and not staged(8, 513) and not staged(3, 2048) and not staged(64, 1000)
