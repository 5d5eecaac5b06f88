"""The ranged graph walk (expann_graph_search_mode, mode 2: bottom layer over the rows' affine int8 bytes,
fp32 re-score) against the existing oracle, composed as tests/graph_ranged_helpers.py describes: ids, distance
bits and distance-evaluation counts must be equal.  m = 48 queries, k = 10, ef in {10, 40}."""
import ctypes as C

import numpy as np
import pytest

M_Q, K, EFS = 48, 10, (10, 40)
INVALID_ARG, UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    return _lib.load()


def _queries(rng, rows, draw):
    """44 queries like the rows, 3 with components far outside the rows' range (they clamp), 1 equal to a row"""
    q = draw(M_Q)
    q[44:47] *= 3.0
    q[44, 0], q[45, 1] = rows.min() - 5.0, rows.max() + 5.0
    q[47] = rows[rng.randint(len(rows))]
    return np.ascontiguousarray(q, dtype=np.float32)


def _check_composition(lib, oracle, tmp_path, rows, q):
    """serial build of `rows`, layer 0 only on both sides; mode 2 == the composed oracle"""
    from graph_ranged_helpers import (build_layer0, graph_create_layer0, ranged_convert, ranged_expected,
                                      search_mode)
    sv, lists0 = build_layer0(lib, rows, tmp_path)
    scale, offset, want = ranged_expected(oracle, tmp_path, rows, lists0, sv, q, K, EFS)
    h = graph_create_layer0(lib, rows, lists0, sv)
    try:
        s, o = C.c_float(), C.c_float()
        assert lib.expann_graph_ranged_params(h, C.byref(s), C.byref(o)) == 0, lib.expann_graph_last_error(h)
        got = np.array([s.value, o.value], np.float32)
        assert np.array_equal(got.view(np.uint32), np.array([scale, offset], np.float32).view(np.uint32)), (got, scale, offset)
        for ef in EFS:
            rc, ids, dists, dc = search_mode(lib, h, q, K, ef, 2)
            assert rc == 0, lib.expann_graph_last_error(h)
            oids, od, odc = want[ef]
            assert np.array_equal(ids, oids), ef
            assert np.array_equal(dists.view(np.uint32), od.view(np.uint32)), ef
            assert np.array_equal(dc.astype(np.uint64), odc), ef
    finally:
        lib.expann_graph_destroy(h)
    return ranged_convert(q, scale, offset)


@pytest.mark.gpu
@pytest.mark.parametrize("normalise", [False, True])
@pytest.mark.parametrize("n,d", [(3000, 64), (3000, 128), (2000, 256), (1500, 832), (1500, 192), (600, 1024)])
def test_ranged_walk_equals_the_composed_oracle(lib, oracle, tmp_path, n, d, normalise):
    """Gaussian rows, and the same L2-normalised (what take_norms=True stores): one dword per lane (64), 16 / 8 / 4
    rows in flight (128 / 256 / 832, the last no multiple of 128), the run-time-dim instance (192, 1024)"""
    rng = np.random.RandomState(1000 * d + normalise)

    def draw(cnt):
        x = rng.standard_normal((cnt, d)).astype(np.float32)
        if normalise:
            x = (x / np.sqrt(np.einsum("ij,ij->i", x, x, dtype=np.float32))[:, None]).astype(np.float32)
        return x
    rows = draw(n)
    q = _queries(rng, rows, draw)
    qb = _check_composition(lib, oracle, tmp_path, rows, q)
    assert qb[44, 0] == 0 and qb[45, 1] == 127  # the out-of-range components did clamp
    assert len(np.unique(qb[:44])) > 32          # and the bytes are not the cast's garbage


@pytest.mark.gpu
def test_ranged_walk_on_integer_rows_in_0_127(lib, oracle, tmp_path):
    """SIFT-like integers clipped to [0, 127] with both ends present: min and max are exact, scale_factor = 128 / 127,
    so the quantiser is NOT the identity on them; queries carry fractional parts"""
    rng = np.random.RandomState(127)
    n, d = 3000, 128

    def draw(cnt):
        return np.clip(np.round(np.abs(rng.standard_normal((cnt, d))) * 40.0), 0, 127).astype(np.float32)
    rows = draw(n)
    assert rows.min() == 0 and rows.max() == 127
    q = np.minimum(127.5, draw(M_Q) + rng.uniform(0, 0.99, size=(M_Q, d))).astype(np.float32)
    q[47] = rows[5]
    _check_composition(lib, oracle, tmp_path, rows, q)


@pytest.mark.gpu
def test_ranged_walk_on_massive_ties(lib, oracle, tmp_path):
    """two distinct values per component: the bytes are 0 and 127, every integer distance is a multiple of 127^2
    and most queue comparisons are ties -- the order is libstdc++'s (tests/test_heap_pin.py for the uint8 walk)"""
    rng = np.random.RandomState(2)
    n, d = 2000, 128
    rows = (rng.randint(0, 2, size=(n, d)) * 0.5 - 0.25).astype(np.float32)
    q = (rng.randint(0, 2, size=(M_Q, d)) * 0.5 - 0.25).astype(np.float32)
    qb = _check_composition(lib, oracle, tmp_path, rows, q)
    assert set(np.unique(qb)) == {0, 127}
    one = ((qb[0].astype(np.int64) - (rows > 0) * 127) ** 2).sum(1)
    assert len(np.unique(one)) < n // 10


@pytest.mark.gpu
def test_python_surface_leaves_the_reference_modes_bit_exact(oracle, tmp_path):
    """AntitopoEngine(..., "ranged"), all layers: the ranged answers carry the exact fp32 distances of their ids;
    set_compression("none") / ("cast") on the same handle equal the oracle's fp32 / uint8 walk of the saved file,
    and the file is the one an engine created with False writes.
    Rows are Gaussian with mean 100 and sigma 20, clipped to [0, 255]: the uint8 cast of a negative float is
    undefined behaviour in the reference and the oracle (x86 wraps, the device saturates), so the cast mode can
    only be compared where it is defined."""
    from expann_amd import AntitopoEngine
    from graph_helpers import check_against_oracle
    rng = np.random.RandomState(3000)
    n, d = 3000, 128

    def draw(cnt):
        return np.clip(rng.standard_normal((cnt, d)) * 20.0 + 100.0, 0, 255).astype(np.float32)
    rows, q = draw(n), draw(M_Q)
    eng = AntitopoEngine(16, 80, 1, 0, "ranged", dim=d)
    eng.store_many_vectors(rows, False)
    eng.build()
    idx = str(tmp_path / "ranged.index")
    eng.save_index(idx)
    assert eng.param_list()["compression_mode"] == "ranged"
    for ef in EFS:
        eng.set_ef_search(ef)
        ids, dists = eng.query_many(q, K)
        assert ids.max() < n
        want = np.array([[oracle.l2_f32(q[i], rows[int(j)]) for j in ids[i]] for i in range(M_Q)], np.float32)
        assert np.array_equal(dists.view(np.uint32), want.view(np.uint32)), ef
    eng.set_compression("none")
    check_against_oracle(oracle, {False: eng}, idx, q, K, EFS, compressions=(False,))
    eng.set_compression("cast")
    check_against_oracle(oracle, {True: eng}, idx, q, K, EFS, compressions=(True,))
    # the mode is a run-time property: the same bytes whichever is set (the sticky ef_search is recorded by now)
    eng.save_index(str(tmp_path / "as_cast.index"))
    eng.set_compression("ranged")
    eng.save_index(str(tmp_path / "as_ranged.index"))
    assert open(tmp_path / "as_cast.index", "rb").read() == open(tmp_path / "as_ranged.index", "rb").read()
    plain = AntitopoEngine(16, 80, 1, 0, False, dim=d)
    plain.store_many_vectors(rows, False)
    plain.save_index(str(tmp_path / "plain.index"))
    assert open(idx, "rb").read() == open(tmp_path / "plain.index", "rb").read()
    eng.close()
    plain.close()


def _ring(lib, vec):
    n, d = vec.shape
    off = np.arange(n + 1, dtype=np.uint64)
    nb = ((np.arange(n) + 1) % n).astype(np.uint32)
    h = C.c_void_p()
    assert lib.expann_graph_create(d, 0, vec.ctypes.data, n, 1, 0, off.ctypes.data, nb.ctypes.data, C.byref(h)) == 0
    return h


@pytest.mark.gpu
def test_refusals_leave_the_handle_usable(lib):
    from graph_ranged_helpers import search_mode
    rng = np.random.RandomState(80)
    n = 64

    def fp32_still_answers(h, vec):
        rc, ids, dists, _ = search_mode(lib, h, vec[:2], 4, 8, 0)
        assert rc == 0, lib.expann_graph_last_error(h)
        assert ids[0, 0] == 0 and ids[1, 0] == 1 and dists[0, 0] == 0 and dists[1, 0] == 0

    vec = rng.standard_normal((n, 80)).astype(np.float32)  # a dim the byte walks do not take
    h = _ring(lib, vec)
    assert search_mode(lib, h, vec[:2], 4, 8, 3)[0] == INVALID_ARG
    assert b"mode" in lib.expann_graph_last_error(h)
    fp32_still_answers(h, vec)
    assert search_mode(lib, h, vec[:2], 4, 8, -1)[0] == INVALID_ARG
    assert search_mode(lib, h, vec[:2], 4, 8, 2)[0] == UNSUPPORTED
    assert b"64" in lib.expann_graph_last_error(h)
    fp32_still_answers(h, vec)
    s, o = C.c_float(), C.c_float()
    assert lib.expann_graph_ranged_params(h, C.byref(s), C.byref(o)) == UNSUPPORTED
    fp32_still_answers(h, vec)
    lib.expann_graph_destroy(h)

    const = np.full((n, 64), 3.0, np.float32)  # max == min: scale_factor = 128 / 0
    h = _ring(lib, const)
    for _ in range(2):  # (the verdict is remembered)
        assert search_mode(lib, h, const[:2], 4, 8, 2)[0] == INVALID_ARG
        assert b"scale_factor" in lib.expann_graph_last_error(h)
    assert lib.expann_graph_ranged_params(h, C.byref(s), C.byref(o)) == INVALID_ARG
    rc, ids, dists, _ = search_mode(lib, h, const[:2], 4, 8, 0)
    assert rc == 0 and (ids < n).all() and (dists == 0).all()
    lib.expann_graph_destroy(h)

    e = C.c_void_p()
    assert lib.expann_antitopo_create(80, 0, 16, 80, 1, 0, 0, C.byref(e)) == 0
    assert lib.expann_antitopo_set_compression(e, 2) == INVALID_ARG
    assert lib.expann_antitopo_set_compression(e, 3) == INVALID_ARG
    assert lib.expann_antitopo_set_compression(e, 0) == 0
    lib.expann_antitopo_destroy(e)
