"""CPU-side checks of the ranged (affine int8) graph walk: the new entry points exist and refuse NULL
handles, the Python surface validates its arguments before it asks for a device, and the numpy restatement
of the quantiser's convert -- the yardstick of tests/test_gpu_graph_ranged.py -- equals the oracle's bytes."""
import ctypes as C
import os

import numpy as np
import pytest

INVALID_ARG = 1


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_new_symbols_exist_and_refuse_null_handles(lib):
    from expann_amd import _lib
    for name in ("expann_graph_search_mode", "expann_graph_ranged_params", "expann_antitopo_set_compression"):
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name), name
    q = np.zeros((1, 64), np.float32)
    ids = np.zeros((1, 1), np.uint64)
    dists = np.zeros((1, 1), np.float32)
    for mode in (0, 1, 2, 3):
        assert lib.expann_graph_search_mode(None, q.ctypes.data, 1, 1, 1, mode, ids.ctypes.data, dists.ctypes.data,
                                            None) == INVALID_ARG
    s, o = C.c_float(), C.c_float()
    assert lib.expann_graph_ranged_params(None, C.byref(s), C.byref(o)) == INVALID_ARG
    for mode in (0, 2, 3):
        assert lib.expann_antitopo_set_compression(None, mode) == INVALID_ARG
    assert lib.expann_abi_version() == 2  # additive entry points only


def test_python_surface_checks_its_arguments_before_the_device():
    from expann_amd import AntitopoEngine
    with pytest.raises(ValueError, match="compression"):
        AntitopoEngine(16, 80, 1, 0, "int8", dim=128)
    with pytest.raises(ValueError, match="64"):
        AntitopoEngine(16, 80, 1, 0, "ranged", dim=80)
    eng = AntitopoEngine(16, 80, 1, 0, "ranged")  # (no dim yet: nothing is opened)
    assert eng.param_list()["compression_mode"] == "ranged"
    with pytest.raises(ValueError, match="compression"):
        eng.set_compression("uint8")
    with pytest.raises(ValueError, match="compression"):
        eng.set_compression(True)
    eng.set_compression("none")
    assert "compression_mode" not in eng.param_list() and eng.param_list()["use_compression"] == "0"
    eng.set_compression("cast")
    assert eng.param_list()["use_compression"] == "1"
    # True / False keep their meaning
    assert AntitopoEngine(16, 80, 1, 0, True).param_list()["use_compression"] == "1"
    assert AntitopoEngine(16, 80, 1, 0, False).param_list()["use_compression"] == "0"


def _dyadic_rows(rng):
    """Gaussian rows clipped to [-4, 4] with both ends present (scale_factor = 16, offset = 64, exactly), and
    rows whose components land exactly on every k + 0.5 after scaling"""
    x = np.clip(rng.standard_normal((300, 64)), -4, 4).astype(np.float32)
    x[0, 0], x[0, 1] = -4.0, 4.0
    halves = ((np.arange(128, dtype=np.float32) + 0.5) / 16 - 4).astype(np.float32)
    return np.concatenate([x, halves.reshape(2, 64), halves[::-1].reshape(2, 64)])


@pytest.mark.parametrize("data", ["gaussian", "halves"])
def test_numpy_convert_equals_the_oracle_quantiser(oracle, data):
    from graph_ranged_helpers import oracle_ranged_q8, ranged_convert
    rng = np.random.RandomState(300)
    x = rng.standard_normal((300, 64)).astype(np.float32) if data == "gaussian" else _dyadic_rows(rng)
    scale, offset, R = oracle_ranged_q8(oracle, x)
    assert np.isfinite(scale) and scale > 0
    if data == "halves":
        assert (scale, offset) == (16.0, 64.0)
        r = x[300:].astype(np.float64) * 16 + 64
        assert np.array_equal(r - np.floor(r), np.full(r.shape, 0.5))  # exactly on .5: rounds away from zero
        assert np.array_equal(R[300], np.minimum(np.arange(64) + 1, 127))
    assert R.min() == 0 and R.max() == 127
    assert np.array_equal(ranged_convert(x, scale, offset), R)
    # components outside the rows' range clamp
    far = np.array([x.min() - 10, x.max() + 10, -np.inf, np.inf], np.float32)
    assert ranged_convert(far, scale, offset).tolist() == [0, 127, 0, 127]
