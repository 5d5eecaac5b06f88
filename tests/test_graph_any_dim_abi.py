"""CPU-side checks of the graph path's dim range (any multiple of 16 up to 4096; the uint8 walk needs a
multiple of 64): expann_graph_create, expann_graph_build_batched and expann_antitopo_create enforce the
limits before they look for a device."""
import ctypes as C
import os

import numpy as np
import pytest

OK, INVALID_ARG, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 5


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _graph_create(lib, dim):
    """a valid two-vertex, one-layer graph at `dim`"""
    n = 2
    vec = np.zeros((n, dim), np.float32)
    off = np.array([0, 1, 2], np.uint64)
    nb = np.array([1, 0], np.uint32)
    h = C.c_void_p()
    rc = lib.expann_graph_create(dim, 0, vec.ctypes.data, n, 1, 0, off.ctypes.data, nb.ctypes.data, C.byref(h))
    if h.value:
        lib.expann_graph_destroy(h)
    return rc


def _build_batched(lib, dim):
    """arguments that pass every other check: 4 vertices, the first 2 built"""
    n, M, M0 = 4, 2, 4
    vec = np.zeros((n, dim), np.float32)
    lv = np.zeros(n, np.uint8)
    up = np.full(n, -1, np.int32)
    ids0 = np.zeros((n, M0), np.uint32)
    d0 = np.zeros((n, M0), np.float32)
    deg0 = np.zeros(n, np.uint32)
    ml, sv = C.c_uint32(1), C.c_uint32(0)
    sz = C.c_size_t
    return lib.expann_graph_build_batched(
        C.c_int(dim), C.c_int(0), C.c_void_p(vec.ctypes.data), sz(n), C.c_void_p(lv.ctypes.data), sz(2),
        C.byref(ml), C.byref(sv), sz(M), sz(M0), sz(16), sz(0), C.c_float(0.5), C.c_float(0.0), sz(0),
        C.c_void_p(ids0.ctypes.data), C.c_void_p(d0.ctypes.data), C.c_void_p(deg0.ctypes.data), sz(M0),
        C.c_void_p(up.ctypes.data), sz(0), sz(0), None, None, None, sz(M), None)


def _antitopo_create(lib, dim, use_compression):
    h = C.c_void_p()
    rc = lib.expann_antitopo_create(dim, 0, 16, 80, 1, 0, use_compression, C.byref(h))
    if h.value:
        lib.expann_antitopo_destroy(h)
    return rc


def test_graph_create_dim_over_4096_is_unsupported_before_any_device_check(lib):
    assert _graph_create(lib, 4112) == UNSUPPORTED
    assert b"4096" in lib.expann_graph_last_error(None)
    assert _graph_create(lib, 8192) == UNSUPPORTED


def test_graph_build_batched_dim_over_4096_is_unsupported(lib):
    assert _build_batched(lib, 4112) == UNSUPPORTED
    assert b"4096" in lib.expann_graph_last_error(None)


def test_antitopo_create_limits(lib):
    assert _antitopo_create(lib, 4160, 0) == UNSUPPORTED
    assert b"4096" in lib.expann_antitopo_last_error(None)
    # fp32 engines take any multiple of 16: no device here -> NO_DEVICE, with one -> OK
    assert _antitopo_create(lib, 48, 0) in (OK, NO_DEVICE)
    assert _antitopo_create(lib, 4096, 0) in (OK, NO_DEVICE)
    # the uint8 walk works in 64-dim blocks
    assert _antitopo_create(lib, 48, 1) == INVALID_ARG
    assert _antitopo_create(lib, 1536, 1) in (OK, NO_DEVICE)


def test_dim_not_a_multiple_of_16_stays_invalid(lib):
    assert _graph_create(lib, 100) == INVALID_ARG
    assert _build_batched(lib, 100) == INVALID_ARG
    assert _antitopo_create(lib, 100, 0) == INVALID_ARG
    assert _antitopo_create(lib, 4100, 0) == INVALID_ARG


def test_python_engine_names_the_limit():
    from expann_amd import AntitopoEngine
    with pytest.raises(ValueError, match="4096"):
        AntitopoEngine(16, 80, 1, 0, False, dim=4160)
