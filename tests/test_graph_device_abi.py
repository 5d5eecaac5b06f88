"""CPU-side checks of the device-buffer graph search entry points (expann_graph_search_device and its
companions): they exist, and a NULL handle is refused before anything touches a device."""
import ctypes as C
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_null_handle_is_invalid_arg_in_all_six_calls(lib):
    from expann_amd import _lib
    out = C.c_uint64(7)
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    assert lib.expann_graph_search_device(None, p, 1, 1, 1, 0, p, p, None, None) == _lib.ERR_INVALID_ARG
    assert lib.expann_graph_sync(None) == _lib.ERR_INVALID_ARG
    assert lib.expann_graph_set_option(None, b"cand_capacity", 8) == _lib.ERR_INVALID_ARG
    assert lib.expann_graph_get_stat(None, b"redo_queries", C.byref(out)) == _lib.ERR_INVALID_ARG
    assert out.value == 7
    assert lib.expann_antitopo_query_device(None, p, 1, 1, p, p, None) == _lib.ERR_INVALID_ARG
    assert lib.expann_antitopo_sync(None) == _lib.ERR_INVALID_ARG


def test_null_handle_with_unknown_names(lib):
    from expann_amd import _lib
    out = C.c_uint64(0)
    assert lib.expann_graph_get_stat(None, b"no_such_stat", C.byref(out)) == _lib.ERR_INVALID_ARG
    assert lib.expann_graph_get_stat(None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.expann_graph_set_option(None, b"no_such_option", 0) == _lib.ERR_INVALID_ARG
    assert lib.expann_graph_set_option(None, None, 0) == _lib.ERR_INVALID_ARG


def test_python_surface_has_the_device_calls():
    from expann_amd import AntitopoEngine
    assert callable(AntitopoEngine.query_many_device) and callable(AntitopoEngine.sync)
    assert "padded" in AntitopoEngine.query_many_device.__doc__
