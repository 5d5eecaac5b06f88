"""The append calls at the C ABI, as far as they go without a device: the symbols exist with their prototypes, and a
NULL handle is EXPANN_ERR_INVALID_ARG before anything else is looked at."""
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


def test_a_null_handle_is_an_invalid_argument(lib):
    rows = (C.c_float * 128)()
    assert lib.expann_append(None, rows, 1) == 1
    assert lib.expann_append(None, None, 0) == 1
    assert lib.expann_append_device(None, rows, 1, None) == 1
    assert lib.expann_reserve(None, 1000) == 1
    assert lib.expann_reserve(None, 0) == 1


def test_the_engine_offers_the_calls():
    from expann_amd import GpuBruteForceEngine, _lib
    for name in ("append", "append_device", "reserve"):
        assert callable(getattr(GpuBruteForceEngine, name))
    for name in ("expann_append", "expann_append_device", "expann_reserve"):
        assert name in _lib.ABI_SYMBOLS
