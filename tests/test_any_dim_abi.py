"""CPU-side checks of the f32 dim range (any multiple of 16 up to 4096): both limits are enforced
by expann_create before it looks for a device."""
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


def test_dim_over_4096_is_unsupported_before_any_device_check(lib):
    h = C.c_void_p()
    assert lib.expann_create(4112, 0, 0, 0, C.byref(h)) == 5          # EXPANN_ERR_UNSUPPORTED
    assert not h.value
    assert b"4096" in lib.expann_last_error(None)
    assert lib.expann_create(8192, 0, 1, 0, C.byref(h)) == 5
    assert b"4096" in lib.expann_last_error(None)


def test_dim_not_a_multiple_of_16_stays_invalid(lib):
    h = C.c_void_p()
    assert lib.expann_create(100, 0, 0, 0, C.byref(h)) == 1           # EXPANN_ERR_INVALID_ARG
    assert b"multiple of 16" in lib.expann_last_error(None)
    assert lib.expann_create(4100, 0, 0, 0, C.byref(h)) == 1
