"""CPU-side checks of the 8-bit dim range (any multiple of 64 up to 4096): both limits are enforced by
expann_create before it looks for a device; int16 rows keep their compiled dims."""
import ctypes as C
import os

import pytest

UNSUPPORTED, INVALID_ARG, NO_DEVICE = 5, 1, 2
U8, I8, I16 = 1, 2, 3
L2, IP = 0, 1


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.mark.parametrize("dim,dtype,metric", [(8192, U8, L2), (4160, I8, IP)])
def test_8bit_dim_over_4096_is_unsupported_before_any_device_check(lib, dim, dtype, metric):
    h = C.c_void_p()
    assert lib.expann_create(dim, dtype, metric, 0, C.byref(h)) == UNSUPPORTED
    assert not h.value
    assert b"4096" in lib.expann_last_error(None)


@pytest.mark.parametrize("dim,dtype,metric", [(528, U8, L2), (4080, I8, L2)])
def test_8bit_dim_not_a_multiple_of_64_stays_invalid(lib, dim, dtype, metric):
    h = C.c_void_p()
    assert lib.expann_create(dim, dtype, metric, 0, C.byref(h)) == INVALID_ARG
    assert not h.value
    assert b"64" in lib.expann_last_error(None)


def test_int16_rows_at_512_are_still_refused(lib):
    h = C.c_void_p()
    rc = lib.expann_create(512, I16, L2, 0, C.byref(h))
    assert not h.value
    if lib.expann_device_count() < 1:
        assert rc == NO_DEVICE            # (the compiled-dim lookup comes after the device check)
    else:
        assert rc == UNSUPPORTED
        assert b"int16 64,128" in lib.expann_last_error(None)
