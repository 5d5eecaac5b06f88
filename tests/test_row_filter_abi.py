"""CPU-side checks of the row filter's surface: the three entry points exist with the declared signatures and
reject a NULL handle before they look for a device; pack_row_filter is the bit layout the header describes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_symbols_and_signatures(lib):
    vp, sz = C.c_void_p, C.c_size_t
    want = {"expann_set_row_filter": [vp, vp, sz],
            "expann_set_row_filter_device": [vp, vp, sz, vp],
            "expann_clear_row_filter": [vp]}
    for name, argtypes in want.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert list(fn.argtypes) == argtypes, name
    # ... and the header declares them with these parameters
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "expann_hip.h")).read(), flags=re.S)
    text = " ".join(text.split())
    assert "int expann_set_row_filter(expann_index* h, const uint32_t* allow_bits, size_t n_words);" in text
    assert ("int expann_set_row_filter_device(expann_index* h, const uint32_t* d_allow_bits, size_t n_words, "
            "void* stream);") in text
    assert "int expann_clear_row_filter(expann_index* h);" in text
    assert "#define EXPANN_ABI_VERSION 2" in text


def test_null_handle_is_invalid_arg(lib):
    words = (C.c_uint32 * 4)(1, 2, 3, 4)
    assert lib.expann_set_row_filter(None, words, 4) == 1            # EXPANN_ERR_INVALID_ARG
    assert lib.expann_set_row_filter_device(None, words, 4, None) == 1
    assert lib.expann_clear_row_filter(None) == 1


@pytest.mark.parametrize("n", [1, 31, 32, 33, 4099])
def test_pack_row_filter_is_little_endian_words(n):
    from expann_amd import pack_row_filter
    rng = np.random.RandomState(n)
    for allow in (rng.rand(n) < 0.5, np.ones(n, bool), np.zeros(n, bool)):
        words = pack_row_filter(allow)
        assert words.dtype == np.uint32 and words.shape == ((n + 31) // 32,)
        by = np.packbits(allow, bitorder="little")
        got = words.astype("<u4").view(np.uint8)
        assert np.array_equal(got[:by.size], by)
        assert not got[by.size:].any()
        # bit r & 31 of word r >> 5, and nothing past n
        r = np.arange(words.size * 32)
        bits = (words[r >> 5] >> (r & 31).astype(np.uint32)) & 1
        assert np.array_equal(bits[:n].astype(bool), allow)
        assert not bits[n:].any()
    # a pure function: the argument is left alone, lists and 0 / 1 integers are taken too
    a = [1, 0, 1]
    assert pack_row_filter(a).tolist() == [5] and a == [1, 0, 1]
