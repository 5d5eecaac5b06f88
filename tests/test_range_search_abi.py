"""CPU-side checks of the range search's surface: the two entry points exist with the declared signatures, the
header declares them under ABI version 2, and they reject a NULL handle before they look for a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED, NOT_BUILT = 1, 5, 4  # EXPANN_ERR_INVALID_ARG, EXPANN_ERR_UNSUPPORTED, EXPANN_ERR_NOT_BUILT


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _header():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "expann_hip.h")).read(), flags=re.S)
    return " ".join(text.split())


def test_symbols_and_signatures(lib):
    from expann_amd import _lib
    vp, sz = C.c_void_p, C.c_size_t
    want = {"expann_range_search": [vp, vp, vp, sz, sz, vp, vp, vp],
            "expann_range_search_device": [vp, vp, vp, sz, sz, vp, vp, vp, vp]}
    for name, argtypes in want.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert list(fn.argtypes) == argtypes, name
        assert name in _lib.ABI_SYMBOLS, name


def test_header_declares_them_and_the_abi_version_stays():
    text = _header()
    assert ("int expann_range_search(expann_index* h, const void* queries, const float* radii, size_t m, "
            "size_t max_results, uint64_t* ids, float* dists, uint32_t* counts);") in text
    assert ("int expann_range_search_device(expann_index* h, const void* d_queries, const float* d_radii, size_t m, "
            "size_t max_results, uint64_t* d_ids, float* d_dists, uint32_t* d_counts, void* stream);") in text
    assert "#define EXPANN_ABI_VERSION 2" in text
    # the rule and what is not offered are stated in the header's comment
    raw = " ".join(open(os.path.join(ROOT, "include", "expann_hip.h")).read().replace(" * ", " ").split())
    for phrase in ("THE RANGE RULE", "score(q_i, b) <= radii[i]", "A NaN radius is in range of nothing",
                   "never an estimate, never saturated", "0 <= max_results <= 8192", "\"range_list_queries\"",
                   "\"range_topk_queries\"", "\"range_retries\"", "range search under a row filter or per row group",
                   "on the sharded handles", "more than 8192 rows per query"):
        assert phrase in raw, phrase


def test_null_handle_is_invalid_arg(lib):
    q = (C.c_float * 64)()
    r = (C.c_float * 4)()
    ids = (C.c_uint64 * 4)()
    d = (C.c_float * 4)()
    cnt = (C.c_uint32 * 4)()
    assert lib.expann_range_search(None, q, r, 4, 1, ids, d, cnt) == INVALID_ARG
    assert lib.expann_range_search_device(None, q, r, 4, 1, ids, d, cnt, None) == INVALID_ARG
    # (a NULL handle comes before every other check: also with a max_results beyond the bound)
    assert lib.expann_range_search(None, q, r, 4, 8193, ids, d, cnt) == INVALID_ARG


@pytest.mark.gpu
def test_checks_by_value_where_a_handle_can_be_made(lib):
    """a handle needs a device (its stream), hence the gpu mark; with one: 8-bit rows are UNSUPPORTED, NULL pointers
    come first, and max_results = 8193 is UNSUPPORTED before the missing rows are NOT_BUILT"""
    from expann_amd import _lib
    assert (_lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_NOT_BUILT) == (INVALID_ARG, UNSUPPORTED, NOT_BUILT)
    q = np.zeros((4, 64), np.float32)
    r = np.ones(4, np.float32)
    ids = np.zeros((4, 8193), np.uint64)
    cnt = np.zeros(4, np.uint32)
    args = (q.ctypes.data, r.ctypes.data, 4)
    h = C.c_void_p()
    assert lib.expann_create(64, _lib.DTYPE_U8, _lib.METRIC_L2, 0, C.byref(h)) == _lib.OK
    try:
        assert lib.expann_range_search(h, *args, 8, ids.ctypes.data, None, cnt.ctypes.data) == UNSUPPORTED
        assert lib.expann_range_search_device(h, *args, 8, ids.ctypes.data, None, cnt.ctypes.data, None) == UNSUPPORTED
        assert lib.expann_range_search(h, *args, 8, ids.ctypes.data, None, None) == INVALID_ARG
    finally:
        lib.expann_destroy(h)
    h = C.c_void_p()
    assert lib.expann_create(64, _lib.DTYPE_F32, _lib.METRIC_L2, 0, C.byref(h)) == _lib.OK
    try:
        assert lib.expann_range_search(h, None, r.ctypes.data, 4, 8, ids.ctypes.data, None, cnt.ctypes.data) == INVALID_ARG
        assert lib.expann_range_search(h, q.ctypes.data, None, 4, 8, ids.ctypes.data, None, cnt.ctypes.data) == INVALID_ARG
        assert lib.expann_range_search(h, *args, 8, None, None, cnt.ctypes.data) == INVALID_ARG
        assert lib.expann_range_search(h, *args, 8193, ids.ctypes.data, None, cnt.ctypes.data) == UNSUPPORTED
        assert lib.expann_range_search_device(h, *args, 8193, ids.ctypes.data, None, cnt.ctypes.data, None) == UNSUPPORTED
        assert lib.expann_range_search(h, *args, 8192, ids.ctypes.data, None, cnt.ctypes.data) == NOT_BUILT
        assert lib.expann_range_search(h, *args, 0, None, None, cnt.ctypes.data) == NOT_BUILT
    finally:
        lib.expann_destroy(h)
