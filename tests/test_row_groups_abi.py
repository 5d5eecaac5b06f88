"""CPU-side checks of the brute-force row groups' surface: the five entry points exist with the declared signatures,
the header declares them, and they reject a NULL handle before they look for a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = 1, 5  # EXPANN_ERR_INVALID_ARG, EXPANN_ERR_UNSUPPORTED


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
    vp, sz = C.c_void_p, C.c_size_t
    want = {"expann_set_row_groups": [vp, vp, sz],
            "expann_set_row_groups_device": [vp, vp, sz, vp],
            "expann_clear_row_groups": [vp],
            "expann_search_grouped": [vp, vp, vp, sz, sz, vp, vp],
            "expann_search_grouped_device": [vp, vp, vp, sz, sz, vp, vp, vp]}
    for name, argtypes in want.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert list(fn.argtypes) == argtypes, name


def test_header_declares_them_and_the_abi_version_stays():
    text = _header()
    assert "int expann_set_row_groups(expann_index* h, const uint32_t* groups, size_t n);" in text
    assert "int expann_set_row_groups_device(expann_index* h, const uint32_t* d_groups, size_t n, void* stream);" in text
    assert "int expann_clear_row_groups(expann_index* h);" in text
    assert ("int expann_search_grouped(expann_index* h, const void* queries, const uint32_t* query_groups, size_t m, "
            "size_t k, uint64_t* ids, float* dists);") in text
    assert ("int expann_search_grouped_device(expann_index* h, const void* d_queries, const uint32_t* query_groups , "
            "size_t m, size_t k, uint64_t* d_ids, float* d_dists, void* stream);") in text
    assert "#define EXPANN_ABI_VERSION 2" in text
    assert "#define EXPANN_GROUP_ANY 0xFFFFFFFFu" in text
    # the rule and what is not offered are stated in the header's comment
    raw = " ".join(open(os.path.join(ROOT, "include", "expann_hip.h")).read().replace(" * ", " ").split())
    for phrase in ("query_groups IS HOST MEMORY", "\"group_list_rows\"", "ONE HOST WAIT PER DISTINCT SUCH GROUP",
                   "deferred grouped searches", "groups on the sharded handles"):
        assert phrase in raw, phrase
    assert "groups on the brute-force" not in raw


def test_null_handle_is_invalid_arg(lib):
    lab = (C.c_uint32 * 4)(1, 2, 3, 4)
    q = (C.c_float * 64)()
    ids = (C.c_uint64 * 4)()
    d = (C.c_float * 4)()
    assert lib.expann_set_row_groups(None, lab, 4) == INVALID_ARG
    assert lib.expann_set_row_groups_device(None, lab, 4, None) == INVALID_ARG
    assert lib.expann_clear_row_groups(None) == INVALID_ARG
    assert lib.expann_search_grouped(None, q, lab, 4, 1, ids, d) == INVALID_ARG
    assert lib.expann_search_grouped_device(None, q, lab, 4, 1, ids, d, None) == INVALID_ARG


def test_u8_handle_is_unsupported_where_a_handle_can_be_made(lib):
    """a handle needs a device (its stream); where one can be made, 8-bit rows refuse the set call before the
    device is touched again -- and a NULL array comes first"""
    from expann_amd import _lib
    h = C.c_void_p()
    if lib.expann_create(64, _lib.DTYPE_U8, _lib.METRIC_L2, 0, C.byref(h)) != _lib.OK:
        return  # (no device here: no handle of any dtype can be made)
    try:
        lab = np.zeros(8, np.uint32)
        assert lib.expann_set_row_groups(h, None, 8) == INVALID_ARG
        assert lib.expann_set_row_groups(h, lab.ctypes.data, 8) == UNSUPPORTED
        assert lib.expann_set_row_groups_device(h, lab.ctypes.data, 8, None) == UNSUPPORTED
    finally:
        lib.expann_destroy(h)
