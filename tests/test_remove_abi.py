"""The remove calls at the C ABI, as far as they go without a device: the symbols exist with their prototypes, a NULL
handle is EXPANN_ERR_INVALID_ARG before anything else is looked at, and every layer above offers the calls."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_a_null_handle_is_an_invalid_argument(lib):
    ids = (C.c_uint64 * 4)(0, 1, 2, 3)
    removed = C.c_size_t(77)
    assert lib.expann_remove(None, ids, 4, C.byref(removed)) == 1
    assert lib.expann_remove(None, None, 0, None) == 1
    assert lib.expann_remove_device(None, ids, 4, None, C.byref(removed)) == 1
    assert lib.expann_remove_device(None, None, 0, None, None) == 1
    assert lib.expann_compact_row_filter(None, C.byref(removed)) == 1
    assert lib.expann_compact_row_filter(None, None) == 1
    assert removed.value == 77   # (a refused call writes nothing)


def test_the_engines_offer_the_calls():
    from expann_amd import GpuBruteForceEngine, _lib
    for name in ("remove", "remove_device", "compact_row_filter"):
        assert callable(getattr(GpuBruteForceEngine, name))
    for name in ("expann_remove", "expann_remove_device", "expann_compact_row_filter"):
        assert name in _lib.ABI_SYMBOLS
    cpp = open(os.path.join(ROOT, "include", "expann", "gpu_brute_force_engine.h")).read()
    assert re.search(r"size_t\s+remove_rows\(const uint64_t\*\s*ids,\s*size_t\s+n\)", cpp)
    assert re.search(r"size_t\s+compact_row_filter\(\)", cpp)


def test_the_header_declares_them():
    text = open(os.path.join(ROOT, "include", "expann_hip.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert "int expann_remove(expann_index* h, const uint64_t* ids, size_t n_ids, size_t* n_removed);" in flat
    assert ("int expann_remove_device(expann_index* h, const uint64_t* d_ids, size_t n_ids, void* stream, "
            "size_t* n_removed);") in flat
    assert "int expann_compact_row_filter(expann_index* h, size_t* n_removed);" in flat
    assert "THE REMOVE RULE" in text
    assert re.search(r"#define\s+EXPANN_ABI_VERSION\s+2\b", text)
    for name in ("remove_calls", "remove_rows", "remove_compacts", "remove_rebuilds"):
        assert f'"{name}"' in text
