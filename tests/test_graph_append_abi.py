"""CPU-side checks of the graph engine's append (THE GRAPH APPEND RULE, include/expann_hip.h): the new symbols, their
argtypes and the header text, the refusals that come before any device is looked for, the Python surface, and the
stat names in the table behind expann_graph_get_stat.  What needs a handle -- expann_antitopo_create asks for a
device -- is in tests/test_gpu_graph_append.py: EXPANN_ERR_NOT_BUILT from the C calls, n == 0, the stats' values."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ["append_calls", "append_rows", "append_batches", "append_device", "append_host", "graph_reallocs",
         "capacity_rows", "append_tables_ns", "append_edges"]


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_new_symbols_and_signatures(lib):
    from expann_amd import _lib
    vp, sz, szp = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    want = {"expann_antitopo_append": [vp, vp, sz, szp],
            "expann_antitopo_reserve": [vp, sz],
            "expann_antitopo_get_stat": [vp, C.c_char_p, u64p],
            "expann_graph_reserve": [vp, sz],
            "expann_graph_adopt_build_state": [vp, sz, sz, sz, sz, C.c_float, C.c_float, vp, vp, vp, vp, vp, sz, sz, sz,
                                               vp, vp, vp, sz],
            "expann_graph_append": [vp, vp, sz, vp, u32p, u32p, szp],
            "expann_graph_build_state_shape": [vp, szp],
            "expann_graph_read_build_state": [vp] * 9,
            "expann_graph_note_host_append": [vp, u64p, sz]}
    for name, argtypes in want.items():
        assert name in _lib.ABI_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
    raw = open(os.path.join(ROOT, "include", "expann_hip.h")).read()
    text = " ".join(re.sub(r"/\*.*?\*/", " ", raw, flags=re.S).split())
    for decl in ("int expann_antitopo_append(expann_antitopo* e, const float* rows, size_t n, size_t* n_appended);",
                 "int expann_antitopo_reserve(expann_antitopo* e, size_t n_rows);",
                 "int expann_antitopo_get_stat(expann_antitopo* e, const char* name, uint64_t* out);",
                 "int expann_graph_reserve(expann_graph* g, size_t n_rows);",
                 "int expann_graph_append(expann_graph* g, const float* rows, size_t n, const uint8_t* levels, "
                 "uint32_t* max_layer_out, uint32_t* starting_vertex_out, size_t* n_appended);",
                 "#define EXPANN_ABI_VERSION 2"):
        assert decl in text, decl
    assert lib.expann_abi_version() == 2
    # the declarations come last: nothing that existed moved
    assert text.index("int expann_antitopo_append(") > text.index("int expann_compact_row_filter(")
    rule = raw[raw.index("THE GRAPH APPEND RULE"):]
    for phrase in ["THE DEVICE ROUTE", "THE HOST ROUTE", "Not offered", "EXPANN_ERR_OVERFLOW", "1.47 GB"] + \
            ['"%s"' % s for s in STATS]:
        assert phrase in rule, phrase


def test_the_stat_names_are_rows_of_the_table():
    src = open(os.path.join(ROOT, "expann_amd", "csrc", "expann_graph.hip")).read()
    table = src[src.index("kGraphAppendStatTable[] = {"):]
    table = table[:table.index("};")]
    assert sorted(re.findall(r'\{"(\w+)",', table)) == sorted(STATS)


def test_null_arguments_are_refused_before_the_device(lib):
    from expann_amd import _lib
    INV = _lib.ERR_INVALID_ARG
    f = (C.c_float * 16)()
    lv = (C.c_uint8 * 1)()
    done = C.c_size_t(7)
    assert lib.expann_antitopo_append(None, f, 1, C.byref(done)) == INV and done.value == 0
    assert lib.expann_antitopo_append(None, f, 1, None) == INV
    assert lib.expann_antitopo_append(None, None, 0, None) == INV  # (a NULL engine before n == 0)
    assert lib.expann_antitopo_reserve(None, 10) == INV
    out = C.c_uint64(7)
    assert lib.expann_antitopo_get_stat(None, b"append_calls", C.byref(out)) == INV
    for name in STATS:
        assert lib.expann_graph_get_stat(None, name.encode(), C.byref(out)) == INV
    assert out.value == 7
    assert lib.expann_graph_reserve(None, 10) == INV
    assert lib.expann_graph_append(None, f, 1, lv, None, None, C.byref(done)) == INV and done.value == 0
    shape = (C.c_size_t * 6)()
    assert lib.expann_graph_build_state_shape(None, shape) == INV
    assert lib.expann_graph_read_build_state(None, *([None] * 8)) == INV
    assert lib.expann_graph_note_host_append(None, None, 1) == INV
    assert lib.expann_graph_adopt_build_state(None, 8, 16, 40, 0, 0.5, 0.0, None, None, None, None, None, 80, 0, 0, None,
                                              None, None, 72) == INV


def test_python_surface():
    from expann_amd import AntitopoEngine, _lib
    for name in ("append", "reserve", "stat"):
        assert callable(getattr(AntitopoEngine, name))
    eng = AntitopoEngine(16, 80, 1, 0, False)  # (no dim yet: nothing is opened, no device is asked for)
    for call in (lambda: eng.append(np.zeros((1, 16), np.float32)), lambda: eng.reserve(10),
                 lambda: eng.stat("append_calls")):
        with pytest.raises(_lib.ExpannError) as ei:
            call()
        assert ei.value.code == _lib.ERR_NOT_BUILT
    assert eng.size() == 0


def test_the_engine_header_offers_append_rows_and_reserve():
    text = open(os.path.join(ROOT, "include", "expann", "gpu_antitopo_engine.h")).read()
    assert "int append_rows(const float* rows, size_t n, size_t* n_appended = nullptr)" in text
    assert "int reserve(size_t n_rows)" in text


def test_the_host_refresh_round_trips_at_a_wider_upper_stride(tmp_path):
    """tests/native/graph_append_hook.cpp: to_strided, the upper arrays at a capacity's stride, from_strided as
    refresh_host calls it -- under the address and undefined-behaviour sanitizers where g++ has their static runtimes"""
    import subprocess
    exe = tmp_path / "graph_append_hook"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "graph_append_hook.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:  # (no static sanitizer runtimes here)
        subprocess.check_call(cmd)
    out = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
