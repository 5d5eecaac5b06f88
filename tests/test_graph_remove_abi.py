"""CPU-side checks of the graph engine's remove (THE GRAPH REMOVE RULE, include/expann_hip.h): the host statement
of the rule, antitopo_index::remove_rows, against the NumPy restatement of tests/graph_remove_helpers.py, edge for
edge and length bits for length bits; the new symbols, their argtypes and the header text; the stat names; the
refusals that come before any device is looked for.  What needs a device is in tests/test_gpu_graph_remove.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import graph_remove_helpers as grh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ["remove_calls", "remove_rows", "remove_touched_rows", "remove_truncated_rows", "remove_device", "remove_host",
         "remove_repair_ns"]


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def hook_dir(tmp_path_factory):
    """tests/native/graph_remove_hook.cpp built -- under the address and undefined-behaviour sanitizers where g++ has
    their static runtimes -- and run once"""
    d = tmp_path_factory.mktemp("graph_remove_hook")
    exe = d / "graph_remove_hook"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "graph_remove_hook.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:  # (no static sanitizer runtimes here)
        subprocess.check_call(cmd)
    out = subprocess.run([str(exe), str(d)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
    return d


@pytest.fixture(scope="module")
def restated(hook_dir):
    """the NumPy restatement of every case, computed once"""
    before = str(hook_dir / "before.index")
    return {c: grh.apply_remove(before, np.fromfile(str(hook_dir / f"case_{c}.ids"), np.uint64)) for c in "abcde"}


@pytest.mark.parametrize("case", list("abcde"))
def test_the_host_rule_is_the_numpy_restatement(hook_dir, restated, case):
    grh.assert_file_is(str(hook_dir / f"case_{case}.index"), restated[case])


def test_the_cases_show_what_they_are_for(hook_dir, restated):
    hdr, _ = grh.read_index_edges(str(hook_dir / "before.index"))
    assert hdr["max_layer"] >= 3 and hdr["n"] == 700
    ids_a = np.fromfile(str(hook_dir / "case_a.ids"), np.uint64)
    assert len(ids_a) == 80 and len(np.unique(ids_a)) < len(ids_a) and (np.diff(ids_a.astype(np.int64)) < 0).any()
    assert restated["a"]["touched"] > 0
    assert restated["b"]["max_layer"] < hdr["max_layer"]
    assert restated["c"]["truncated"] > 0
    assert restated["d"]["empty_rows"] > 0
    assert restated["e"]["n"] == 1 and restated["e"]["starting_vertex"] == 0


def test_new_symbols_and_signatures(lib):
    from expann_amd import _lib
    vp, sz, szp = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    want = {"expann_antitopo_remove": [vp, vp, sz, szp],
            "expann_antitopo_compact_row_filter": [vp, szp],
            "expann_graph_remove": [vp, vp, sz, u32p, u32p, szp],
            "expann_graph_note_host_remove": [vp, u64p, sz]}
    for name, argtypes in want.items():
        assert name in _lib.ABI_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
    raw = open(os.path.join(ROOT, "include", "expann_hip.h")).read()
    text = " ".join(re.sub(r"/\*.*?\*/", " ", raw, flags=re.S).split())
    for decl in ("int expann_antitopo_remove(expann_antitopo* e, const uint64_t* ids, size_t n_ids, size_t* n_removed);",
                 "int expann_antitopo_compact_row_filter(expann_antitopo* e, size_t* n_removed);",
                 "int expann_graph_remove(expann_graph* g, const uint64_t* ids, size_t n_ids, uint32_t* max_layer_out, "
                 "uint32_t* starting_vertex_out, size_t* n_removed);",
                 "#define EXPANN_ABI_VERSION 2"):
        assert decl in text, decl
    assert lib.expann_abi_version() == 2
    # the declarations come last: nothing that existed moved
    assert text.index("int expann_antitopo_remove(") > text.index("int expann_graph_note_host_append(")
    rule = raw[raw.index("THE GRAPH REMOVE RULE"):]
    for phrase in ["THE DEVICE ROUTE", "THE HOST ROUTE", "Not offered", "One hop", "prune_edges"] + \
            ['"%s"' % s for s in STATS]:
        assert phrase in rule, phrase


def test_the_stat_names_are_rows_of_the_table():
    src = open(os.path.join(ROOT, "expann_amd", "csrc", "expann_graph.hip")).read()
    table = src[src.index("kGraphRemoveStatTable[] = {"):]
    table = table[:table.index("};")]
    assert sorted(re.findall(r'\{"(\w+)",', table)) == sorted(STATS)


def test_null_arguments_are_refused_before_the_device(lib):
    from expann_amd import _lib
    INV = _lib.ERR_INVALID_ARG
    ids = (C.c_uint64 * 2)(1, 2)
    done = C.c_size_t(7)
    assert lib.expann_antitopo_remove(None, ids, 2, C.byref(done)) == INV and done.value == 0
    assert lib.expann_antitopo_remove(None, None, 0, None) == INV  # (a NULL engine before n_ids == 0)
    done = C.c_size_t(7)
    assert lib.expann_antitopo_compact_row_filter(None, C.byref(done)) == INV and done.value == 0
    done = C.c_size_t(7)
    assert lib.expann_graph_remove(None, ids, 2, None, None, C.byref(done)) == INV and done.value == 0
    assert lib.expann_graph_note_host_remove(None, None, 1) == INV
    out = C.c_uint64(7)
    for name in STATS:
        assert lib.expann_graph_get_stat(None, name.encode(), C.byref(out)) == INV
    assert out.value == 7


def test_python_surface():
    from expann_amd import AntitopoEngine, _lib
    for name in ("remove", "compact_row_filter"):
        assert callable(getattr(AntitopoEngine, name))
    eng = AntitopoEngine(16, 80, 1, 0, False)  # (no dim yet: nothing is opened, no device is asked for)
    for call in (lambda: eng.remove(np.array([1], np.uint64)), lambda: eng.compact_row_filter()):
        with pytest.raises(_lib.ExpannError) as ei:
            call()
        assert ei.value.code == _lib.ERR_NOT_BUILT


def test_the_engine_header_offers_remove_rows_and_compact_row_filter():
    text = open(os.path.join(ROOT, "include", "expann", "gpu_antitopo_engine.h")).read()
    assert "int remove_rows(const uint64_t* ids, size_t n, size_t* n_removed = nullptr)" in text
    assert "int compact_row_filter(size_t* n_removed = nullptr)" in text
