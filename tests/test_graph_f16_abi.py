"""CPU-side checks of the graph engine over binary16 rows (THE F16 ROW RULE, include/expann_hip.h): what is
defined before the device is touched.

  * expann_graph_create_f16 makes expann_graph_create's argument checks, in the same order;
  * expann_antitopo_set_rows_f16 on a NULL handle;
  * the host side of an engine with rows_f16 -- rounding on insert, the refusal of a NaN and of 70000.0, the index
    file, the pack to halves, the refusal to load rows that are not binary16 values -- through
    tests/native/f16_graph_engine_hook.cpp, a stand-alone program over gpu_antitopo_engine<float> with the C ABI
    stubbed.  expann_antitopo_create asks for a device before it returns a handle, so the same cases through the C
    ABI and through AntitopoEngine(rows="f16") live in tests/test_gpu_graph_f16.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import graph_filter_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 5


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _create(fn, dim, rows=True, n=2, sv=0, out=True, off0=0):
    """a two-vertex, one-layer graph at `dim` with one argument made wrong; (rc, message)"""
    elem = np.float16 if fn.__name__.endswith("_f16") else np.float32
    vec = np.zeros((2, max(dim, 16)), elem)
    off = np.array([off0, 1, 2], np.uint64)
    nb = np.array([1, 0], np.uint32)
    h = C.c_void_p()
    rc = fn(dim, 0, vec.ctypes.data if rows else None, n, 1, sv, off.ctypes.data, nb.ctypes.data,
            C.byref(h) if out else None)
    assert rc != OK or h.value
    return rc, h


# (what is wrong, the status both calls must give): every case fails before the device is looked for
_BAD = [("out == NULL", dict(out=False), INVALID_ARG),
        ("dim 24", dict(dim=24), INVALID_ARG),
        ("dim 4112", dict(dim=4112), UNSUPPORTED),
        ("NULL rows", dict(rows=False), INVALID_ARG),
        ("starting_vertex >= n", dict(sv=2), INVALID_ARG),
        ("layer_offsets[0] != 0", dict(off0=1), INVALID_ARG)]


@pytest.mark.parametrize("what,kw,status", _BAD, ids=[b[0] for b in _BAD])
def test_create_f16_makes_the_checks_of_create(lib, what, kw, status):
    kw = dict(dict(dim=64), **kw)
    rc32, _ = _create(lib.expann_graph_create, **kw)
    msg32 = lib.expann_graph_last_error(None).decode()
    rc16, _ = _create(lib.expann_graph_create_f16, **kw)
    msg16 = lib.expann_graph_last_error(None).decode()
    assert rc32 == status and rc16 == status, what
    assert msg16 == msg32.replace("expann_graph_create", "expann_graph_create_f16"), what


def test_create_f16_checks_arrive_in_the_order_of_create(lib):
    """two things wrong at once: the earlier check answers, for both calls"""
    pairs = [(dict(out=False, dim=4112), INVALID_ARG),    # out before dim
             (dict(dim=4112, rows=False), UNSUPPORTED),   # dim before the pointers
             (dict(dim=24, sv=2), INVALID_ARG),
             (dict(rows=False, off0=1), INVALID_ARG)]
    for kw, status in pairs:
        kw = dict(dict(dim=64), **kw)
        msgs = []
        for fn in (lib.expann_graph_create, lib.expann_graph_create_f16):
            rc, _ = _create(fn, **kw)
            assert rc == status, (kw, fn.__name__)
            msgs.append(lib.expann_graph_last_error(None).decode().replace("_f16", ""))
        assert msgs[0] == msgs[1], kw
    # valid arguments get as far as the device in both: none here, one on a GPU machine
    for fn in (lib.expann_graph_create, lib.expann_graph_create_f16):
        rc, h = _create(fn, 64)
        assert rc in (OK, NO_DEVICE)
        if h.value:
            lib.expann_graph_destroy(h)


def test_new_symbols_and_signatures(lib):
    from expann_amd import _lib
    vp, sz = C.c_void_p, C.c_size_t
    assert "expann_graph_create_f16" in _lib.ABI_SYMBOLS and "expann_antitopo_set_rows_f16" in _lib.ABI_SYMBOLS
    assert list(lib.expann_graph_create_f16.argtypes) == [C.c_int, C.c_int, vp, sz, C.c_uint32, C.c_uint32, vp, vp,
                                                          C.POINTER(vp)]
    assert list(lib.expann_antitopo_set_rows_f16.argtypes) == [vp, C.c_int]
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "expann_hip.h")).read(), flags=re.S)
    text = " ".join(text.split())
    assert ("int expann_graph_create_f16(int dim, int device, const void* rows_f16, size_t n, uint32_t n_layers, "
            "uint32_t starting_vertex, const uint64_t* layer_offsets, const uint32_t* neighbours, "
            "expann_graph** out);") in text
    assert "int expann_antitopo_set_rows_f16(expann_antitopo* e, int on);" in text
    assert "#define EXPANN_ABI_VERSION 2" in text and lib.expann_abi_version() == 2
    raw = open(os.path.join(ROOT, "include", "expann_hip.h")).read()
    assert "THE F16 ROW RULE" in raw and "vector_bytes" in raw


def test_null_handles_are_refused(lib):
    assert lib.expann_antitopo_set_rows_f16(None, 1) == INVALID_ARG
    assert lib.expann_antitopo_set_rows_f16(None, 0) == INVALID_ARG
    out = C.c_uint64(7)
    assert lib.expann_graph_get_stat(None, b"vector_bytes", C.byref(out)) == INVALID_ARG and out.value == 7


def test_python_surface():
    from expann_amd import AntitopoEngine
    eng = AntitopoEngine(16, 80, 1, 0, False, rows="f16")  # (no dim yet: nothing is opened, no device is asked for)
    assert eng.param_list()["rows"] == "f16"
    assert "rows" not in AntitopoEngine(16, 80, 1, 0, False).param_list()
    with pytest.raises(ValueError, match="rows"):
        AntitopoEngine(16, 80, 1, 0, False, rows="bf16")


def test_half_to_float_is_exact_for_every_half(tmp_path):
    """expann::f16_bits_to_f32 over all 65536 patterns against numpy, and f32_to_f16_bits back"""
    src = tmp_path / "h2f.cpp"
    src.write_text('#include "expann/half.h"\n'
                   'extern "C" void h2f(float* out) { for (unsigned h = 0; h < 65536; ++h) out[h] = '
                   "expann::f16_bits_to_f32((uint16_t)h); }\n"
                   'extern "C" void f2h(const float* in, uint16_t* out) { for (unsigned h = 0; h < 65536; ++h) out[h] = '
                   "expann::f32_to_f16_bits(in[h]); }\n")
    so = tmp_path / "h2f.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(so)])
    L = C.CDLL(str(so))
    got = np.zeros(65536, np.float32)
    L.h2f(C.c_void_p(got.ctypes.data))
    halves = np.arange(65536, dtype=np.uint16)
    want = halves.view(np.float16).astype(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert np.isnan(got[nan]).all()
    back = np.zeros(65536, np.uint16)
    L.f2h(C.c_void_p(got.ctypes.data), C.c_void_p(back.ctypes.data))
    assert np.array_equal(back[~nan], halves[~nan])


def test_rows_f16_engine_rounds_on_insert_and_saves_what_the_device_holds(tmp_path, oracle):
    """Gaussian fp32 rows (n = 500, d = 64, serial build) through the stand-alone hook: the file's vectors equal
    base.astype(float16).astype(float32) bit for bit, the halves handed to expann_graph_create_f16 are numpy's,
    oracle.Graph opens the file, and a file of non-representable rows is refused before any upload (the hook's
    exit status names the check that failed)."""
    from graph_helpers import read_index_edges
    n, d, M, efc = 500, 64, 16, 80
    rng = np.random.RandomState(16)
    base = rng.standard_normal((n, d)).astype(np.float32)
    base[0, :4] = [6.0e-8, -3.1e-5, 65504.0, 0.0]  # a subnormal, another, the largest half, a zero
    rounded = base.astype(np.float16).astype(np.float32)
    assert not np.array_equal(rounded, base)
    bad_idx = H.build_index_cpu(tmp_path, base[:64], M, efc, name="not_halves")  # fp32 rows as they are
    exe = tmp_path / "f16_graph_engine_hook"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "f16_graph_engine_hook.cpp"), "-o", str(exe)])
    rows_path, idx, halves_path = tmp_path / "rows.f32", tmp_path / "f16.index", tmp_path / "rows.f16"
    base.tofile(rows_path)
    rc = subprocess.run([str(exe), str(rows_path), str(n), str(d), str(M), str(efc), str(idx), str(halves_path),
                         bad_idx]).returncode
    assert rc == 0, f"f16_graph_engine_hook: check {rc} failed"
    og = oracle.Graph(str(idx))
    assert (og.n, og.dim) == (n, d)
    assert np.array_equal(og.vectors().view(np.uint32), rounded.view(np.uint32))
    halves = np.fromfile(halves_path, np.uint16).reshape(n, d)
    assert np.array_equal(halves, base.astype(np.float16).view(np.uint16))
    # the builder saw the rounded rows: the file is the one the serial builder writes from them
    ref_idx = H.build_index_cpu(tmp_path, rounded, M, efc, name="rounded")
    assert open(ref_idx, "rb").read() == open(idx, "rb").read()
    hdr, _ = read_index_edges(str(idx))
    assert hdr["n"] == n
