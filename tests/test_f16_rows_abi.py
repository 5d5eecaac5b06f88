"""CPU-side checks of EXPANN_DTYPE_F16: the header's constants, expann_create's argument checks (made before it looks
for a device, as for f32 rows) and the host rounding of include/expann/half.h against numpy's float32 -> float16."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16 = 4


@pytest.fixture(scope="module")
def lib():
    from expann_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_appends_the_dtype_and_keeps_the_abi_version():
    from expann_amd import _lib
    txt = open(os.path.join(ROOT, "include", "expann_hip.h")).read()
    assert re.search(r"\bEXPANN_DTYPE_F16\s*=\s*4\b", txt)
    assert re.search(r"^#define EXPANN_ABI_VERSION 2$", txt, re.M)
    assert _lib.DTYPE_F16 == F16


def test_create_checks_f16_arguments_before_any_device_check(lib):
    h = C.c_void_p()
    assert lib.expann_create(24, F16, 0, 0, C.byref(h)) == 1            # EXPANN_ERR_INVALID_ARG
    assert b"multiple of 16" in lib.expann_last_error(None)
    assert lib.expann_create(4112, F16, 0, 0, C.byref(h)) == 5          # EXPANN_ERR_UNSUPPORTED
    assert not h.value
    assert b"4096" in lib.expann_last_error(None)
    assert lib.expann_create(4112, F16, 1, 0, C.byref(h)) == 5
    assert lib.expann_create(128, F16, 2, 0, C.byref(h)) == 1           # (the int8 metric)
    assert b"metric" in lib.expann_last_error(None)
    assert not h.value


@pytest.fixture(scope="module")
def to_half(tmp_path_factory):
    so = tmp_path_factory.mktemp("native") / "half_hook.so"
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "half_hook.cpp"), "-o", str(so)])
    hook = C.CDLL(str(so))
    hook.f32_to_f16_bits.restype = None
    hook.f32_to_f16_bits.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]

    def f(x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty(x.size, np.uint16)
        hook.f32_to_f16_bits(x.ctypes.data, x.size, out.ctypes.data)
        return out
    return f


def _numpy_bits(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)


def _same_but_for_nan_payloads(got, x):
    want = _numpy_bits(x)
    nan = np.isnan(np.asarray(x, np.float32))
    assert np.array_equal(got[~nan], want[~nan])
    assert np.isnan(got[nan].view(np.float16)).all()
    assert np.array_equal(got[nan] >> 15, want[nan] >> 15)              # (the sign is kept)


def test_every_half_round_trips(to_half):
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    up = bits.view(np.float16).astype(np.float32)                       # exact
    got = to_half(up)
    nan = np.isnan(up)
    assert np.array_equal(got[~nan], bits[~nan])
    assert np.isnan(got[nan].view(np.float16)).all()


def test_midpoints_between_adjacent_halves_and_their_neighbours(to_half):
    """every tie, and the floats one ulp either side of it: nearest even, subnormal halves included"""
    pos = np.arange(0, 0x7C00, dtype=np.uint32).astype(np.uint16)       # finite non-negative halves below the largest
    lo = pos.view(np.float16).astype(np.float64)
    hi = (pos + np.uint16(1)).view(np.float16).astype(np.float64)
    hi[-1] = 65536.0                                                    # (above 65504: the tie that overflows, 65520)
    mid = ((lo + hi) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (lo + hi) / 2)        # the midpoints are fp32 values
    below = np.nextafter(mid, np.float32(-np.inf))
    above = np.nextafter(mid, np.float32(np.inf))
    for x in (mid, below, above, -mid, -below, -above):
        assert np.array_equal(to_half(x), _numpy_bits(x))
    assert mid[-1] == 65520.0 and to_half(mid[-1:])[0] == 0x7C00 and to_half(below[-1:])[0] == 0x7BFF


def test_special_values(to_half):
    x = np.array([65520.0, -65520.0, 65519.996, -65519.996, 0.0, -0.0, np.inf, -np.inf, 1e30, -1e30,
                  2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23), 2.0 ** -14, 2.0 ** -149, 1e-40], np.float32)
    assert np.array_equal(to_half(x), _numpy_bits(x))
    assert list(to_half(x)[:2]) == [0x7C00, 0xFC00]
    assert list(to_half(x)[4:8]) == [0x0000, 0x8000, 0x7C00, 0xFC00]
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF], np.uint32).view(np.float32)
    _same_but_for_nan_payloads(to_half(nans), nans)


def test_a_million_random_bit_patterns(to_half):
    x = np.random.default_rng(16).integers(0, 2 ** 32, 1_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    _same_but_for_nan_payloads(to_half(x), x)


def test_rows_f16_is_a_compile_time_error_for_other_row_types(tmp_path):
    """config::rows_f16 exists on gpu_brute_force_engine<float> only: naming it for another T does not compile"""
    src = ('#include "expann/gpu_brute_force_engine.h"\n'
           "void f() {{ gpu_brute_force_engine<{T}>::config c(0); c.rows_f16 = true; (void)c; }}\n")
    for T, ok in (("float", True), ("uint8_t", False), ("int8_t", False), ("int16_t", False)):
        cpp = tmp_path / f"rows_f16_{T}.cpp"
        cpp.write_text(src.format(T=T))
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(cpp)],
                           capture_output=True, text=True)
        assert (r.returncode == 0) == ok, (T, r.stderr[-500:])
        if not ok:
            assert "rows_f16" in r.stderr
