"""EXPANN_DTYPE_I4 at the ABI and in the planner, without a device: pack_i4 / unpack_i4 against a three-line NumPy
statement of the nibble order, expann_create's checks that come before the device lookup, and plan_i4 as plan_scan
reaches it through tests/native/bf_plan_hook.cpp (the family shares the value the hook prints as "gemm_i8")."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = 1, 5
I4 = 6
L2, IP, L2_REFCOMPAT, HAMMING = 0, 1, 2, 3


def test_pack_round_trip_and_nibble_order():
    from expann_amd import pack_i4, unpack_i4
    values = np.random.default_rng(1).integers(-8, 8, (7, 128), dtype=np.int8)
    values[0, :16] = np.arange(-8, 8)
    rows = pack_i4(values)
    low = (rows & 15).astype(np.int16)
    high = (rows >> 4).astype(np.int16)
    assert np.array_equal(np.where(low > 7, low - 16, low), values[:, 0::2])
    assert np.array_equal(np.where(high > 7, high - 16, high), values[:, 1::2])
    assert rows.dtype == np.uint8 and rows.shape == (7, 64) and np.array_equal(unpack_i4(rows), values)
    for bad in (np.full((1, 64), 8, np.int8), np.zeros((1, 64), np.int16), np.zeros((1, 63), np.int8)):
        with pytest.raises(ValueError):
            pack_i4(bad)


@pytest.mark.parametrize("dim,metric,code", [(100, IP, INVALID_ARG), (96, L2, INVALID_ARG), (4160, IP, UNSUPPORTED),
                                             (8192, L2, UNSUPPORTED), (256, HAMMING, INVALID_ARG),
                                             (256, L2_REFCOMPAT, INVALID_ARG)])
def test_create_refuses_before_the_device(dim, metric, code):
    from expann_amd import _lib
    h = C.c_void_p()
    assert _lib.load().expann_create(dim, I4, metric, 0, C.byref(h)) == code
    assert not h.value


# (inputs of the hook beyond dtype = int_mode = 6, n = 1 M rows, m = 1000, k = 10, cap = 2048) -> status, family
PLANS = [("metric=1 dim=64 m=1", 0, "gemm_i8"),
         ("metric=0 dim=4096 m=100000", 0, "gemm_i8"),
         ("metric=1 dim=768 scan_kernel=1", 0, "gemm_i8"),       # "scan_kernel" is not read
         ("metric=1 dim=768 force_direct=1", 0, "gemm_i8"),      # there is no direct scan to fall back to
         ("metric=0 dim=768 k=8192 cap=16384", 0, "gemm_i8"),
         ("metric=0 dim=768 k=8193 cap=16384", UNSUPPORTED, "direct"),
         ("metric=0 dim=768 k=2000 cap=2048", UNSUPPORTED, "direct"),
         ("metric=3 dim=768", UNSUPPORTED, "direct")]


def test_the_plan_of_4_bit_rows(tmp_path):
    exe = tmp_path / "bf_plan_hook"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "expann_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "bf_plan_hook.cpp"), "-o", str(exe)])
    text = "".join(f"dtype=6 int_mode=6 n=1000000 {case[0]}\n" for case in PLANS)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(PLANS)
    for case, line in zip(PLANS, out):
        f = line.split("\t")
        assert (int(f[0]), f[1], int(f[4])) == (case[1], case[2], 64), (case, line)
        assert f[2] == "-" and f[3] == "0" and f[8] == "0" and f[9] == "0" and f[10] == "0"  # no q-form, shadow, speculation, sample, restart
