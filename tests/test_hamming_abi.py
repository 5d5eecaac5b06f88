"""EXPANN_DTYPE_B1 / EXPANN_METRIC_HAMMING at the ABI and in the planner, without a device: expann_create's checks
come before the device lookup, and the plan is read through tests/native/bf_plan_hook.cpp (which names the matrix-core
Hamming family by the value it shares, "gemm_i8")."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = 1, 5
F32, B1 = 0, 5
L2, IP, HAMMING = 0, 1, 3


@pytest.mark.parametrize("dim,dtype,metric,code", [(256, B1, L2, INVALID_ARG), (256, B1, IP, INVALID_ARG),
                                                   (256, F32, HAMMING, INVALID_ARG), (100, B1, HAMMING, INVALID_ARG),
                                                   (8192, B1, HAMMING, UNSUPPORTED)])
def test_create_refuses_before_the_device(dim, dtype, metric, code):
    from expann_amd import _lib
    h = C.c_void_p()
    assert _lib.load().expann_create(dim, dtype, metric, 0, C.byref(h)) == code
    assert not h.value


# (inputs of the hook beyond int_mode=5, n = 1 M rows, m = 1000, k = 10) -> status, family, direct_tq, tie_fallback, sampled
PLANS = [("dim=256", 0, "gemm_i8", 8, 1, 0),
         ("dim=256 m=511", 0, "direct", 8, 0, 1),
         ("dim=256 m=512", 0, "gemm_i8", 8, 1, 0),
         ("dim=256 m=4096 n=999999", 0, "gemm_i8", 8, 1, 0),
         ("dim=256 m=4095 n=999999", 0, "direct", 8, 0, 1),
         ("dim=256 m=4096 n=65535", 0, "direct", 8, 0, 1),
         ("dim=256 m=4096 n=65536", 0, "gemm_i8", 8, 1, 0),
         ("dim=256 m=3 scan_kernel=2", 0, "gemm_i8", 4, 0, 0),
         ("dim=256 scan_kernel=1", 0, "direct", 8, 0, 1),
         ("dim=256 force_direct=1", 0, "direct", 8, 0, 1),
         ("dim=1024", 0, "gemm_i8", 8, 1, 0),
         ("dim=1088", 0, "direct", 8, 0, 1),
         ("dim=1088 scan_kernel=2", UNSUPPORTED, "direct", 8, 0, 0),
         ("dim=256 scan_kernel=3", INVALID_ARG, "direct", 8, 0, 0),
         ("dim=4096 m=1", 0, "direct", 1, 0, 1)]


def test_the_plan_of_packed_bit_rows(tmp_path):
    exe = tmp_path / "bf_plan_hook"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "expann_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "bf_plan_hook.cpp"), "-o", str(exe)])
    text = "".join(f"dtype=5 int_mode=5 metric=3 n=1000000 {case[0]}\n" for case in PLANS)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(PLANS)
    for case, line in zip(PLANS, out):
        f = line.split("\t")
        got = (int(f[0]), f[1], int(f[4]), int(f[10]), int(f[9]))
        assert got == case[1:], (case, line)
        assert f[2] == "-" and f[3] == "0" and f[8] == "0"  # no q-form, no shadow, no speculation
