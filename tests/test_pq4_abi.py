"""EXPANN_DTYPE_PQ4 without a device: expann_create's early checks, pack_pq4 / unpack_pq4, plan_pq4 through
tests/native/pq4_plan_hook.cpp, and THE PQ4 RULE on a four-row example worked by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = 1, 5
PQ4 = 8
L2, IP, L2_REFCOMPAT, HAMMING = 0, 1, 2, 3
GEMM_I8 = 7  # ScanFamily::kHamming = kGemmI8: the threshold ladder on the int8 matrix cores, plan_i4's family


@pytest.mark.parametrize("dim,metric,code", [(128, HAMMING, INVALID_ARG), (128, L2_REFCOMPAT, INVALID_ARG), (0, L2, INVALID_ARG),
                                             (15, IP, INVALID_ARG), (4097, L2, UNSUPPORTED)])
def test_create_refuses_before_the_device(dim, metric, code):
    from expann_amd import _lib
    h = C.c_void_p()
    assert _lib.load().expann_create(dim, PQ4, metric, 0, C.byref(h)) == code
    assert not h.value


def test_pack_and_unpack():
    from expann_amd import pack_pq4, unpack_pq4
    codes = np.random.default_rng(0).integers(0, 16, (7, 48), dtype=np.uint8)
    rows = pack_pq4(codes)
    assert rows.dtype == np.uint8 and np.array_equal(rows, codes[:, 0::2] + 16 * codes[:, 1::2])
    assert np.array_equal(unpack_pq4(rows), codes)


# "metric dim M m k cap" -> status, family, query tile
PLANS = [("0 128 16 1 10 2048", 0, GEMM_I8, 64), ("1 2048 256 1000 10 2048", 0, GEMM_I8, 64),
         ("0 144 48 9 8192 16384", 0, GEMM_I8, 64),
         # M below 16, no multiple of 16, not dividing dim: no tile
         ("0 128 8 9 10 2048", 0, GEMM_I8, 0), ("0 120 24 9 10 2048", 0, GEMM_I8, 0), ("0 100 32 9 10 2048", 0, GEMM_I8, 0),
         ("0 128 16 1000 8193 16384", UNSUPPORTED, 0, 64),  # k beyond 8 192, k beyond half the lists
         ("0 128 16 1000 2000 2048", UNSUPPORTED, 0, 64),
         ("3 128 16 1000 10 2048", UNSUPPORTED, 0, 64)]    # a metric it does not take


def test_the_plan_of_pq4_rows(tmp_path):
    exe = tmp_path / "pq4_plan_hook"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "expann_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "pq4_plan_hook.cpp"), "-o", str(exe)])
    text = "".join(case[0] + "\n" for case in PLANS)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(PLANS)
    for case, line in zip(PLANS, out):
        status, family, tq, sampled = (int(x) for x in line.split())
        assert (status, family, tq, sampled) == case[1:] + (0,), (case, line)


def test_the_rule_on_four_rows_worked_by_hand():
    """M = 16, dsub = 1, inner product, the query is 1 everywhere, so T = -cb.  T[0][c] = 34 c, T[i][c] = c + i for i >= 1:
    lo_0 = 0, lo_i = i, bias = 120; span = 510, r = 0.5, step = 2.  u[0][c] = 17 c; u[i][c] = rint(c / 2), half to even:
    u[i][1] = 0, u[i][3] = 2, u[i][5] = 2.  Rows: all codes 0 -> S = 0; all 1 -> 17 + 15 * 0; all 3 -> 51 + 15 * 2 = 81;
    15 then 5s -> 255 + 15 * 2 = 285.  Distances 120 + 2 S."""
    from test_gpu_pq4 import reference
    cb = -(np.arange(16.0) + np.arange(16.0)[:, None])
    cb[0] = -34.0 * np.arange(16)
    cb = cb.astype(np.float32)[:, :, None]
    codes = np.array([[0] * 16, [1] * 16, [3] * 16, [15] + [5] * 15], dtype=np.uint8)
    ids, dists = reference(cb, codes, np.ones((1, 16), np.float32), 5, "ip", id_offset=10)
    assert ids[0].tolist() == [10, 11, 12, 13, 2 ** 64 - 1] and dists[0].tolist() == [120.0, 154.0, 282.0, 690.0, np.inf]
