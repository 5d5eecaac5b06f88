"""EXPANN_DTYPE_PQ8 at the ABI and in the planner, without a device: expann_create's checks that come before the
device lookup, plan_pq and plan_pq_chunks through tests/native/pq_plan_hook.cpp (the existing hook cannot name M),
and THE PQ RULE on a four-row example worked by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = 1, 5
PQ8 = 7
L2, IP, L2_REFCOMPAT, HAMMING = 0, 1, 2, 3


@pytest.mark.parametrize("dim,metric,code", [(128, HAMMING, INVALID_ARG), (128, L2_REFCOMPAT, INVALID_ARG), (0, L2, INVALID_ARG),
                                             (7, IP, INVALID_ARG), (4097, L2, UNSUPPORTED)])
def test_create_refuses_before_the_device(dim, metric, code):
    from expann_amd import _lib
    h = C.c_void_p()
    assert _lib.load().expann_create(dim, PQ8, metric, 0, C.byref(h)) == code
    assert not h.value


# "metric dim M m k cap query_tile n_groups n_qtiles slots" -> status, direct_tq, chunks (1 M rows: rows / (3 840 dsub), or a
# chunk per slot where that is more)
PLANS = [("1 128 16 1000 10 2048 0 65536 125 256", 0, 8, 34),      # the classes of M at their boundaries
         ("0 192 24 1000 10 2048 0 65536 125 256", 0, 4, 34),
         ("0 128 32 1000 10 2048 0 65536 125 256", 0, 4, 68),
         ("0 128 64 1000 10 2048 0 65536 125 256", 0, 2, 136),
         ("0 216 72 1000 10 2048 0 65536 125 256", 0, 1, 91),
         ("0 1024 128 1000 10 2048 0 65536 125 256", 0, 1, 34),
         ("0 128 16 1 10 2048 0 65536 1 512", 0, 1, 512),          # one query: TQ = 1, a chunk per slot
         ("0 128 64 9 10 2048 0 65536 5 256", 0, 2, 136),
         ("0 128 16 1000 10 2048 4 64 250 256", 0, 4, 2),          # "query_tile" inside the class; a step per chunk at least
         ("0 128 64 1000 10 2048 4 64 250 256", 0, 0, 2),          # ... and outside it: no instance
         ("0 128 12 1000 10 2048 0 64 125 256", 0, 0, 3),          # M that is no multiple of 8
         ("0 128 16 1000 8193 16384 0 64 125 256", UNSUPPORTED, 8, 3),   # k beyond 8 192, k beyond half the lists
         ("0 128 16 1000 2000 2048 0 64 125 256", UNSUPPORTED, 8, 3),
         ("3 128 16 1000 10 2048 0 64 125 256", UNSUPPORTED, 8, 3)]


def test_the_plan_of_product_quantised_rows(tmp_path):
    exe = tmp_path / "pq_plan_hook"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "expann_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "pq_plan_hook.cpp"), "-o", str(exe)])
    text = "".join(case[0] + "\n" for case in PLANS)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(PLANS)
    for case, line in zip(PLANS, out):
        status, family, tq, sampled, chunks = (int(x) for x in line.split())
        assert (status, tq, chunks) == case[1:], (case, line)
        assert family == 0 and sampled == (status == 0)  # the direct family, its sampled class minima


def test_the_rule_on_four_rows_worked_by_hand():
    """M = 8, dsub = 1, centroid c of sub-quantiser i is c / 4 + i; the query is 1 everywhere.
    L2 entry: (1 - c/4 - i)^2; IP entry: c/4 + i.  Rows: all codes 0; all codes 4; code i = 4 i; codes 4, 0, 0, ...
    L2: sum (1-i)^2 = 1+0+1+4+9+16+25+36 = 92; sum i^2 = 140; sum (1-2i)^2 = 1+1+9+25+49+81+121+169 = 456;
        0 + (92 - 1) = 91.   IP: -(0+..+7) = -28; -(28 + 8) = -36; -(28 + 28) = -56; -(28 + 1) = -29."""
    from test_gpu_pq import reference
    cb = (np.arange(256) / 4.0 + np.arange(8)[:, None]).astype(np.float32)[:, :, None]
    codes = np.array([[0] * 8, [4] * 8, [4 * i for i in range(8)], [4] + [0] * 7], dtype=np.uint8)
    q = np.ones((1, 8), np.float32)
    ids, dists = reference(cb, codes, q, 5, "l2")
    assert ids[0].tolist() == [3, 0, 1, 2, 2 ** 64 - 1] and dists[0].tolist() == [91.0, 92.0, 140.0, 456.0, np.inf]
    ids, dists = reference(cb, codes, q, 4, "ip", id_offset=10)
    assert ids[0].tolist() == [12, 11, 13, 10] and dists[0].tolist() == [-56.0, -36.0, -29.0, -28.0]
