"""expann_search_asym_i8 at the ABI and in the planner, without a device: the refusals that come before any device
work, Python's own check of the query array, and plan_asym / plan_asym_tiles through tests/native/asym_plan_hook.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = 1, 5
GEMM_I8 = 7  # ScanFamily::kHamming, the value it shares with kGemmI8


def test_null_handle_and_null_queries_are_refused():
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_search_asym_i8(None, None, 1, 1, None, None) == INVALID_ARG
    assert L.expann_search_asym_i8_device(None, None, 1, 1, None, None, None) == INVALID_ARG


@pytest.mark.parametrize("queries", [np.zeros((2, 64), np.float32), np.zeros((2, 64), np.uint8), np.zeros((2, 8), np.int8),
                                     np.zeros(64, np.int8)])
def test_python_refuses_what_is_not_int8_m_by_dim(queries):
    from expann_amd import GpuBruteForceEngine
    eng = object.__new__(GpuBruteForceEngine)  # (no handle: the check comes before the call)
    eng.dim = 64
    with pytest.raises(ValueError):
        eng.query_k_batch_asym(queries, 1)


# int_mode k cap n sel_rows first last -> status family n_tiles_sel tile_stride fixed
PLANS = [("5 10 2048 1061 1024 1 0", (0, GEMM_I8, 2, 1, 1024)),       # level 0: the whole tiles of its sample
         ("5 10 2048 1061 1072 1 1", (0, GEMM_I8, 3, 1, 1536)),       # one level: every tile, the ragged one included
         ("5 10 2048 1000000 1024 1 0", (0, GEMM_I8, 2, 977, 1024)),  # a strided sample (1 954 tiles)
         ("5 10 2048 1000000 32768 0 0", (0, GEMM_I8, 64, 30, 2048)),
         ("5 10 2048 1000000 1000000 0 1", (0, GEMM_I8, 1954, 1, 2048)),
         ("5 300 16384 100 112 1 1", (0, GEMM_I8, 1, 1, 512)),
         ("5 8192 16384 1000 1008 1 1", (0, GEMM_I8, 2, 1, 1024)),
         ("5 8193 16384 1000 1008 1 1", (UNSUPPORTED, 0, 2, 1, 1024)),
         ("3 10 2048 1000 1008 1 1", (UNSUPPORTED, 0, 2, 1, 1024))]     # int8 rows: not this entry point's


def test_the_plan(tmp_path):
    exe = tmp_path / "asym_plan_hook"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "expann_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "asym_plan_hook.cpp"), "-o", str(exe)])
    text = "".join(case[0] + "\n" for case in PLANS)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert [tuple(int(v) for v in line.split()) for line in out] == [case[1] for case in PLANS]
