"""CPU check of the oracle's batched-builder restatement (oracle_graph_build_batched): with batches of one it
is the serial algorithm, so it must reproduce the serial host builder of include/expann/antitopo_index.h
(reached without a device through tests/native/serial_build_hook.cpp) edge for edge and in row order --
Gaussian rows and integer rows with exact duplicates, one case with a nonzero ortho_bias (the hook is compiled
by g++ at its default contraction setting, the oracle by gcc with -ffp-contract=off)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from graph_build_helpers import Params, Strided, contraction_case, draw_levels, sift_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def serial(tmp_path_factory):
    so = tmp_path_factory.mktemp("native") / "serial_build_hook.so"
    subprocess.check_call(["g++", "-O2", "-march=x86-64-v3", "-std=c++17", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "serial_build_hook.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.serial_build.restype = C.c_int
    return lib


def _serial_build(lib, st, p):
    vp, sz = C.c_void_p, C.c_size_t
    ml, sv = C.c_uint32(0), C.c_uint32(0)
    rc = lib.serial_build(sz(st.dim), vp(st.vec.ctypes.data), sz(st.n), vp(st.levels.ctypes.data), sz(st.M), sz(st.M0),
                          sz(p.ef), sz(p.prune_overflow), C.c_float(p.ortho_factor), C.c_float(p.ortho_bias),
                          vp(st.ids0.ctypes.data), vp(st.d0.ctypes.data), vp(st.deg0.ctypes.data), sz(st.stride0),
                          vp(st.upper_idx.ctypes.data), sz(st.U), vp(st.idsu.ctypes.data), vp(st.du.ctypes.data),
                          vp(st.degu.ctypes.data), sz(st.strideu), C.byref(ml), C.byref(sv))
    assert rc == 0
    st.max_layer, st.sv = ml.value, sv.value


@pytest.mark.parametrize("kind,p", [("gauss", Params(40)), ("gauss", Params(40, 1, 1.5, 0.1)),
                                    ("ties", Params(32, 1)), ("ties", Params(32, 0, 0.5, 0.25))],
                         ids=["gauss", "gauss-bias", "ties", "ties-bias"])
def test_batches_of_one_are_the_serial_builder(serial, kind, p):
    rng = np.random.RandomState(400)
    n, d, M = 400, 64, 6
    if kind == "gauss":
        vec = rng.standard_normal((n, d)).astype(np.float32)
    else:
        vec = sift_like(rng, n, d)
        dup = rng.choice(np.arange(20, n), n // 20, replace=False)
        vec[dup] = vec[rng.randint(0, 20, dup.size)]   # exact duplicates of earlier rows
    levels = draw_levels(rng, n, M)
    assert levels.max() >= 2
    a = Strided(vec, levels, M, 2 * M, slack=1)       # (a serial row never holds more than cap + 1 entries)
    b = Strided(vec, levels, M, 2 * M, slack=1)
    r = a.oracle_build(n, 1, p, max_batch=1)
    _serial_build(serial, b, p)
    assert int(r["stats"][0]) == n - 1 and int(r["stats"][1]) == 0 and int(r["stats"][2]) > 0
    assert (a.max_layer, a.sv) == (b.max_layer, b.sv)
    assert a.max_layer == int(levels.max()) + 1
    for (name, ia, da, ga, stride, _), (_, ib, db, gb, _, _) in zip(a.groups(), b.groups()):
        assert np.array_equal(ga, gb), name
        live = np.arange(stride)[None, :] < ga[:, None]
        assert not (((ia != ib) | (da != db)) & live).any(), name
    if kind == "ties":
        assert r["tie_hazards"] > 0
        z = (a.d0 == 0) & (np.arange(a.stride0)[None, :] < a.deg0[:, None])
        assert z.any(), "no edge of length 0 between distinct vertices"


@pytest.mark.parametrize("which", [0, 1])
def test_score_is_not_contracted(serial, which):
    """rows on which one fused multiply-add in the score changes the order of a row: the oracle and the serial
    host builder (compiled here for a target that has FMA, at the compiler's default contraction setting) both
    give the row that two rounded operations give"""
    vec, p, row = contraction_case(64, which)
    lv = np.zeros(4, np.uint8)
    a, b = Strided(vec, lv, 4, 8, slack=1), Strided(vec, lv, 4, 8, slack=1)
    a.oracle_build(4, 1, p, max_batch=1)
    _serial_build(serial, b, p)
    assert a.ids0[3, :a.deg0[3]].tolist() == row
    assert b.ids0[3, :b.deg0[3]].tolist() == row
    assert sorted(a.d0[3, :3].tolist()) == [3.0, 6.0, 15.0]


def test_batch_rule():
    """b1 = min(n, b0 + min(max_batch or 32768, max(1, b0 / 16))), cut before the first vertex whose level is
    >= max_layer; such a vertex goes alone when it comes first"""
    import oracle_ctypes as oc
    lv = np.zeros(100000, np.uint8)
    assert oc.graph_batch_end(lv, 100000, 1, 1) == 2
    assert oc.graph_batch_end(lv, 100000, 31, 1) == 32
    assert oc.graph_batch_end(lv, 100000, 32, 1) == 34
    assert oc.graph_batch_end(lv, 100000, 1600, 1) == 1700
    assert oc.graph_batch_end(lv, 1650, 1600, 1) == 1650
    assert oc.graph_batch_end(lv, 100000, 1600, 1, 7) == 1607
    assert oc.graph_batch_end(lv, 100000, 99000, 1) == 100000
    lv[1650] = 1
    assert oc.graph_batch_end(lv, 100000, 1600, 1) == 1650
    assert oc.graph_batch_end(lv, 100000, 1600, 2) == 1700
    assert oc.graph_batch_end(lv, 100000, 1650, 1) == 1651
