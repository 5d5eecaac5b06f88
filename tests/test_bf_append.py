"""The rules of an append to a built brute-force index (expann_amd/csrc/bf_append.hpp), without a device.

tests/native/bf_append_hook.cpp, a stand-alone program that includes nothing but that header, prints what the header
decides for the cases it reads.  The expectations below are written out by hand from include/expann_hip.h's text --
the scale rule 2^floor(log2(32768 / max |v|)), the order of the errors, the growth by half -- not read from the code
under test.  The program is built with the address and undefined-behaviour sanitizers where g++ has their static
runtimes, else without."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, NOT_BUILT, UNSUPPORTED = 0, 1, 4, 5
MAX_ROWS = 2 ** 32 - 32


@pytest.fixture(scope="module")
def hook(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bf_append") / "bf_append_hook"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "expann_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "bf_append_hook.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:  # (no static sanitizer runtimes here)
        subprocess.check_call(cmd)

    def ask(*lines):
        r = subprocess.run([str(exe)], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = [ln.split("\t") for ln in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return ask


def _plan(fields):
    status, n, capacity, realloc, copies = fields
    return dict(status=int(status), n=int(n), capacity=int(capacity), realloc=int(realloc), copies=copies)


BUILT = "on_device=1 owned=1 n=4500 capacity=4500"
COPY = BUILT + " f16_scale=16384 state_maxabs=1.5"  # (2^14: the scale of max |v| = 1.5)


def test_f16_scale_for(hook):
    cases = [("1.5", 2.0 ** 14, 1), ("1.9", 2.0 ** 14, 1), ("2.5", 2.0 ** 13, 1), ("2.0", 2.0 ** 14, 1), ("1.0", 2.0 ** 15, 1),
             ("32768", 1.0, 1), ("32769", 0.5, 1), ("0", 1.0, 1), ("1e-30", 2.0 ** 40, 1),  # (the exponent is clamped to +-40)
             ("inf", None, 0), ("nan", None, 0), ("1e30", None, 0)]
    got = hook(*[f"scale maxabs={v}" for v, _, _ in cases])
    for (v, scale, usable), (g_scale, g_usable) in zip(cases, got):
        assert int(g_usable) == usable, v
        if usable:
            assert float(g_scale) == scale, v


def test_what_happens_to_the_fp16_copy(hook):
    cases = [
        (COPY + " n_new=1 maxabs_new=1.9", "extend"),      # 1.9 -> 2^14 still
        (COPY + " n_new=1 maxabs_new=2.0", "extend"),      # 32768 / 2 = 2^14 exactly
        (COPY + " n_new=1 maxabs_new=0.01", "extend"),     # the maximum is the old rows'
        (COPY + " n_new=1 maxabs_new=0", "extend"),
        (COPY + " n_new=1 maxabs_new=2.5", "drop"),        # 2^13
        (COPY + " n_new=1 maxabs_new=nan", "drop"),        # (the rebuilt copy is then marked unusable)
        (COPY + " n_new=1 maxabs_new=inf", "drop"),
        (BUILT + " n_new=1 maxabs_new=2.5", "nothing"),    # no copy yet
        (BUILT + " f16_scale=-1 state_maxabs=1e30 n_new=1 maxabs_new=1.0", "nothing"),  # unusable stays unusable
        (COPY + " float_rows=0 n_new=1 maxabs_new=2.5", "nothing"),  # U8 / I8 / I16 rows
        (COPY + " n_new=0 maxabs_new=2.5", "nothing"),     # nothing appended
    ]
    got = hook(*["append " + c for c, _ in cases])
    for (c, want), g in zip(cases, got):
        p = _plan(g)
        assert p["status"] == OK and p["copies"] == want, (c, p)


def test_the_order_of_the_errors(hook):
    huge = MAX_ROWS
    cases = [
        ("have_handle=0 have_rows=0 n_new=5", INVALID_ARG),
        ("have_handle=0 " + BUILT + " n_new=5", INVALID_ARG),
        ("have_rows=0 n_new=5", INVALID_ARG),                      # NULL rows before "not built"
        ("have_rows=0 on_device=1 owned=0 n=10 capacity=0 n_new=5", INVALID_ARG),
        ("have_rows=0 n_new=0", NOT_BUILT),                        # (NULL rows are fine with n == 0)
        ("n_new=5", NOT_BUILT),
        (f"n_new={huge}", NOT_BUILT),                              # before the bound
        ("on_device=1 owned=0 n=10 capacity=0 n_new=5", UNSUPPORTED),  # adopted rows
        ("on_device=1 owned=0 n=10 capacity=0 n_new=0", UNSUPPORTED),
        (BUILT + f" n_new={MAX_ROWS - 4500}", UNSUPPORTED),        # n + size >= 2^32 - 32
        (BUILT + f" n_new={2 ** 40}", UNSUPPORTED),
        (BUILT + f" n_new={MAX_ROWS - 4501}", OK),
        (BUILT + " have_rows=0 n_new=0", OK),
    ]
    got = hook(*["append " + c for c, _ in cases])
    for (c, want), g in zip(cases, got):
        p = _plan(g)
        assert p["status"] == want, (c, p)
        if want != OK:
            assert p["realloc"] == 0 and p["copies"] == "nothing", (c, p)


def test_capacity(hook):
    got = [_plan(g) for g in hook(
        "append on_device=1 owned=1 n=4500 capacity=12000 n_new=100 maxabs_new=0",
        "append on_device=1 owned=1 n=4500 capacity=4600 n_new=100 maxabs_new=0",
        "append " + BUILT + " n_new=1 maxabs_new=0",
        "append " + BUILT + " n_new=5000 maxabs_new=0",
        "append " + BUILT + " n_new=0 maxabs_new=0")]
    assert got[0] == dict(status=OK, n=4600, capacity=12000, realloc=0, copies="nothing")
    assert got[1] == dict(status=OK, n=4600, capacity=4600, realloc=0, copies="nothing")
    assert got[2] == dict(status=OK, n=4501, capacity=6750, realloc=1, copies="nothing")   # by half
    assert got[3] == dict(status=OK, n=9500, capacity=9500, realloc=1, copies="nothing")   # ... or what is needed
    assert got[4] == dict(status=OK, n=4500, capacity=4500, realloc=0, copies="nothing")


def test_geometric_growth(hook):
    """64 appends of 100 rows onto 4 500: at most 6 reallocations, where one per append would be 64"""
    (reallocs, capacity), = hook("grow n=4500 step=100 count=64")
    assert 1 <= int(reallocs) <= 6
    assert int(capacity) >= 4500 + 64 * 100
    (reallocs, capacity), = hook("grow n=1000000 step=1 count=3000")
    assert int(reallocs) == 1 and int(capacity) == 1500000


def test_reserve(hook):
    got = [_plan(g) for g in hook(
        "reserve " + BUILT + " n_rows=12000",
        "reserve " + BUILT + " n_rows=4500",
        "reserve " + BUILT + " n_rows=100",
        "reserve on_device=1 owned=0 n=10 capacity=0 n_rows=5",
        "reserve n_rows=12000",                       # before build(): remembered by the caller, nothing to reallocate
        "reserve have_handle=0 n_rows=12000",
        "reserve " + BUILT + f" n_rows={MAX_ROWS}")]
    assert got[0]["status"] == OK and got[0]["realloc"] == 1 and got[0]["capacity"] == 12000 and got[0]["n"] == 4500
    assert got[1]["status"] == OK and got[1]["realloc"] == 0 and got[1]["capacity"] == 4500
    assert got[2]["status"] == OK and got[2]["realloc"] == 0 and got[2]["capacity"] == 4500
    assert got[3]["status"] == UNSUPPORTED
    assert got[4]["status"] == OK and got[4]["realloc"] == 0
    assert got[5]["status"] == INVALID_ARG
    assert got[6]["status"] == UNSUPPORTED


def test_the_rules_are_one_header_that_needs_no_hip():
    text = open(os.path.join(ROOT, "expann_amd", "csrc", "bf_append.hpp")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)
    assert includes and all("hip/" not in i and not i.endswith(".hpp") for i in includes), includes
    # the engine builds its copy with the header's rule and decides no scale by itself
    engine = open(os.path.join(ROOT, "expann_amd", "csrc", "expann_hip.hip")).read()
    assert "f16_scale_for(" in engine and "plan_append(" in engine and "plan_reserve(" in engine
    assert not re.search(r"log2\(\s*32768", engine)
