"""The rules of a remove from a built brute-force index (expann_amd/csrc/bf_remove.hpp), without a device.

tests/native/bf_remove_hook.cpp, a stand-alone program that includes nothing but that header, prints what the header
decides for the cases it reads.  The expectations below are written out by hand from include/expann_hip.h's text --
THE REMOVE RULE: the order of the errors, the fate of the fp16 copy by the scale rule 2^floor(log2(32768 / max |v|)),
the order-preserving shift of the ids, "an index is never empty" -- not read from the code under test.  The program is
built with the address and undefined-behaviour sanitizers where g++ has their static runtimes, else without."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, NOT_BUILT, UNSUPPORTED = 0, 1, 4, 5


@pytest.fixture(scope="module")
def hook(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bf_remove") / "bf_remove_hook"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "expann_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "bf_remove_hook.cpp"), "-o", str(exe)]
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


BUILT = "on_device=1 owned=1 n=4500 capacity=4500"
ADOPTED = "on_device=1 owned=0 n=10 capacity=0"
COPY14 = BUILT + " f16_scale=16384"   # 2^14: the scale of 1 < max |v| <= 2
COPY13 = BUILT + " f16_scale=8192"    # 2^13: the scale of 2 < max |v| <= 4


def test_the_order_of_the_errors(hook):
    cases = [
        ("have_handle=0 have_ids=0 n_ids=5", INVALID_ARG),
        ("have_handle=0 " + BUILT + " n_ids=5", INVALID_ARG),
        ("have_ids=0 n_ids=5", INVALID_ARG),                  # NULL ids before "not built"
        ("have_ids=0 " + ADOPTED + " n_ids=5", INVALID_ARG),  # ... and before "adopted"
        ("have_ids=0 n_ids=0", NOT_BUILT),                    # (NULL ids are fine with n_ids == 0)
        ("n_ids=5", NOT_BUILT),
        ("n_ids=0", NOT_BUILT),
        (ADOPTED + " n_ids=5", UNSUPPORTED),
        (ADOPTED + " n_ids=0", UNSUPPORTED),
        (BUILT + " n_ids=5", OK),
        (BUILT + " have_ids=0 n_ids=0", OK),
    ]
    got = hook(*["check " + c for c, _ in cases])
    for (c, want), (status,) in zip(cases, got):
        assert int(status) == want, c
    # the same four come first when the mark pass has something to say as well
    got = hook(*["remove " + c + " bad_id=1 survivors=0 maxabs=1" for c, _ in cases])
    for (c, want), (status, n, copies) in zip(cases, got):
        if want != OK:
            assert int(status) == want and copies == "nothing", c
    # n_ids == 0 does nothing, whatever else is said
    (status, n, copies), = hook("remove " + COPY14 + " n_ids=0 bad_id=1 survivors=0 maxabs=9")
    assert (int(status), int(n), copies) == (OK, 4500, "nothing")


def test_a_bad_id_and_an_empty_index_are_refused(hook):
    got = hook(
        "remove " + COPY14 + " n_ids=3 bad_id=1 survivors=4498 maxabs=1.5",   # an id at or beyond size()
        "remove " + COPY14 + " n_ids=4500 bad_id=0 survivors=0 maxabs=0",     # would leave no row
        "remove " + BUILT + " float_rows=0 n_ids=9000 bad_id=0 survivors=0 maxabs=0",
        "remove " + COPY14 + " n_ids=4499 bad_id=0 survivors=1 maxabs=1.5",   # one row may stay
        "remove " + COPY14 + " n_ids=4500 bad_id=1 survivors=0 maxabs=0")     # (the bad id is named first)
    for g in (got[0], got[1], got[2], got[4]):
        assert int(g[0]) == INVALID_ARG and int(g[1]) == 4500 and g[2] == "nothing", g   # the handle keeps its rows
    assert (int(got[3][0]), int(got[3][1]), got[3][2]) == (OK, 1, "compact")


def test_what_happens_to_the_fp16_copy(hook):
    cases = [
        # max |v| 1.9 -> 1.5: both 2^14, the copy is compacted
        (COPY14 + " state_maxabs=1.9 n_ids=1 survivors=4499 maxabs=1.5", "compact"),
        (COPY14 + " state_maxabs=1.9 n_ids=1 survivors=4499 maxabs=1.9", "compact"),   # the maximum stayed
        (COPY14 + " state_maxabs=2.0 n_ids=1 survivors=4499 maxabs=1.0001", "compact"),
        # 2.5 -> 1.5: 2^13 -> 2^14, the copy is dropped
        (COPY13 + " state_maxabs=2.5 n_ids=1 survivors=4499 maxabs=1.5", "drop"),
        (COPY14 + " state_maxabs=1.9 n_ids=1 survivors=4499 maxabs=1.0", "drop"),      # 1.0 -> 2^15
        (COPY14 + " state_maxabs=1.9 n_ids=1 survivors=4499 maxabs=0", "drop"),        # all-zero survivors: scale 1
        # rows marked unusable: the mark is forgotten, whatever the survivors hold
        (BUILT + " f16_scale=-1 state_maxabs=1e30 n_ids=1 survivors=4499 maxabs=1.5", "drop"),
        (BUILT + " f16_scale=-1 state_maxabs=nan n_ids=1 survivors=4499 maxabs=0", "drop"),
        # no copy yet
        (BUILT + " n_ids=1 survivors=4499 maxabs=1.5", "nothing"),
        # 8-bit / int16 rows
        (COPY14 + " float_rows=0 n_ids=1 survivors=4499 maxabs=1.5", "nothing"),
        (BUILT + " float_rows=0 n_ids=1 survivors=4499 maxabs=0", "nothing"),
    ]
    got = hook(*["remove " + c for c, _ in cases])
    for (c, want), (status, n, copies) in zip(cases, got):
        assert (int(status), int(n), copies) == (OK, 4499, want), c


def test_the_new_ids_on_a_hand_made_bitmap(hook):
    # 96 rows; removed: 0, 5, 31 (word 0), all of word 1 but row 40, and 95 (the last row)
    w0 = 0xFFFFFFFF & ~(1 << 0) & ~(1 << 5) & ~(1 << 31)
    w1 = 1 << (40 - 32)
    w2 = 0xFFFFFFFF & ~(1 << 31)
    (total, pairs), = hook(f"newid bits={w0:x},{w1:x},{w2:x}")
    got = dict(tuple(int(x) for x in p.split(":")) for p in pairs.split(","))
    removed = {0, 5, 31, 95} | (set(range(32, 64)) - {40})
    want = {}
    for i in range(96):
        if i not in removed:
            want[i] = i - sum(1 for s in removed if s < i)   # THE REMOVE RULE's shift, as the header states it
    assert int(total) == 96 - len(removed) == 61
    assert got == want
    assert got[1] == 0 and got[6] == 4 and got[30] == 28 and got[40] == 29 and got[64] == 30 and got[94] == 60
    # nothing removed: every row keeps its id; everything but one row removed: it becomes row 0
    (total, pairs), = hook("newid bits=ffffffff,ffffffff")
    assert int(total) == 64 and pairs.split(",")[37] == "37:37"
    (total, pairs), = hook("newid bits=0,0,0,8000")
    assert int(total) == 1 and pairs == "111:0"


def test_the_rules_are_one_header_that_needs_no_hip():
    text = open(os.path.join(ROOT, "expann_amd", "csrc", "bf_remove.hpp")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)
    assert includes and all("hip/" not in i for i in includes), includes
    assert [i for i in includes if i.endswith(".hpp")] == ["bf_append.hpp"]   # (the scale rule: itself without HIP)
    # the engine carries the header's answers out and decides no fate by itself
    engine = open(os.path.join(ROOT, "expann_amd", "csrc", "expann_hip.hip")).read()
    assert "plan_remove(" in engine and "keep_words(" in engine
    body = engine[engine.index("---- remove (DESIGN.md 4.6j)"):engine.index("int expann_compact_row_filter(")]
    assert "f16_scale_for(" not in body
