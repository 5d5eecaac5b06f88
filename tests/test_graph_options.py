"""The option table of the graph handle (expann_amd/csrc/graph_options.hpp), without a device.

tests/native/graph_options_hook.cpp, a stand-alone program that includes nothing but that header, prints every row
of the table: its default, and what a set of each probe value stores and returns.  The expectations below are written
out from the rules the C ABI documents -- "filter_flat_rows" any count >= 0; "cand_capacity" 0 or a power of two in
[8, 2^20]; "redo_capacity" 0 or a power of two in [8, 8192] -- not read from the code under test.  The program is
built with the address and undefined-behaviour sanitizers where g++ has their static runtimes (a statically linked
runtime starts whatever else the loader brings in first), else without."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG = 0, 1

PROBES = [-1, 0, 1, 7, 8, 12, 4096, 8192, 16384, 2 ** 20, 2 ** 21]
# name: (default, stored value per probe on a fresh table, return code per probe); a refused value leaves the default
EXPECT = {
    "filter_flat_rows": (0, [0, 0, 1, 7, 8, 12, 4096, 8192, 16384, 2 ** 20, 2 ** 21],
                         [INVALID_ARG] + [OK] * 10),
    "cand_capacity": (0, [0, 0, 0, 0, 8, 0, 4096, 8192, 16384, 2 ** 20, 0],
                      [INVALID_ARG, OK, INVALID_ARG, INVALID_ARG, OK, INVALID_ARG, OK, OK, OK, OK, INVALID_ARG]),
    "redo_capacity": (0, [0, 0, 0, 0, 8, 0, 4096, 8192, 0, 0, 0],
                      [INVALID_ARG, OK, INVALID_ARG, INVALID_ARG, OK, INVALID_ARG, OK, OK, INVALID_ARG, INVALID_ARG,
                       INVALID_ARG]),
}
REFUSAL = {
    "filter_flat_rows": "filter_flat_rows must be >= 0 (0 = auto)",
    "cand_capacity": "cand_capacity must be 0 or a power of two >= 8",
    "redo_capacity": "redo_capacity must be 0 or a power of two >= 8 and <= 8192",
}
# what expann_graph_get_stat answers to
STATS = ["redo_queries", "redo_overflows", "deferred_searches", "distcomps", "redo_kernel_ns", "filter_active",
         "filter_rows", "flat_searches", "groups_active", "group_count", "group_walk_queries", "group_scan_queries",
         "group_pad_queries", "vector_bytes"]


@pytest.fixture(scope="module")
def hook(tmp_path_factory):
    exe = tmp_path_factory.mktemp("graph_options") / "graph_options_hook"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "expann_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "graph_options_hook.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:  # (no static sanitizer runtimes here)
        subprocess.check_call(cmd)

    def run(*args):
        r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return [line.split("\t") for line in r.stdout.splitlines()]
    return run


def test_every_row_has_the_documented_default_and_rule(hook):
    rows, sets = {}, {}
    for f in hook("table"):
        if f[0] == "row":
            assert f[1] not in rows, f"{f[1]} has two rows"
            rows[f[1]] = int(f[2])
        else:
            assert f[0] == "set"
            sets.setdefault(f[1], []).append((int(f[2]), int(f[3]), int(f[4]), f[5]))
    assert sorted(rows) == sorted(EXPECT)
    for name, (default, stored, codes) in EXPECT.items():
        assert rows[name] == default, name
        got = sets[name]
        assert [g[0] for g in got] == PROBES, name
        assert [g[1] for g in got] == stored, name
        assert [g[2] for g in got] == codes, name
        for v, _, rc, text in got:
            assert text == ("-" if rc == OK else REFUSAL[name]), (name, v)


@pytest.mark.parametrize("name,kept,refused", [("filter_flat_rows", 4096, -1), ("cand_capacity", 4096, 12),
                                               ("cand_capacity", 8, 2 ** 21), ("redo_capacity", 8192, 16384),
                                               ("redo_capacity", 8, 7)])
def test_a_refused_value_leaves_the_stored_one(hook, name, kept, refused):
    others = [f"{n}=0" for n in EXPECT if n != name]
    first, second = hook("set", name, kept, refused)
    assert first[:2] == [str(OK), "-"] and second[:2] == [str(INVALID_ARG), REFUSAL[name]]
    for line in (first, second):
        assert sorted(line[2:]) == sorted(others + [f"{name}={kept}"])


@pytest.mark.parametrize("name", ["", "Cand_capacity", "cand_capacity ", "opt_cand_cap", "cand_cap", "no_such_option"])
def test_an_unknown_name_is_refused_and_changes_nothing(hook, name):
    unchanged = sorted(f"{n}=0" for n in EXPECT)
    for line in hook("set", name, 8, 0):
        assert line[:2] == [str(INVALID_ARG), "unknown option: " + name]
        assert sorted(line[2:]) == unchanged


def _comment_before(text, decl):
    at = text.index(decl)
    return text[text.rindex("/*", 0, at):at]


def test_the_header_names_every_option_and_every_statistic():
    text = open(os.path.join(ROOT, "include", "expann_hip.h")).read()
    options = _comment_before(text, "int expann_graph_set_option(expann_graph* g")
    for name in EXPECT:
        assert re.search(r'"%s"' % re.escape(name), options), f'"{name}" is not in the option comment of expann_hip.h'
    stats = _comment_before(text, "int expann_graph_get_stat(expann_graph* g")
    for name in STATS:
        assert re.search(r'"%s"' % re.escape(name), stats), f'"{name}" is not in the statistics comment of expann_hip.h'
    # the table behind expann_graph_get_stat has these names and no others
    src = open(os.path.join(ROOT, "expann_amd", "csrc", "expann_graph.hip")).read()
    table = src[src.index("kGraphStatTable[] = {"):]
    table = table[:table.index("};")]
    assert re.findall(r'\{"(\w+)",', table) == STATS
