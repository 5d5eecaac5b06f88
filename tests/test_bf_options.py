"""The option table of the brute-force handle (expann_amd/csrc/bf_options.hpp), without a device.

tests/native/bf_options_hook.cpp, a stand-alone program that includes nothing but that header, prints every row of
the table: its default, its environment variable, and what a set of each probe value stores and returns.  The
expectations below are written out from the rules the C ABI documents, not read from the code under test.  The
program is built with the address and undefined-behaviour sanitizers where g++ has their static runtimes (a
statically linked runtime starts whatever else the loader brings in first), else without."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 5

PROBES = [-5, -1, 0, 1, 2, 3, 64, 65, 16384, 16385, 1000000]
AS_GIVEN = [-5, -1, 0, 1, 2, 3, 64, 65, 16384, 16385, 1000000]
CLAMP_0_2 = [0, 0, 0, 1, 2, 2, 2, 2, 2, 2, 2]
AT_LEAST_0 = [0, 0, 0, 1, 2, 3, 64, 65, 16384, 16385, 1000000]
AT_LEAST_2 = [2, 2, 2, 2, 2, 3, 64, 65, 16384, 16385, 1000000]
CLAMP_1_64 = [1, 1, 1, 1, 2, 3, 64, 64, 64, 64, 64]
ONE_OR_TWO = [2, 2, 2, 1, 2, 2, 2, 2, 2, 2, 2]
FLAG = [1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1]
ALL_OK = [OK] * len(PROBES)

# name: (default, environment variable, stored value per probe, return code per probe)
EXPECT = {
    "query_tile": (0, None, AS_GIVEN, ALL_OK),
    "cand_capacity": (0, None, AS_GIVEN, ALL_OK),
    "debug": (0, None, AS_GIVEN, ALL_OK),
    "scan_kernel": (0, None, AS_GIVEN, ALL_OK),
    "scan_chunks": (0, None, AS_GIVEN, ALL_OK),
    "ip_rescale": (1, None, AS_GIVEN, ALL_OK),
    "sample_pass": (1, None, AS_GIVEN, ALL_OK),
    "u8_exact": (1, None, AS_GIVEN, ALL_OK),
    "latency_mode": (1, None, AS_GIVEN, ALL_OK),
    "async_search": (0, None, AS_GIVEN, ALL_OK),
    "tail_chunks": (1, "EXPANN_TAIL_CHUNKS", AS_GIVEN, ALL_OK),
    "persist": (1, "EXPANN_PERSIST", AS_GIVEN, ALL_OK),
    "redo_bound": (1, "EXPANN_REDO_BOUND", AS_GIVEN, ALL_OK),
    "select_overlap": (1, "EXPANN_SELECT_OVERLAP", AS_GIVEN, ALL_OK),
    "i8_filter": (1, "EXPANN_I8_FILTER", CLAMP_0_2, ALL_OK),
    "i8_sample": (1, "EXPANN_I8_SAMPLE", CLAMP_0_2, ALL_OK),
    "spec_rank": (0, "EXPANN_SPEC_RANK", AT_LEAST_0, ALL_OK),
    "rerank_rounds": (2, "EXPANN_RERANK_ROUNDS", ONE_OR_TWO, ALL_OK),
    "rerank_stats": (0, None, FLAG, ALL_OK),
    "xcd_tolerance": (3, None, AT_LEAST_0, ALL_OK),
    "sample_run": (1, None, CLAMP_1_64, ALL_OK),
    "sample_frac": (0, None, AT_LEAST_0, ALL_OK),
    "sample_ratio": (32, None, AT_LEAST_2, ALL_OK),
    # outside [0, 16384]: refused, the value stays at its default
    "group_list_rows": (0, None, [0, 0, 0, 1, 2, 3, 64, 65, 16384, 0, 0],
                        [INVALID_ARG, INVALID_ARG, OK, OK, OK, OK, OK, OK, OK, INVALID_ARG, INVALID_ARG]),
    # the removed A/B switches store nothing: 0 is refused, anything else is accepted
    "f16x": (None, None, [None] * 11, [OK, OK, UNSUPPORTED, OK, OK, OK, OK, OK, OK, OK, OK]),
    "i8x": (None, None, [None] * 11, [OK, OK, UNSUPPORTED, OK, OK, OK, OK, OK, OK, OK, OK]),
    "i8w": (None, None, [None] * 11, [OK, OK, UNSUPPORTED, OK, OK, OK, OK, OK, OK, OK, OK]),
}
GROUP_LIST_ROWS_TEXT = "group_list_rows: 0 (auto) or 1..16384"
REMOVED_TEXT = " = 0: the 32 x 32 MFMA forms of rounds 1-2 were removed in round 3"

# what each environment variable leaves in its option when it reads -3, 1 and 7: what a set of that value gives
ENV_EXPECT = {
    "EXPANN_TAIL_CHUNKS": ("tail_chunks", [-3, 1, 7]),
    "EXPANN_PERSIST": ("persist", [-3, 1, 7]),
    "EXPANN_REDO_BOUND": ("redo_bound", [-3, 1, 7]),
    "EXPANN_SELECT_OVERLAP": ("select_overlap", [-3, 1, 7]),
    "EXPANN_I8_FILTER": ("i8_filter", [0, 1, 2]),
    "EXPANN_I8_SAMPLE": ("i8_sample", [0, 1, 2]),
    "EXPANN_SPEC_RANK": ("spec_rank", [0, 1, 7]),
    "EXPANN_RERANK_ROUNDS": ("rerank_rounds", [2, 1, 2]),
}


def _num(text):
    return None if text == "-" else int(text)


@pytest.fixture(scope="module")
def hook(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bf_options") / "bf_options_hook"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "expann_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "bf_options_hook.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:  # (no static sanitizer runtimes here)
        subprocess.check_call(cmd)

    def run(*args, env=None):
        clean = {k: v for k, v in os.environ.items() if not k.startswith("EXPANN_")}
        clean.update(env or {})
        r = subprocess.run([str(exe)] + [str(a) for a in args], env=clean, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return [line.split("\t") for line in r.stdout.splitlines()]
    return run


def test_every_row_has_the_documented_default_environment_name_and_rule(hook):
    rows, sets = {}, {}
    for f in hook("table"):
        if f[0] == "row":
            assert f[1] not in rows, f"{f[1]} has two rows"
            rows[f[1]] = (_num(f[2]), None if f[3] == "-" else f[3])
        else:
            assert f[0] == "set"
            sets.setdefault(f[1], []).append((int(f[2]), _num(f[3]), int(f[4]), f[5]))
    assert sorted(rows) == sorted(EXPECT)
    for name, (default, env, stored, codes) in EXPECT.items():
        assert rows[name] == (default, env), name
        got = sets[name]
        assert [g[0] for g in got] == PROBES, name
        assert [g[1] for g in got] == stored, name
        assert [g[2] for g in got] == codes, name
        for v, _, rc, text in got:
            if rc == OK:
                assert text == "-", (name, v)
            elif name == "group_list_rows":
                assert text == GROUP_LIST_ROWS_TEXT
            else:
                assert text == name + REMOVED_TEXT


@pytest.mark.parametrize("name", ["", "Query_tile", "query_tile ", "opt_query_tile", "EXPANN_PERSIST", "efs", "no_such_option"])
def test_an_unknown_name_is_refused_and_changes_nothing(hook, name):
    assert hook("set", name, 1) == [[str(INVALID_ARG), "unknown option " + name, "unchanged"]]


def test_the_environment_goes_through_the_rule_of_a_set(hook):
    defaults = {name: e[0] for name, e in EXPECT.items()}
    assert {f[1]: _num(f[2]) for f in hook("env")} == defaults  # (nothing set: the defaults)
    assert sorted(ENV_EXPECT) == sorted(e[1] for e in EXPECT.values() if e[1])
    for var, (name, want) in ENV_EXPECT.items():
        assert EXPECT[name][1] == var
        for text, w in zip(["-3", "1", "7"], want):
            got = {f[1]: _num(f[2]) for f in hook("env", env={var: text})}
            assert got == dict(defaults, **{name: w}), (var, text)
    # several at once, and text that atol reads as a number followed by something else
    got = {f[1]: _num(f[2]) for f in hook("env", env={"EXPANN_I8_FILTER": "9", "EXPANN_SPEC_RANK": "12abc", "EXPANN_PERSIST": "0"})}
    assert got == dict(defaults, i8_filter=2, spec_rank=12, persist=0)


def test_the_header_names_every_option_and_every_environment_variable():
    text = open(os.path.join(ROOT, "include", "expann_hip.h")).read()
    decl = text.index("int expann_set_option(expann_index* h")
    comment = text[text.rindex("/*", 0, decl):decl]
    assert comment.lstrip("/* ").startswith("integer options")
    for name, (_, env, _, _) in EXPECT.items():
        assert re.search(r'"%s"' % re.escape(name), comment), f'"{name}" is not in the option comment of expann_hip.h'
        if env:
            assert re.search(r"\b%s\b" % env, comment), f"{env} is not in the option comment of expann_hip.h"
