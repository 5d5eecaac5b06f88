"""The brute-force planner (expann_amd/csrc/bf_plan.hpp), without a device.

tests/native/bf_plan_hook.cpp, a stand-alone program that includes nothing but that header, prints the plan for the
cases it reads.  The expectations below are written out from the measured crossovers DESIGN.md documents -- both
sides of each -- not read from the code under test.  The program is built with the address and undefined-behaviour
sanitizers where g++ has their static runtimes, else without."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED = 0, 5
F32, U8, I8, I16, F16 = 0, 1, 2, 3, 4          # EXPANN_DTYPE_*
L2, IP = 0, 1                                  # EXPANN_METRIC_*
U8L2, I8L2, I8L2REF, I8IP, I16L2REF = 0, 1, 2, 3, 4  # int_mode
M = 1_000_000

REFUSE_GEMM = ("GEMM-form scan (scan_kernel=2): 8-bit L2/IP with dim 128/256/768 (the fp32-input MFMA form of "
               "rounds 1-2 is gone: scan_kernel 3 = bf16x3, 4 = fp16)")
REFUSE_BF16 = "bf16x3 GEMM-form scan: f32 L2 with dim 64 or 128 only"
REFUSE_F16 = "fp16 GEMM-form scan: f32 with dim a multiple of 16 from 64 to 4096 only"

FIELDS = ["status", "family", "i8q", "u8_shadow", "direct_tq", "direct_f16_tq", "i8f", "i8f_min_cap", "speculate", "sampled",
          "tie_fallback", "message"]


def f32(**kw):
    """fp32 L2 rows, d = 128, 1 M rows; the hook's call is m = 1000, k = 10, cap = 2048"""
    return dict(dict(dtype=F32, int_mode=-1, metric=L2, dim=128, n=M), **kw)


def f16(**kw):
    return f32(dtype=F16, **kw)


def u8(**kw):
    return dict(dict(dtype=U8, int_mode=U8L2, metric=L2, dim=128, n=M), **kw)


def i8ip(**kw):
    return dict(dict(dtype=I8, int_mode=I8IP, metric=IP, dim=128, n=M), **kw)


CASES = []


def expect(inputs, **want):
    CASES.append((inputs, want))


# ---- float rows: few queries.  From 5 queries on the fp16 form wins; below, only where scan_direct_f16 has a tile
# that takes the batch in one pass (d 64 / 128 / 256: 4 queries, 512: 2, 768 / 832 / 960: 1, other dims: none)
expect(f32(m=1), family="f16x", direct_f16_tq=2, direct_tq=1)
expect(f32(m=3), family="f16x", direct_f16_tq=4, direct_tq=4)
expect(f32(m=4), family="f16x", direct_f16_tq=4, tie_fallback=1, sampled=1)
expect(f32(m=5), family="f16x", direct_f16_tq=0, direct_tq=8)
expect(f32(m=17), family="f16x", direct_tq=16)
expect(f32(dim=144, m=4), family="direct", direct_f16_tq=0, tie_fallback=0, sampled=1)
expect(f32(dim=144, m=5), family="f16kl", direct_f16_tq=0)
expect(f32(dim=512, m=2), family="f16y", direct_f16_tq=2)
expect(f32(dim=512, m=3), family="direct")
expect(f32(dim=512, m=4), family="direct")
expect(f32(dim=512, m=5), family="f16y", direct_f16_tq=0)
expect(f32(dim=768, m=1), family="f16kx", direct_f16_tq=1)
expect(f32(dim=768, m=2), family="direct")
expect(f32(dim=768, m=4), family="direct")
expect(f32(dim=768, m=5), family="f16kx")
expect(f32(metric=IP, m=4), family="f16x", direct_f16_tq=4)
expect(f32(metric=IP, dim=144, m=4), family="direct")
expect(f32(metric=IP, dim=144, m=5), family="f16kl")
expect(f16(m=4), family="f16x", direct_f16_tq=4)
expect(f16(dim=144, m=4), family="direct")
expect(f16(dim=144, m=5), family="f16kl")
# ... without the fp16 form only bf16x3 is left (fp32 L2, d = 64 / 128), which pays from 24 queries on
expect(f32(no_f16=1, m=23), family="direct")
expect(f32(no_f16=1, m=24), family="bf16x3", sampled=0, tie_fallback=1)
expect(f32(dim=64, no_f16=1, m=24), family="bf16x3")
expect(f32(dim=256, no_f16=1, m=24), family="direct")
expect(f32(f16_ok=0, no_f16=1, m=23), family="direct")
expect(f32(f16_ok=0, no_f16=1, m=24), family="bf16x3")
expect(f32(f16_ok=0, m=23), family="direct")        # (rows outside the fp16 range: the 24-query rule from the start;
expect(f32(f16_ok=0, m=24), family="f16x")          # the attempt then learns no_f16 from the copy it cannot build)
# (the inner product has no bf16x3 form: without the fp16 form, the direct scan at any batch size)
expect(f32(metric=IP, no_f16=1, m=23), family="direct")
expect(f32(metric=IP, no_f16=1, m=24), family="direct", tie_fallback=0)
expect(f32(metric=IP, dim=64, no_f16=1), family="direct")
expect(f32(metric=IP, dim=256, no_f16=1, m=24), family="direct")
expect(f32(metric=IP, scan_kernel=4, no_f16=1), family="direct", status=OK)
expect(f32(metric=IP, f16_ok=0), family="direct")
expect(f16(no_f16=1), family="direct")
expect(f32(dim=48), family="direct", direct_tq=4)
# ---- 8-bit rows: the matrix cores from 96 queries on
expect(u8(m=95), family="direct", i8q="-", direct_tq=16)
expect(u8(m=96), family="gemm_i8", i8q="i8q_w", tie_fallback=1, sampled=0)
expect(u8(dim=192, m=95), family="direct", i8q="-", direct_tq=8)
expect(u8(dim=192, m=96), family="direct", i8q="i8q_kl")
expect(i8ip(m=95), family="direct", i8q="-")
expect(i8ip(m=96), family="gemm_i8", i8q="i8q_w")
# ---- rows: 4 096 for any matrix-core form, 32 768 for the int8 hit-log forms, 65 536 for the q-forms and the shadow on auto
expect(f32(n=4095), family="direct", tie_fallback=0)
expect(f32(n=4096), family="f16x")
expect(f32(metric=IP, n=4095), family="direct")
expect(f32(metric=IP, n=4096), family="f16x")
expect(f32(n=4095, scan_kernel=4), family="f16x")
expect(u8(m=96, n=4095), family="direct", i8q="-")
expect(u8(m=96, n=4096), family="gemm_i8", i8q="-")
expect(u8(m=96, n=65535), family="gemm_i8", i8q="-")
expect(u8(m=96, n=65536), family="gemm_i8", i8q="i8q_w")
expect(u8(scan_kernel=5, n=32767), family="gemm_i8", i8q="-")
expect(u8(scan_kernel=5, n=32768, m=1), family="gemm_i8", i8q="i8q_w")
expect(f32(i8_filter=2, n=32767), i8f=0)
expect(f32(i8_filter=2, n=32768), i8f=1, family="f16x", i8f_min_cap=4096)
expect(f32(m=96, n=65535), u8_shadow=0)
expect(f32(m=96, n=65536), u8_shadow=1, family="f16x")
expect(f32(m=95, n=65536), u8_shadow=0)
expect(f32(m=96, dim=256), u8_shadow=1)
expect(f32(m=96, dim=64), u8_shadow=0)
expect(f32(m=96, metric=IP), u8_shadow=0)
expect(f16(m=96), u8_shadow=0)
expect(f32(m=96, u8_exact_opt=0), u8_shadow=0)
expect(f32(m=96, u8_exact=-1), u8_shadow=0)
expect(f32(m=96, u8_exact=1), u8_shadow=1, i8f=0)
expect(f32(m=96, scan_kernel=4), u8_shadow=0)
expect(f32(m=96, filter_on=1, n_allowed=M), u8_shadow=0)
# ---- k: 256 is the most the int8 hit-log forms and the shadow take
expect(u8(m=96, k=256), i8q="i8q_w")
expect(u8(m=96, k=257), i8q="-", family="gemm_i8")
expect(f32(i8_filter=2, k=256), i8f=1)
expect(f32(i8_filter=2, k=257), i8f=0)
expect(f32(m=96, k=256), u8_shadow=1)
expect(f32(m=96, k=257), u8_shadow=0)
# ---- the int8 filter's auto region ("i8_filter" 1): every corner of the measured grid
for n, m, k, inside in [(499_999, 2048, 1, 0), (500_000, 2047, 1, 0), (500_000, 2048, 1, 1),
                        (M, 4096, 10, 1), (M - 1, 4096, 10, 0), (M, 4095, 10, 0), (2 * M, 2048, 10, 1),
                        (2 * M - 1, 2048, 10, 0), (2 * M, 2047, 10, 0), (500_000, 10000, 10, 0), (M, 4096, 2, 1),
                        (2 * M, 2048, 16, 1), (2 * M, 2047, 16, 0), (2 * M - 1, 2048, 16, 0), (M, 10000, 16, 1),
                        (M, 9999, 16, 0), (M - 1, 10000, 16, 0), (M, 4096, 11, 0), (M, 10000, 11, 1),
                        (2 * M, 10000, 17, 0), (4 * M, 100_000, 17, 0)]:
    expect(f32(n=n, m=m, k=k), i8f=inside, family="f16x")
expect(f32(m=4096, i8f_state=2), i8f=0)
expect(f32(m=4096, i8f_state=2, i8_filter=2), i8f=1)
expect(f32(m=4096, i8f_state=-1, i8_filter=2), i8f=0)
expect(f32(m=4096, i8_filter=0), i8f=0)
expect(f32(m=4096, debug=2), i8f=0, family="f16dbg")
expect(f32(m=4096, debug=16), i8f=1, family="f16x")
expect(f32(m=4096, cand_capacity=512), i8f=1, i8f_min_cap=0)
expect(f32(m=4096, metric=IP, i8_filter=2), i8f=0)
expect(f32(m=4096, dim=64, i8_filter=2), i8f=0)
expect(f16(m=4096, i8_filter=2), i8f=0)
expect(f32(m=4096, scan_kernel=4, i8_filter=2), i8f=0)
# ---- speculative thresholds on auto ("spec_rank" 0): 4 096 queries on the int8 filter, or at k > 32
expect(f32(m=4096), i8f=1, speculate=1)
expect(f32(m=4095), i8f=0, speculate=0)
expect(f32(m=4095, i8_filter=2), i8f=1, speculate=0)
expect(f32(m=4096, i8_filter=2), i8f=1, speculate=1)
expect(f32(m=4096, i8_filter=0, k=32), speculate=0)
expect(f32(m=4096, i8_filter=0, k=33), speculate=1)
expect(f32(m=4095, i8_filter=0, k=33), speculate=0)
expect(f32(m=4096, dim=64, k=33), speculate=1, family="f16x")
expect(f32(m=4096, dim=256, k=33), speculate=0, family="f16y")
expect(f32(m=4096, dim=144, k=33), speculate=0, family="f16kl")
# ... and with a rank set: batches beyond the latency mode's 64, the f16x stream, no debug value, no row filter
expect(f32(m=64, spec_rank=4, i8_filter=0), speculate=0)
expect(f32(m=65, spec_rank=4, i8_filter=0), speculate=1)
expect(f32(m=65, spec_rank=4, i8_filter=0, spec_off=1), speculate=0)
expect(f32(m=65, spec_rank=4, dim=64, debug=2), speculate=0, family="f16x")
expect(f32(m=65, spec_rank=4, dim=256), speculate=0)
expect(f32(m=65, spec_rank=4, filter_on=1, n_allowed=M), speculate=0, family="f16x")
# ---- dims: the geometry of the fp16 form and the direct scan's largest tile (m = 1000)
for d, family, tq in [(48, "direct", 4), (64, "f16x", 16), (128, "f16x", 16), (144, "f16kl", 4), (256, "f16y", 8),
                      (512, "f16y", 4), (768, "f16kx", 2), (832, "f16kx", 2), (960, "f16kx", 2), (1024, "f16kl", 2),
                      (4096, "f16kl", 4), (4112, "direct", 0)]:
    expect(f32(dim=d, i8_filter=0), family=family, direct_tq=tq, status=OK)
    expect(f32(dim=d, metric=IP), family=family, direct_tq=tq)
    expect(f16(dim=d), family=family, direct_tq=4 if tq else 0)
for d, family, q, tq in [(64, "direct", "-", 16), (128, "gemm_i8", "i8q_w", 16), (256, "gemm_i8", "i8q_w", 8),
                         (512, "direct", "i8q_kl", 8), (768, "gemm_i8", "i8q_x", 8), (832, "direct", "i8q_x", 4),
                         (896, "direct", "i8q_x", 8), (960, "direct", "i8q_x", 4), (1024, "direct", "i8q_kl", 8),
                         (4096, "direct", "i8q_kl", 8), (4160, "direct", "-", 0)]:
    expect(u8(dim=d), family=family, i8q=q, direct_tq=tq)
    expect(i8ip(dim=d), family=family, i8q=q, direct_tq=tq)
expect(u8(dtype=I8, int_mode=I8L2REF, dim=128), family="direct", i8q="-", direct_tq=16)
expect(u8(dtype=I8, int_mode=I8L2REF, dim=192), family="direct", i8q="-", direct_tq=8)
expect(u8(dtype=I16, int_mode=I16L2REF, dim=64), family="direct", i8q="-", direct_tq=16)
expect(u8(dtype=I16, int_mode=I16L2REF, dim=128), family="direct", i8q="-", direct_tq=8)
expect(u8(dtype=I16, int_mode=I16L2REF, dim=256), family="direct", i8q="-", direct_tq=0)
# the direct scan's tile: the forced one or none; else the smallest that covers m, else the largest
expect(f32(query_tile=8), direct_tq=8)
expect(f32(query_tile=3), direct_tq=0)
expect(f32(dim=64, m=2), direct_tq=4)
expect(u8(m=5), direct_tq=16)
expect(u8(query_tile=4), direct_tq=4)
# ---- "scan_kernel" 0 .. 6
for sk, family in enumerate(["f16x", "direct", None, "bf16x3", "f16x", "bf16x3", "f16x"]):
    if family:
        expect(f32(scan_kernel=sk, i8_filter=2), family=family, status=OK, message="-", tie_fallback=int(sk == 0), i8f=int(sk == 0),
               direct_f16_tq=0)
        expect(f32(scan_kernel=sk, m=4), direct_f16_tq=4 if sk == 0 else 0)
for sk, family in enumerate(["f16x", "direct", None, None, "f16x", "direct", "f16x"]):
    if family:
        expect(f32(scan_kernel=sk, metric=IP), family=family, status=OK, message="-")
for sk, family in enumerate(["f16x", "direct", None, "direct", "f16x", "direct", "f16x"]):
    if family:
        expect(f16(scan_kernel=sk), family=family, status=OK)
        expect(f16(scan_kernel=sk, metric=IP), family=family, status=OK)
for rows in (u8, i8ip):
    expect(rows(scan_kernel=0), family="gemm_i8", i8q="i8q_w", status=OK)
    expect(rows(scan_kernel=1), family="direct", i8q="-", status=OK)
    expect(rows(scan_kernel=2), family="gemm_i8", i8q="-", status=OK)
    expect(rows(scan_kernel=5), family="gemm_i8", i8q="i8q_w", status=OK, tie_fallback=0)
    expect(rows(scan_kernel=2, dim=192), status=UNSUPPORTED, message=REFUSE_GEMM)
    expect(rows(scan_kernel=3), status=UNSUPPORTED, message=REFUSE_BF16)
    expect(rows(scan_kernel=4), status=UNSUPPORTED, message=REFUSE_F16)
    expect(rows(scan_kernel=6), status=UNSUPPORTED, message=REFUSE_F16)
# ---- the three refusals
for rows in (f32, f16):
    expect(rows(scan_kernel=2), status=UNSUPPORTED, message=REFUSE_GEMM)
    expect(rows(scan_kernel=2, metric=IP), status=UNSUPPORTED, message=REFUSE_GEMM)
    expect(rows(scan_kernel=4, dim=48), status=UNSUPPORTED, message=REFUSE_F16)
    expect(rows(scan_kernel=6, dim=48), status=UNSUPPORTED, message=REFUSE_F16)
    expect(rows(scan_kernel=4, dim=48, no_f16=1), status=OK, family="direct")
expect(f32(scan_kernel=3, dim=256), status=UNSUPPORTED, message=REFUSE_BF16)
expect(f32(scan_kernel=3, metric=IP), status=UNSUPPORTED, message=REFUSE_BF16)
expect(f32(scan_kernel=3, force_direct=1), status=UNSUPPORTED, message=REFUSE_BF16)
expect(f32(scan_kernel=3, filter_on=1, n_allowed=M), status=OK, family="direct")
expect(f32(scan_kernel=4, no_f16=1), status=OK, family="bf16x3")
expect(f32(scan_kernel=4, dim=256, no_f16=1), status=OK, family="direct")
# ---- the debug instance: d = 128 only; bit 4 only prints clocks
expect(f32(debug=2), family="f16dbg")
expect(f32(debug=18), family="f16dbg")
expect(f32(debug=16), family="f16x")
expect(f32(debug=2, dim=64), family="f16x")
expect(f32(debug=2, dim=256), family="f16y")
# ---- a row filter: the fp16 forms only, and the exact scan of the filter's list when it fits a candidate list
expect(f32(filter_on=1, n_allowed=2048, cap=2048), family="direct", sampled=0)
expect(f32(filter_on=1, n_allowed=2049, cap=2048, i8_filter=2, spec_rank=4), family="f16x", sampled=1, i8f=0, speculate=0)
expect(f32(filter_on=1, n_allowed=8192, cap=8192), family="direct")
expect(f32(filter_on=1, n_allowed=8193, cap=8192), family="f16x")
expect(f32(filter_on=1, n_allowed=M, no_f16=1), family="direct")
expect(f32(filter_on=1, n_allowed=2048, cap=2048, scan_kernel=4), family="direct", status=OK)
expect(f32(filter_on=1, n_allowed=2049, cap=2048, scan_kernel=4, dim=48), status=UNSUPPORTED, message=REFUSE_F16)
expect(f16(filter_on=1, n_allowed=2049, cap=2048), family="f16x")
# ---- what an attempt learned
expect(f32(force_direct=1), family="direct", tie_fallback=0, sampled=1, i8f=0)
expect(u8(force_direct=1), family="direct", i8q="i8q_w")
expect(f32(m=4096, i8f_off=1), i8f=0, speculate=0, family="f16x")
expect(f32(m=4096, i8f_off=1, k=33), i8f=0, speculate=1)
expect(f32(m=4096, spec_off=1), i8f=1, speculate=0)
# ---- the sampled pass
expect(f32(sample_pass=0), family="f16x", sampled=0)
expect(f32(sample_pass=0, scan_kernel=1), family="direct", sampled=0)
expect(f32(scan_kernel=1), family="direct", sampled=1)
expect(f32(scan_kernel=3), family="bf16x3", sampled=0)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bf_plan") / "bf_plan_hook"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "expann_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "bf_plan_hook.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:  # (no static sanitizer runtimes here)
        subprocess.check_call(cmd)
    text = "".join(" ".join(f"{k}={v}" for k, v in inputs.items()) + "\n" for inputs, _ in CASES)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(CASES)
    out = []
    for line in lines:
        f = line.split("\t")
        assert len(f) == len(FIELDS), line
        out.append({name: (v if name in ("family", "i8q", "message") else int(v)) for name, v in zip(FIELDS, f)})
    return out


def test_the_plan_on_both_sides_of_every_documented_boundary(plans):
    wrong = []
    for (inputs, want), got in zip(CASES, plans):
        for name, v in want.items():
            if got[name] != v:
                wrong.append(f"{inputs}: {name} = {got[name]!r}, expected {v!r}")
    assert not wrong, "\n".join(wrong)


def test_a_refusal_names_its_code_and_a_plan_that_stands_has_no_message(plans):
    for (inputs, _), got in zip(CASES, plans):
        if got["status"] == OK:
            assert got["message"] == "-", inputs
        else:
            assert got["status"] == UNSUPPORTED and got["message"] in (REFUSE_GEMM, REFUSE_BF16, REFUSE_F16), inputs


def test_the_planner_is_one_header_that_needs_no_hip():
    text = open(os.path.join(ROOT, "expann_amd", "csrc", "bf_plan.hpp")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)
    assert includes and all("hip/" not in i and not i.endswith(".hpp") for i in includes), includes
    assert "std::string" not in text and "std::vector" not in text  # (no allocation: once per attempt in latency mode)


REMOVED = ["pick_gemm", "pick_gemm_i8", "pick_gemm_i8q", "i8f_wanted", "i8f_auto_region", "spec_auto_region", "f16_choice",
           "GemmVariant", "GemmFn", "kGemmF16Only", "kGemmF16KLOnly", "GemmScanParams", "kGemmTQ", "gemm_filter_eps",
           "pick_scan_f32", "pick_scan_i8", "pick_direct_f16", "no GEMM-form scan kernel"]


def test_the_engine_no_longer_holds_the_absorbed_rules():
    text = open(os.path.join(ROOT, "expann_amd", "csrc", "expann_hip.hip")).read()
    for name in REMOVED:
        assert not re.search(r"\b%s\b" % re.escape(name), text), f"{name} is still in expann_hip.hip"
    terms = open(os.path.join(ROOT, "expann_amd", "csrc", "gemm_terms.hpp")).read()
    for name in ("GemmScanParams", "kGemmTQ", "gemm_filter_eps"):
        assert not re.search(r"\b%s\b" % name, terms), f"{name} is still in gemm_terms.hpp"
    # the crossovers themselves are in the header alone
    for rule in (r"m\s*<\s*(5|24|96)\b", r"n\s*<\s*(4096|65536)\b", r"opt_scan_kernel\s*==\s*[2-6]\b", r"opt_debug\s*&\s*~16L"):
        assert not re.search(rule, text), f"{rule} is still decided in expann_hip.hip"
