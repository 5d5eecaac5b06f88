"""CPU tests of the oracle (oracle/expann_oracle.c): against the reference-generated golden
vectors for the top-k rule (hand-picked cases and random sequences), and
against independent float64 / integer arithmetic for the distance kernels (whose parity is
UNPINNED: src/distance.h cannot be built in this image)."""
import json
import os

import numpy as np
import pytest


def _cases(golden_dir):
    with open(os.path.join(golden_dir, "topk_ref.json")) as f:
        return json.load(f)["cases"]


def _run_oracle_topk(oracle, c):
    t = oracle.TopK(c["k"])
    trace = dict(is_good=[], size_after=[], worst_after=[], worst_val_after=[],
                 at_capacity_after=[])
    for d, v in zip(c["d"], c["v"]):
        trace["is_good"].append(int(t.consider(np.float32(d), v)))
        trace["size_after"].append(t.size())
        trace["worst_after"].append(t.worst() if t.size() else 0)
        trace["worst_val_after"].append(float(t.worst_val()) if t.size() else 0.0)
        trace["at_capacity_after"].append(int(t.at_capacity()))
    if c["discard_goal"] >= 0:
        t.discard_until_size(c["discard_goal"])
    ids, dists = t.to_combined()
    return trace, ids, dists


def test_topk_matches_reference_golden(oracle, golden_dir):
    """oracle_topk_* == reference src/topk_t.h on every golden case, step by step."""
    cases = _cases(golden_dir)
    assert len(cases) >= 10
    for c in cases:
        trace, ids, dists = _run_oracle_topk(oracle, c)
        for key in ("is_good", "size_after", "worst_after", "at_capacity_after"):
            assert trace[key] == c[key], (c["name"], key)
        assert np.array_equal(np.float32(trace["worst_val_after"]),
                              np.float32(c["worst_val_after"])), c["name"]
        assert [int(x) for x in ids] == c["out_ids"], c["name"]
        assert np.array_equal(dists, np.float32(c["out_dists"])), c["name"]


def test_survey_kat(oracle, golden_dir):
    c = [c for c in _cases(golden_dir) if c["name"] == "survey_kat"][0]
    assert list(zip(c["out_dists"], c["out_ids"])) == [(1.0, 6), (3.0, 3), (3.0, 4)]


def test_topk_matches_live_reference_build(oracle, golden_dir):
    """Same check on 40 random consider() sequences, against the answers of the reference
    build (oracle/_ref/libtopk_ref.so) stored by oracle/gen_golden.py in topk_ref_trials.json."""
    with open(os.path.join(golden_dir, "topk_ref_trials.json")) as f:
        trials = json.load(f)["trials"]
    assert len(trials) == 40
    for ref in trials:
        c = dict(k=ref["k"], d=ref["d"], v=ref["v"], discard_goal=-1)
        trace, ids, dists = _run_oracle_topk(oracle, c)
        assert trace["is_good"] == ref["is_good"]
        assert [int(x) for x in ids] == ref["out_ids"]
        assert np.array_equal(dists, np.float32(ref["out_dists"]))


def test_brute_force_selection_rule_is_topk_rule(oracle, golden_dir):
    """brute_force_engine.h:28-46 admission == topk_t rule on unique increasing ids: the
    oracle's brute force over 1-d 'distances' must reproduce the golden scan cases."""
    for c in _cases(golden_dir):
        if not c["name"].startswith("scan_") and c["name"] != "survey_kat":
            continue
        # encode the distance sequence as d-dimensional rows whose L2 to the zero query is
        # exactly the golden distance: row = [sqrt(d_i), 0, ...] only works for squares, so
        # use the selection rule directly through the inner-product metric on 16-d rows:
        # score = -dot(q, row) with q = e0, row = [-d_i, 0...] -> score = d_i exactly.
        d = np.float32(c["d"])
        base = np.zeros((len(d), 16), np.float32)
        base[:, 0] = -d
        q = np.zeros(16, np.float32)
        q[0] = 1.0
        ids, dists = oracle.brute_force(base, q, c["k"], oracle.METRIC_IP_F32)
        n_out = len(c["out_ids"])
        assert [int(x) for x in ids[0, :n_out]] == c["out_ids"], c["name"]
        assert np.array_equal(dists[0, :n_out], np.float32(c["out_dists"])), c["name"]
        assert np.all(ids[0, n_out:] == np.uint64(2 ** 64 - 1))


@pytest.mark.parametrize("d", [16, 64, 128, 256, 960])
def test_l2_and_dot_f32_against_float64(oracle, d):
    rng = np.random.RandomState(d)
    for _ in range(50):
        a = rng.standard_normal(d).astype(np.float32)
        b = rng.standard_normal(d).astype(np.float32)
        ref = np.sum((a.astype(np.float64) - b.astype(np.float64)) ** 2)
        assert abs(oracle.l2_f32(a, b) - ref) <= 1e-5 * ref
        refd = np.dot(a.astype(np.float64), b.astype(np.float64))
        assert abs(oracle.dot_f32(a, b) - refd) <= 1e-5 * np.sum(np.abs(a * b))


def test_l2_f32_lane_order_is_the_documented_one(oracle):
    """Independent numpy restatement of the 16-lane FMA order + reduce tree (float32 ops,
    fma emulated in float64 which is exact for one product-sum of float32 values)."""
    rng = np.random.RandomState(3)
    for d in (16, 128, 256):
        for _ in range(20):
            a = (rng.standard_normal(d) * 10 ** rng.uniform(-3, 3)).astype(np.float32)
            b = (rng.standard_normal(d) * 10 ** rng.uniform(-3, 3)).astype(np.float32)
            acc = np.zeros(16, np.float32)
            for i in range(0, d, 16):
                diff = (a[i:i + 16] - b[i:i + 16]).astype(np.float32)
                # fma: exact product+sum in float64 (24+24 bit product fits 53 bits; the sum
                # with a float32 addend can lose bits only below float32 rounding precision
                # in rare double-rounding cases, which the comparison below tolerates as
                # <= 1 ulp and the C oracle is authoritative)
                acc = (diff.astype(np.float64) * diff.astype(np.float64)
                       + acc.astype(np.float64)).astype(np.float32)
            t8 = (acc[8:] + acc[:8]).astype(np.float32)
            t4 = (t8[4:] + t8[:4]).astype(np.float32)
            t2 = (t4[:2] + t4[2:]).astype(np.float32)
            want = np.float32(t2[0] + t2[1])
            got = oracle.l2_f32(a, b)
            assert abs(float(got) - float(want)) <= 2 * np.spacing(np.float32(want))


def test_int_kernels(oracle):
    rng = np.random.RandomState(11)
    for d in (64, 128, 768):
        a = rng.randint(-128, 128, size=d).astype(np.int8)
        b = rng.randint(-128, 128, size=d).astype(np.int8)
        ai, bi = a.astype(np.int64), b.astype(np.int64)
        assert oracle.int_kernel("oracle_l2_i8", a, b) == int(np.sum((ai - bi) ** 2))
        wrapped = ((ai - bi) & 0xFF) ** 2
        assert oracle.int_kernel("oracle_l2_i8_refcompat", a, b) == int(np.sum(wrapped))
        assert oracle.int_kernel("oracle_ip_i8", a, b) == int(np.sum(ai * bi))
    # the survey's observation: on [0,127] data the reference kernel differs from true L2
    a = rng.randint(0, 128, size=64).astype(np.int8)
    b = rng.randint(0, 128, size=64).astype(np.int8)
    assert oracle.int_kernel("oracle_l2_i8_refcompat", a, b) > oracle.int_kernel("oracle_l2_i8", a, b)
    # refcompat == true when a >= b everywhere
    hi = np.maximum(a, b)
    lo = np.minimum(a, b)
    assert oracle.int_kernel("oracle_l2_i8_refcompat", hi, lo) == oracle.int_kernel("oracle_l2_i8", hi, lo)
    # int16: exact while |diff| <= 181, wraps beyond (distance.h:14-27)
    a16 = rng.randint(0, 128, size=64).astype(np.int16)
    b16 = rng.randint(0, 128, size=64).astype(np.int16)
    assert oracle.int_kernel("oracle_l2_i16_refcompat", a16, b16) == int(
        np.sum((a16.astype(np.int64) - b16.astype(np.int64)) ** 2))
    a16[:] = 300
    b16[:] = 0  # 300^2 = 90000 -> low 16 bits 24464 -> positive
    assert oracle.int_kernel("oracle_l2_i16_refcompat", a16, b16) == 64 * (90000 & 0xFFFF)
    a16[:] = 200  # 40000 -> 0x9C40 -> negative as int16
    assert oracle.int_kernel("oracle_l2_i16_refcompat", a16, b16) == 64 * (40000 - 65536)


def test_int16_metric_in_brute_force(oracle):
    """the int16 kernel (a-5b) is reachable through brute force / filter_by_score like the others"""
    rng = np.random.RandomState(16)
    base = rng.randint(-300, 300, size=(500, 64)).astype(np.int16)
    q = rng.randint(-300, 300, size=(3, 64)).astype(np.int16)
    ids, d = oracle.brute_force(base, q, 5, oracle.METRIC_L2_I16_REFCOMPAT)
    for qi in range(3):
        sc = np.array([oracle.int_kernel("oracle_l2_i16_refcompat", q[qi], base[r]) for r in range(500)])
        order = np.lexsort((np.arange(500), sc.astype(np.float32)))[:5]
        assert np.array_equal(ids[qi], order.astype(np.uint64))
        assert np.array_equal(d[qi], sc[order].astype(np.float32))


def test_u8_compressed(oracle):
    rng = np.random.RandomState(5)
    for d in (64, 128):
        q = np.clip(np.round(np.abs(rng.standard_normal(d)) * 40), 0, 255).astype(np.float32)
        q += rng.uniform(0, 0.99, size=d).astype(np.float32)  # truncation, not rounding
        row = rng.randint(0, 256, size=d).astype(np.uint8)
        want = int(np.sum((np.floor(q).astype(np.int64) - row.astype(np.int64)) ** 2))
        assert oracle.int_kernel("oracle_l2_u8_compressed", q, row) == want
        assert want < 2 ** 24  # exact as float


def test_brute_force_edge_cases(oracle):
    rng = np.random.RandomState(2)
    base = rng.standard_normal((37, 64)).astype(np.float32)
    q = rng.standard_normal((3, 64)).astype(np.float32)
    # k > n: result length n, padded
    ids, dists = oracle.brute_force(base, q, 50)
    assert np.all(ids[:, 37:] == np.uint64(2 ** 64 - 1)) and np.all(np.isinf(dists[:, 37:]))
    assert sorted(int(x) for x in ids[0, :37]) == list(range(37))
    # duplicated rows: ties broken by lower index
    base2 = np.concatenate([base, base], 0)
    ids2, d2 = oracle.brute_force(base2, q, 10)
    for r in range(3):
        assert np.all(np.diff(d2[r]) >= 0)
        for i in range(0, 10, 2):
            assert ids2[r, i] + 37 == ids2[r, i + 1] and d2[r, i] == d2[r, i + 1]
    # threads give the same answer as serial
    ids_t, d_t = oracle.brute_force(base2, q, 10, n_threads=3)
    assert np.array_equal(ids_t, ids2) and np.array_equal(d_t, d2)
    # recall helper
    assert oracle.recall(ids2, ids2) == 1.0


def test_filter_by_score(oracle):
    rng = np.random.RandomState(9)
    base = rng.standard_normal((100, 64)).astype(np.float32)
    q = rng.standard_normal(64).astype(np.float32)
    ids = rng.permutation(100)[:40].astype(np.uint64)
    d_all = np.array([oracle.l2_f32(q, base[i]) for i in ids], np.float32)
    cutoff = float(np.median(d_all))
    kept, kd = oracle.filter_by_score(base, q, ids, cutoff)
    mask = d_all < np.float32(cutoff)
    assert np.array_equal(kept, ids[mask]) and np.array_equal(kd, d_all[mask])


def test_quantizers(oracle):
    import ctypes as C
    rng = np.random.RandomState(4)
    x = np.clip(np.abs(rng.standard_normal((20, 64))) * 40, 0, 255.9).astype(np.float32)
    out = np.empty(x.size, np.uint8)
    oracle.lib().oracle_quantize_simple_u8(x.ctypes.data, x.size, out.ctypes.data)
    assert np.array_equal(out, np.floor(x).astype(np.uint8).ravel())
    y = rng.standard_normal((20, 64)).astype(np.float32)
    q8 = np.empty(y.size, np.int8)
    sf, off = C.c_float(), C.c_float()
    oracle.lib().oracle_quantize_ranged_q8(y.ctypes.data, 20, 64, q8.ctypes.data, C.byref(sf),
                                           C.byref(off))
    scale = np.float32(128) / (y.max() - y.min())
    assert np.isclose(sf.value, scale)
    assert q8.min() >= 0 and q8.max() <= 127
