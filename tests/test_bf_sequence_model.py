"""The conditions that keep tests/test_gpu_bf_sequences.py from passing vacuously, checked without a
GPU over every (config, seed) that file runs: each mutation changes the answers of many queries (SENSITIVITY), each
sequence passes through the sites where a derived copy is dropped, kept, re-pointed or grown (COVERAGE), the generator
is a function of its arguments (DETERMINISM), and the driver fails engines that answer from stale state."""
import numpy as np
import pytest

import bf_sequence_model as bsm

CASES = [(name, seed) for name in sorted(bsm.CONFIGS) for seed in bsm.SEEDS]
IDS = ["%s-%d" % c for c in CASES]

# what every sequence must contain; the second set only where the rows are floats (8-bit rows have no fp16 copy whose
# scale could change, and refuse the filter that a compaction needs), the third only on 8-bit rows
EVERYWHERE = {"cross_up", "cross_down", "tile_inside", "tile_exact", "cap_growth", "within_reserve",
              "refuse_compact_nofilter", "refuse_remove_all", "refuse_remove_id"}
FLOAT_ROWS = {"scale_append", "max_row_removed", "remove_after_filter_used", "compact", "refuse_range_filter",
              "refuse_grouped_filter", "refuse_compact_zero"}
EIGHT_BIT = {"refuse_filter_8bit", "refuse_groups_8bit", "refuse_range_8bit"}


@pytest.mark.parametrize("name,seed", CASES, ids=IDS)
def test_sensitivity(oracle, name, seed):
    """after every accepted mutation of the rows, the filter or the labels, the expected top-10 differs for at least a
    quarter of the 130 queries (the generator aims at a third); simulate() says what is compared with what"""
    sim = bsm.simulate(name, seed)
    judged = [r for r in sim if r["changed"] is not None]
    assert len(judged) >= 8
    for r in judged:
        assert 4 * r["changed"] >= bsm.M, (name, seed, r["i"], r["what"], r["changed"])
    # every mutation is either judged, or one that must change no answer: a reserve, an option, a call that was
    # ITSELF refused (by the status code it returned, not by a refusal one of the checks after it met)
    for r in sim:
        if r["op"] in bsm.MUTATIONS and r["changed"] is None:
            assert r["op"] in ("reserve", "option") or r["status"] != bsm.OK, r
        if r["op"] in bsm.MUTATIONS and r["status"] != bsm.OK:
            assert r["own_tags"] and r["own_tags"][0].startswith("refuse_") and (r["n0"], r["changed"]) == (r["n1"], None), r


@pytest.mark.parametrize("name,seed", CASES, ids=IDS)
def test_coverage(oracle, name, seed):
    sim = bsm.simulate(name, seed)
    cfg = bsm.resolve(name, seed)
    seen = {t for r in sim for t in r["tags"]}
    want = EVERYWHERE | (FLOAT_ROWS if bsm.float_rows(cfg) else EIGHT_BIT)
    assert want <= seen, (name, seed, sorted(want - seen))
    if bsm.float_rows(cfg):   # a REMOVE follows a filter that was set and used (the compaction does so by its nature)
        assert any(r["op"] == "remove" and "remove_after_filter_used" in r["own_tags"] for r in sim)
    else:
        # past 32 768 rows under "scan_kernel" 5: seed 2 keeps whole 64-row tiles through both appends and the reserve
        # (int8 rows: the operand is the base itself), the other seeds stay inside a tile (the operand is a copy)
        at = next(r["i"] for r in sim if r["what"] == "option(scan_kernel=5)")
        grown = [r["n1"] % 64 == 0 for r in sim[at:] if r["op"] == "append"]
        assert len(grown) == 2 and all(g == (seed == 2 and cfg.dtype == "i8") for g in grown), (name, seed, grown)
        assert sim[at + 1]["n1"] >= bsm.I8_MIN_ROWS and "cap_growth" in sim[at + 3]["own_tags"]   # the second reallocates
    # 4 096 rows, where f16_copy_at_build and the direct scan change hands: crossed upward, LATER downward
    up = min(r["i"] for r in sim if "cross_up" in r["tags"])
    assert any("cross_down" in r["tags"] and r["i"] > up for r in sim)
    # the append that stays within a reserve comes after a reserve that grew the capacity
    res = min(r["i"] for r in sim if "reserve_grows" in r["tags"])
    assert any("within_reserve" in r["tags"] and r["i"] > res for r in sim)
    sizes = [r["n1"] for r in sim]
    assert min(sizes) >= 1500 and max(sizes) < bsm.MAX_ROWS[name], (min(sizes), max(sizes))
    ops = bsm.generate(name, seed)
    assert 24 <= len(ops) <= 70
    reads = sum(o["op"] in ("search", "grouped", "range", "score") for o in ops)
    assert reads >= 6 and len(ops) - reads >= 12          # reads and mutations interleave
    if bsm.CONFIGS[name].options:                          # B: every scan form forced, the filter tier forced
        opts = {(o["name"], o["value"]) for o in ops if o["op"] == "option"}
        assert {("scan_kernel", v) for v in (1, 2, 3, 4)} <= opts
        assert {("i8_filter", 2), ("i8_sample", 2), ("sample_pass", 0)} <= opts
        assert any(n == "group_list_rows" and v > 0 for n, v in opts)
    if bsm.CONFIGS[name].async_seed == seed:
        assert any(o.get("deferred") for o in ops if o["op"] == "append")
        assert any(o.get("deferred") for o in ops if o["op"] == "remove")


def test_the_async_seeds_exist():
    assert bsm.CONFIGS["A"].async_seed in bsm.SEEDS and bsm.CONFIGS["E"].async_seed in bsm.SEEDS


def _same_ops(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for key in x:
            if isinstance(x[key], np.ndarray):
                assert x[key].dtype == y[key].dtype and np.array_equal(x[key], y[key]), key
            else:
                assert x[key] == y[key], key


@pytest.mark.parametrize("name", ["A", "F"])
def test_generate_is_deterministic(oracle, name):
    first = bsm.generate(name, 1)
    bsm._generate.cache_clear()
    _same_ops(first, bsm.generate(name, 1))
    assert [bsm.describe(o) for o in bsm.replay(name, 1, 9)] == [bsm.describe(o) for o in first[:10]]
    other = bsm.generate(name, 2)
    assert [bsm.describe(o) for o in other] != [bsm.describe(o) for o in first]


def _drive(oracle, fake_cls, name, seed):
    cfg = bsm.resolve(name, seed)
    rows, queries = bsm.initial(name, seed)
    return bsm.run(fake_cls(oracle, cfg, rows), bsm.Model(oracle, cfg, rows), bsm.generate(name, seed), oracle,
                   queries=queries, config=name, seed=seed)


@pytest.mark.parametrize("name,seed", CASES, ids=IDS)
def test_the_driver_passes_a_faithful_engine(oracle, name, seed):
    drv = _drive(oracle, bsm.FakeEngine, name, seed)
    assert len(drv.log) == len(bsm.generate(name, seed))


@pytest.mark.parametrize("fake", bsm.STALE_FAKES, ids=lambda f: f.__name__)
def test_the_driver_fails_a_stale_engine(oracle, fake):
    """each stale fake fails within the sequence, and the message carries what replays the prefix"""
    with pytest.raises(AssertionError) as e:
        _drive(oracle, fake, "B", 0)
    text = str(e.value)
    assert "config B seed 0 step " in text and "bf_sequence_model.replay('B', 0, " in text
    expected = {"StaleRange": "range search", "StaleFilter": "search(", "StaleScore": "score_ids",
                "StaleOption": "tiers"}[fake.__name__]
    assert expected in text, text


def test_the_model_refuses_mutations_of_adopted_rows(oracle):
    """rows adopted from the caller (owned=False): append, reserve, remove and compaction are EXPANN_ERR_UNSUPPORTED
    and change nothing; the reads, the filter and the labels work as on rows of the handle's own"""
    cfg = bsm.resolve("A", 0)
    rows, queries = bsm.initial("A", 0)
    model = bsm.Model(oracle, cfg, rows[:500], owned=False)
    want = model.expect_search(queries, 10)
    assert model.set_row_filter(np.arange(500) % 2 == 0) == bsm.OK
    for call in (lambda: model.append(rows[500:510]), lambda: model.reserve(900), lambda: model.remove([1, 2]),
                 model.compact_row_filter):
        assert call() == bsm.UNSUPPORTED
    assert (model.n, model.capacity, model.reallocs) == (500, 500, 0) and model.allow is not None
    assert model.set_row_filter(None) == bsm.OK and model.set_row_groups(np.zeros(500, np.uint32)) == bsm.OK
    got = model.expect_search(queries, 10)
    assert got[0] == want[0] == bsm.OK and all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))
