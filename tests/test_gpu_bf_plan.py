"""The brute-force planner against the build before it moved to csrc/bf_plan.hpp: tests/golden/bf_plan_parent.json is
profiles/bf_plan_record.py's output on that build -- per case the inputs, the return code and message, the scan kernel,
query tile, levels and retries of the profile, and the statistics that tell which path ran.  Each case is replayed on a
fresh index and must observe the same, field by field; a search that succeeds must also return the oracle's ids and
distance bits (every case is small enough for the CPU oracle)."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bf_plan_record as rec  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "bf_plan_parent.json")) as _f:
    RECORDED = json.load(_f)


def test_the_recorded_cases_are_the_cases_of_the_recorder():
    assert [{k: v for k, v in r.items() if k != "observed"} for r in RECORDED] == json.loads(json.dumps(rec.cases()))


@pytest.mark.parametrize("recorded", RECORDED, ids=[r["name"] for r in RECORDED])
def test_the_search_runs_what_the_parent_ran(recorded, oracle):
    c = {k: v for k, v in recorded.items() if k != "observed"}
    obs, ids, dists, counts = rec.run(c)
    for field, want in recorded["observed"].items():
        assert obs[field] == want, (field, obs)
    assert set(obs) == set(recorded["observed"])
    if obs["rc"] != 0:
        return
    rids, rd, rcounts = rec.oracle(c)
    assert np.array_equal(ids, rids)
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32))
    if rcounts is not None:
        assert np.array_equal(counts, rcounts)


def test_inner_product_queries_outside_the_fp16_range_restart_on_the_direct_scan(oracle):
    """fp32 inner-product rows at d = 128, 32 queries of which one leaves the fp16 range: the fp16 form's attempt is
    given up and, the inner product having no bf16x3 form, the exact direct scan answers.  (Not in the golden file:
    the build before bf_plan.hpp planned bf16x3 here through a placeholder variant without row-term kernels and
    ended the process in the launch of a null kernel.)"""
    c = rec.case("far-f32-ip-d128", metric="ip", n=8192, m=32, queries="far")
    obs, ids, dists, _ = rec.run(c)
    assert obs["rc"] == 0 and obs["retries"] == 1 and obs["scan_kernel"] == "scan_filter_f32<128,16,IP>", obs
    rids, rd, _ = rec.oracle(c)
    assert np.array_equal(ids, rids)
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32))
