"""The scan kernels whose fp16 and int8 forms are one template (scan_gemm_kl.hpp: run-time dim; scan_gemm_w8.hpp:
8 waves per tile) or line-for-line twins (scan_gemm_f16x.hpp / scan_gemm_i8w.hpp) against
tests/golden/scan_twins.json, recorded by tests/scan_twins_helpers.py --record from the build in which every one
of them was a hand-written kernel of its own: the same kernel chosen, the same candidate total out of the filter
(so the same lists, not only the same top-k after the exact re-rank), no retry, the same ids and distance bits.

Shapes (scan_twins_helpers.py): 65 536 rows and 65 536 + 37, 300 queries, k = 10 and 100; the fp16 form of fp32
rows at d = 64 / 128 (4 waves x 64 queries), 256 / 512 (8 waves per tile), 80 / 1040 (run-time dim), L2 and IP;
the int8 form (scan_kernel = 5) of uint8 L2, int8 L2 and int8 IP at d = 128 / 256, 768 / 832 / 960, 192 / 1088.
The sampled pass of every case runs the SAMPLE instance.  The REDO instances run under a forced speculative rank
(spec_rank = 2, the rank of test_gpu_spec_tau.py's redo cases: 204 of the 300 queries take the redo pass in the
recorded build) with the fp16 form and with the int8 filter of fp32 rows (i8_filter = 2), d = 128, L2, k = 10."""
import json

import pytest

import scan_twins_helpers as H

pytestmark = pytest.mark.gpu

CASES = H.cases()


@pytest.fixture(scope="module")
def golden():
    with open(H.GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("cid,spec", CASES, ids=[c for c, _ in CASES])
def test_same_lists_and_results_as_the_separate_kernels(golden, cid, spec):
    want = dict(golden[cid])
    rank = want.pop("rank", None)
    assert (rank is not None) == spec["redo"]
    got = H.run(spec, [int(key[1:]) for key in sorted(want)], rank)
    print(cid, got)
    for key, w in want.items():
        g = got[key]
        assert g["scan_kernel"] == spec["name"] == w["scan_kernel"], (key, g)
        assert g["retries"] == 0, (key, g)
        if spec["redo"]:
            assert g["redo_queries"] > 0, (key, g)
        assert g == w, (key, g, w)
