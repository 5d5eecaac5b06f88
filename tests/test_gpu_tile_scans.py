"""The four packed-row scans that share one tile skeleton (scan_tile.hpp: tile range, threshold load and epilogue
once; scan_hamming.hpp, scan_asym.hpp, scan_i4.hpp, scan_pq4.hpp supply a policy each) against
tests/golden/tile_scans.json, recorded by tests/tile_scans_helpers.py --record from the build in which each kernel
carried its own copy of all three: the same kernel, the same number of levels, the same candidate total out of the
last level's lists (so the same keys filed -- a looser tie rule or a wrong per-query term shows here, where the
select would hide it), the same retries, the same ids and distance bits.

Shapes (tile_scans_helpers.py): 65 536 rows and 65 536 + 37 (a ragged last tile), 100 queries (a full query tile
and one of 36), k = 10 and 100.  Hamming on the matrix cores at dims 64 and 1024; int8 queries on packed bits at
64, 576 and 4096; 4-bit rows under both metrics at 64, 192 and 1536; 4-bit PQ under both metrics at (dim, M) =
(128, 16), (1024, 128) -- the largest resident M -- and (576, 144), streamed tables.  One asym case and one I4 case
carry 4096 copies of 64 rows, so that the tie rule decides which keys are filed."""
import json

import pytest

import tile_scans_helpers as H

pytestmark = pytest.mark.gpu

CASES = H.cases()


@pytest.fixture(scope="module")
def golden():
    with open(H.GOLDEN) as f:
        return json.load(f)


def test_the_golden_covers_every_case(golden):
    assert sorted(golden) == sorted(c for c, _ in CASES)


@pytest.mark.parametrize("cid,spec", CASES, ids=[c for c, _ in CASES])
def test_same_lists_and_results_as_the_separate_kernels(golden, cid, spec):
    want = golden[cid]
    assert sorted(want) == [f"k{k}" for k in H.KS]
    got = H.run(spec, H.KS)
    print(cid, got)
    for key, w in want.items():
        g = got[key]
        assert g["scan_kernel"] == spec["name"] == w["scan_kernel"], (key, g)
        assert w["levels"] >= 2 and w["candidates"] > 0, (key, w)
        assert g == w, (key, g, w)
