"""The auto rank of the speculative thresholds, host arithmetic only: expann_spec_rank_auto(k, frac)
is the smallest j < k whose binomial tail P(Bin(k - 1, 1/frac) >= j) is at most 1 %, and k (no speculation) when no
such j exists."""
import math

import pytest

TARGET = 0.01


def _tail(k, f, j):
    n = k - 1
    return sum(math.comb(n, i) * f ** i * (1.0 - f) ** (n - i) for i in range(j, n + 1))


@pytest.mark.parametrize("k", [1, 10, 32, 100])
@pytest.mark.parametrize("frac", [4, 6, 8, 12, 16, 24, 32, 48])
def test_auto_rank_is_the_smallest_rank_inside_the_target(k, frac):
    from expann_amd import _lib
    L = _lib.load()
    j = L.expann_spec_rank_auto(k, frac)
    f = 1.0 / frac
    assert 1 <= j <= k
    want = next((x for x in range(1, k) if _tail(k, f, x) <= TARGET), k)
    # (the two sums round differently: accept the neighbour only where the tail sits on the target)
    if j != want:
        assert abs(j - want) == 1 and abs(_tail(k, f, min(j, want)) - TARGET) < 1e-9, (k, frac, j, want)
    if j < k:
        assert _tail(k, f, j) <= TARGET + 1e-12
        assert j == 1 or _tail(k, f, j - 1) > TARGET - 1e-12
    else:
        assert all(_tail(k, f, x) > TARGET - 1e-12 for x in range(1, k))


def test_reference_points():
    """k = 10 at 1/16 of the rows: 10.5 % of the queries fail at j = 2, 1.5 % at j = 3, 0.15 % at j = 4; k = 1 has
    nothing to speculate on"""
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_spec_rank_auto(10, 16) == 4
    assert L.expann_spec_rank_auto(1, 16) == 1
    assert 0.10 < _tail(10, 1 / 16, 2) < 0.11 and 0.014 < _tail(10, 1 / 16, 3) < 0.016 and _tail(10, 1 / 16, 4) < 0.002
