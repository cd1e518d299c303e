"""The exact within-distance reference (tests/dwithin_ref.py) on hand-made cases, and the precondition the GPU tests rely on: on every
committed fixture, at every threshold of the exact comparison, no pair's exact distance lies within the distance routines' a-priori
bound of the threshold.  The share of pairs a GPU test may leave out as "too close to call" is therefore zero."""
from fractions import Fraction

import numpy as np
import pytest

from tests import dwithin_ref as W
from tests import exact_ref as X

PT, MP, LS, MLS, PG, MPG = W.PT, W.MP, W.LS, W.MLS, W.PG, W.MPG


def _sq(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]


def test_three_four_five_and_closedness():
    left = (PT, [(0.0, 0.0), (10.0, 10.0)], None)
    right = (MP, [[(3.0, 4.0), (50.0, 50.0)], [(10.0, 12.0)]], None)
    assert W.dwithin_exact(left, right, 5.0) == [(0, 0), (1, 1)]
    assert W.dwithin_exact(left, right, float(np.nextafter(5.0, 0.0))) == [(1, 1)]
    assert W.dwithin_exact(left, right, 2.0) == [(1, 1)]
    assert W.dwithin_exact(left, right, float(np.nextafter(2.0, 0.0))) == []
    table = W.exact_table(left, right)
    assert table[(0, 0)][0] == Fraction(25) and table[(1, 1)][0] == Fraction(4)
    assert W.classify(table, 5.0)[1] == [(0, 0)]  # a pair exactly on the threshold is "too close to call" for a rounded distance


def test_zero_threshold_is_touching_crossing_or_contained():
    ulp_y = float(np.nextafter(1.0, 2.0))
    left = (LS, [[(1.0, 1.0), (1.0, 5.0)], [(1.0, ulp_y), (1.0, 5.0)], [(2.0, 2.0), (3.0, 3.0)], [(0.0, 9.0), (9.0, 0.0)]], None)
    right = (PG, [[_sq(0.0, -1.0, 4.0, 1.0)], [_sq(1.5, 1.5, 8.0, 8.0), _sq(1.75, 1.75, 3.5, 3.5)[::-1]]], None)
    # row 0 touches polygon 0's edge; row 1 is one ulp above it; row 2 lies in polygon 1's hole; row 3 crosses polygon 1
    assert W.dwithin_exact(left, right, 0.0) == [(0, 0), (3, 1)]
    assert W.classify(W.exact_table(left, right), 0.0, exact_zero=True)[1] == []  # two non-point rows: zero / non-zero is exact
    assert W.classify(W.exact_table(left, right), 0.0)[1] == [(1, 0)]  # by the bound alone the ulp-off pair is too close to call
    d2, lmax = W.exact_table(left, right)[(1, 0)]
    assert d2 == Fraction(ulp_y - 1.0) ** 2


def test_never_matched_rows():
    nan = float("nan")
    left = (PT, [(0.0, 0.0), None, (nan, 0.0), (0.0, 0.0)], [True, True, True, False])
    right = (LS, [[(0.0, 0.0), (1.0, 0.0)], [], [(0.0, 1.0), (1.0, 1.0)]], [True, True, False])
    assert W.dwithin_exact(left, right, 100.0) == [(0, 0)]
    assert W.dwithin_exact((MPG, [[], [[[]]], [[_sq(0.0, 0.0, 1.0, 1.0)]]], None), (MP, [[(0.5, 0.5)], []], None), 1.0) == [(2, 0)]


def test_both_orders_agree():
    a = (LS, [[(0.0, 0.0), (4.0, 0.0)], [(10.0, 10.0), (11.0, 10.0)]], None)
    b = (PG, [[_sq(1.0, 3.0, 2.0, 4.0)], [_sq(10.0, 12.0, 11.0, 13.0)]], None)
    ab, ba = W.dwithin_exact(a, b, 3.0), W.dwithin_exact(b, a, 3.0)
    assert ab == [(0, 0), (1, 1)] and sorted((r, l) for l, r in ba) == ab


@pytest.mark.parametrize("key", W.POINT_FIXTURES, ids=lambda k: f"{k[0]}-G{k[1]}-{'pl' if k[2] else 'pr'}")
def test_point_fixtures_have_no_pair_near_a_threshold(key):
    family, G, point_left = key
    left, right = W.point_fixture(*key)
    other = right if point_left else left
    assert X.group_size_of(X.column(*other)) == G, "the kept rows select another kernel instance"
    table = W.fixture_table(key)
    assert len(table) > 100
    sizes = []
    for t in W.THRESHOLDS:
        within, close = W.classify(table, t)
        assert close == [], (key, t, close)
        sizes.append(len(within))
    assert sizes == sorted(sizes) and 0 < sizes[1] and sizes[2] < sizes[3] < len(table), sizes  # the thresholds cut the fixture
    if family in ("linestring", "multilinestring", "polygon", "multipolygon"):
        assert sizes[0] > 0, "no pair at distance 0"


@pytest.mark.parametrize("key", W.PAIR_FIXTURES, ids=lambda k: f"{k[0]}x{k[1]}-{k[2]}")
def test_pair_fixtures_have_no_pair_near_a_threshold(key):
    ka, kb, size = key
    left, right = W.pair_fixture(*key)
    costs = [sum(len(s) for s in X.row_seqs(ka, x)) * sum(len(s) for s in X.row_seqs(kb, y)) for x in left[1] for y in right[1] if len(x) and len(y)]
    a, b = W.columns(left, right)
    mean = max(c.n_coords / c.n_geoms for c in (a, b))
    if size == "large":
        assert min(costs) > W.LARGE_COST
    else:
        assert max(costs) <= W.LARGE_COST and (mean >= 128) == (size == "g32"), (mean, max(costs))
    table = W.fixture_table(key)
    sizes = []
    for t in W.THRESHOLDS:
        within, close = W.classify(table, t, exact_zero=True)
        assert close == [], (key, t, close)
        sizes.append(len(within))
    assert sizes == sorted(sizes) and sizes[2] > 0 and sizes[3] == len(table), sizes


def test_margin_cases_round_as_described():
    t, cases = W.margin_cases()
    assert len(cases) == 6
    for a, b in cases:
        assert b - a == t and a + t < b and b - t > a  # the difference rounds onto t; neither grown edge reaches the other box
        assert Fraction(b) - Fraction(a) > Fraction(t)  # (exactly, the pair is farther than t: only the computed distance is within)
