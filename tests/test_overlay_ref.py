"""The exact reference of the intersection measures checks itself: hand answers, symmetry, area(A, A) = area(A), the closed form for
rectangles, the validity of every fixture polygon, and that tests/golden/overlay_lattice.npz is what regenerate() writes."""
from fractions import Fraction

import numpy as np
import pytest

from tests import overlay_ref as O
from tests import polyrel_ref as P
from tests import relation_ref as R

PG, MPG, LS, MLS = O.PG, O.MPG, O.LS, O.MLS


def _shoelace_area(polys) -> Fraction:
    """the area of a valid list of polygons from its rings alone: shells minus holes"""
    total = Fraction(0)
    for poly in polys:
        for k, r in enumerate(poly):
            a = np.asarray(r, dtype=object)
            twice = abs(sum(a[i][0] * a[i + 1][1] - a[i + 1][0] * a[i][1] for i in range(len(a) - 1)))
            total += Fraction(twice, 2) * (1 if k == 0 else -1)
    return total


@pytest.mark.parametrize("case", O.AREA_CASES, ids=[c[0] for c in O.AREA_CASES])
def test_area_hand_answers_and_symmetry(case):
    _, a, b, want = case
    assert O.exact_area(MPG, a, MPG, b) == want
    assert O.exact_area(MPG, b, MPG, a) == want
    for g in (a, b):
        assert O.exact_area(MPG, g, MPG, g) == _shoelace_area(g)
    if len(a) == 1 and len(b) == 1:
        assert O.exact_area(PG, a[0], PG, b[0]) == want


@pytest.mark.parametrize("case", O.LENGTH_CASES, ids=[c[0] for c in O.LENGTH_CASES])
def test_length_hand_answers(case):
    _, seqs, polys, want = case
    assert abs(float(O.exact_length(MLS, seqs, MPG, polys)) - want) < 1e-13
    back = [list(s)[::-1] for s in seqs]  # the same point set walked the other way
    assert abs(float(O.exact_length(MLS, back, MPG, polys)) - want) < 1e-13
    assert float(O.exact_length(MLS, seqs, MPG, polys)) <= O.line_length(MLS, seqs) + 1e-13


def test_rectangles_closed_form():
    rng = np.random.default_rng(5)
    for _ in range(200):
        x0, y0, x2, y2 = (int(v) for v in rng.integers(-20, 20, 4))
        w0, h0, w2, h2 = (int(v) for v in rng.integers(1, 25, 4))
        a, b = O.sq(x0, y0, x0 + w0, y0 + h0, cw=bool(rng.integers(2))), O.sq(x2, y2, x2 + w2, y2 + h2)
        want = max(0, min(x0 + w0, x2 + w2) - max(x0, x2)) * max(0, min(y0 + h0, y2 + h2) - max(y0, y2))
        assert O.exact_area(PG, [a], PG, [b]) == want
        # a horizontal line through the first rectangle, inside the second
        y = y0 + h0 // 2
        inside = max(0, min(x0 + w0, x2 + w2) - max(x0, x2)) if y2 <= y <= y2 + h2 else 0
        assert float(O.exact_length(LS, [(x0, y), (x0 + w0, y)], PG, [b])) == inside


def test_unusable_rows_have_no_measure():
    assert O.exact_area(PG, [], PG, [O.S10]) is None and O.exact_area(PG, [O.S10], PG, [O.S10], b_valid=False) is None
    assert O.exact_area(PG, [[(0, 0), (4, 0), (4, 4), (0, 4)]], PG, [O.S10]) is None  # unclosed
    assert O.exact_length(LS, [], PG, [O.S10]) is None and O.exact_length(LS, [(0, 0), (np.nan, 1)], PG, [O.S10]) is None
    assert O.exact_length(LS, [(0, 0), (np.inf, 1)], PG, [O.S10]) is None and O.exact_length(MLS, [[]], PG, [O.S10]) is None


def test_every_fixture_polygon_is_valid():
    for ka, kb in O.AREA_FAMILIES:
        A, B = O.area_rows(ka, kb)
        assert len(A) == len(B) >= 200
        for kind, rows in ((ka, A), (kb, B)):
            for r in rows:
                assert R.polygon_valid(kind, r), (kind, r)
    for kl, kp in O.LENGTH_FAMILIES:
        L, Q = O.length_rows(kl, kp)
        assert len(L) == len(Q) >= 200
        for r in Q:
            assert R.polygon_valid(kp, r), r
    left, right, lines = O.join_rows()
    assert len(left) == len(right) == len(lines) == 200
    for r in left + right:
        assert R.polygon_valid(PG, r), r


def test_fixture_holds_the_stride_rows_and_ties():
    A, B = O.area_rows(PG, PG)
    edges = {len(r[0]) - 1 for r in A}
    assert {5, 33} <= edges and any(len(r) > 1 and len(r[1]) == 40 for r in A)
    z = np.load(O.GOLDEN)
    for what, ka, kb in O.families():
        exact = z[O.fixture_key(what, ka, kb) + "exact"]
        assert (exact == 0).sum() >= 10 and (exact > 0).sum() >= 100  # touching and apart rows next to overlapping ones


def test_regeneration_reproduces_the_golden_file():
    z = np.load(O.GOLDEN)
    arrays = O.build_arrays()
    assert set(z.files) == set(arrays)
    for k, v in arrays.items():
        assert z[k].dtype == np.asarray(v).dtype and np.array_equal(z[k], v), k
