"""CPU: the exact reference of the non-point row-wise distance (tests/pair_distance_ref.py) held against independent answers:
the C oracle's exact segment test (gpko_line_intersects_line) and polygonal `intersects` (gpko_predicate_pair, through
predicate_rowwise), sympy's rational geometry, and brute-force f64 on lattice inputs (where every distance is far from a rounding)."""
from fractions import Fraction

import numpy as np
import pytest

from geopolars_amd import _abi
from tests import exact_ref as X
from tests import pair_distance_ref as R

MP, LS, MLS, PG, MPG = _abi.GEOM_MULTIPOINT, _abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON


def _lattice_segments(rng, n, span=6):
    pts = rng.integers(0, span, (n, 4)).astype(np.float64)
    pts[: n // 8, 2:] = pts[: n // 8, :2]  # some degenerate segments
    return pts


def test_segment_test_matches_the_oracle(oracle):
    rng = np.random.default_rng(1)
    a, b = _lattice_segments(rng, 3000), _lattice_segments(rng, 3000)
    hits = 0
    for p, q in zip(a, b):
        mine = R.segments_intersect(p[:2], p[2:], q[:2], q[2:])
        assert mine == oracle.line_intersects_line(p[:2], p[2:], q[:2], q[2:]), (p, q)
        hits += mine
    assert 300 < hits < 2700  # both outcomes well represented (touching and collinear cases included on a small lattice)


def _lattice_polygon(rng, holes):
    x0, y0 = rng.integers(0, 12, 2)
    w, h = rng.integers(2, 8, 2)
    rings = [[(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h), (x0, y0)]]
    if holes and w >= 3 and h >= 3:
        rings.append([(x0 + 1, y0 + 1), (x0 + 1, y0 + h - 1), (x0 + w - 1, y0 + h - 1), (x0 + w - 1, y0 + 1), (x0 + 1, y0 + 1)])
    return [[(float(x), float(y)) for x, y in r] for r in rings]


def test_polygonal_intersects_matches_the_oracle(oracle):
    rng = np.random.default_rng(2)
    ra = [[_lattice_polygon(rng, True) for _ in range(rng.integers(1, 3))] for _ in range(400)]
    rb = [[_lattice_polygon(rng, True) for _ in range(rng.integers(1, 3))] for _ in range(400)]
    want = oracle.predicate_rowwise(X.column(MPG, ra), X.column(MPG, rb), "intersects")
    mine = np.array([R.intersects(MPG, x, MPG, y) for x, y in zip(ra, rb)])
    assert np.array_equal(mine, want)
    assert 40 < want.sum() < 360
    for x, y, w in zip(ra, rb, want):  # and the distance is zero exactly there
        assert (R.distance2(MPG, x, MPG, y) == 0) == w


def test_distances_match_sympy():
    sg = pytest.importorskip("sympy.geometry")
    from sympy import Rational, simplify

    def sq(d):  # a squared distance between rational points is rational
        e = simplify(d**2)
        assert e.is_Rational, e
        return Fraction(int(e.p), int(e.q))

    rng = np.random.default_rng(3)
    for _ in range(60):
        a = rng.integers(-20, 20, (2, 2)).astype(float) + rng.integers(0, 8, (2, 2)) / 8
        b = rng.integers(-20, 20, (2, 2)).astype(float) + rng.integers(0, 8, (2, 2)) / 8
        if (a[0] == a[1]).all() or (b[0] == b[1]).all():
            continue
        sa = sg.Segment(*[sg.Point(Rational(x), Rational(y)) for x, y in a])
        sb = sg.Segment(*[sg.Point(Rational(x), Rational(y)) for x, y in b])
        if sa.intersection(sb):
            want = Fraction(0)
        else:
            want = min([sq(sa.distance(p)) for p in sb.points] + [sq(sb.distance(p)) for p in sa.points])
        assert R.distance2(LS, [tuple(x) for x in a], LS, [tuple(x) for x in b]) == want, (a, b)
    # convex polygons: sympy's Polygon.distance (defined for disjoint convex polygons)
    for _ in range(20):
        c = rng.integers(-20, 20, 2)
        p1 = [(0, 0), (4, 0), (5, 3), (1, 4)]
        p2 = [(x + int(c[0]) + 12, y + int(c[1])) for x, y in [(0, 0), (3, 1), (2, 4)]]
        P1, P2 = sg.Polygon(*p1), sg.Polygon(*p2)
        if P1.intersection(P2) or P1.encloses_point(p2[0]) or P2.encloses_point(p1[0]):
            continue
        want = sq(P1.distance(P2))
        r1 = [[tuple(map(float, q)) for q in p1 + p1[:1]]]
        r2 = [[tuple(map(float, q)) for q in p2 + p2[:1]]]
        assert R.distance2(PG, r1, PG, r2) == want


def test_distances_match_brute_force_on_a_lattice():
    rng = np.random.default_rng(4)
    for _ in range(200):
        ka, kb = rng.choice([MP, LS, MLS]), rng.choice([MP, LS, MLS])

        def row(k):
            pts = [tuple(map(float, p)) for p in rng.integers(0, 40, (int(rng.integers(1, 6)), 2))]
            if k == MLS:
                return [pts, [(p[0] + 50.0, p[1]) for p in pts]]
            return pts

        a, b = row(ka), row(kb)
        got = R.distance2(ka, a, kb, b)
        a0, a1 = R.segments(ka, a)
        b0, b1 = R.segments(kb, b)
        f = min(min(X._f64_seg_dist(p, b0, b1).min() for p in a0), min(X._f64_seg_dist(p, a0, a1).min() for p in b0))
        inter = any(R.segments_intersect(a0[i], a1[i], b0[j], b1[j]) for i in range(len(a0)) for j in range(len(b0)))
        if inter:
            assert got == 0
        else:
            assert got > 0 and abs(float(got) ** 0.5 - f) <= 1e-12 * max(f, 1.0)


def test_nan_rules_and_degenerate_sequences():
    assert R.distance(LS, [], PG, [[(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0)]])[0] is None
    assert R.distance(MPG, [[[]]], MP, [(1.0, 1.0)])[0] is None
    assert R.distance(MP, [], MP, [(1.0, 1.0)])[0] is None
    assert R.rowwise(LS, [[(0.0, 0.0)]], LS, [[(3.0, 4.0)]], b_rows=[1])[0][0] is None  # out of range
    assert R.rowwise(LS, [[(0.0, 0.0)]], LS, [[(3.0, 4.0)]], valid_a=[False])[0][0] is None
    d, _ = R.distance(LS, [(0.0, 0.0)], LS, [(3.0, 4.0)])  # one-coordinate linestrings: hypot
    assert float(d) == 5.0
    d, _ = R.distance(MLS, [[], [(0.0, 3.0), (0.0, 5.0)]], LS, [(-4.0, 0.0), (4.0, 0.0)])  # empty members are ignored
    assert float(d) == 3.0
    # a polygon in another's hole: the hole ring counts; touching it: 0
    outer = [[(0.0, 0.0), (10.0, 0.0), (10.0, 10.0), (0.0, 10.0), (0.0, 0.0)], [(3.0, 3.0), (3.0, 7.0), (7.0, 7.0), (7.0, 3.0), (3.0, 3.0)]]
    inner = [[(4.0, 4.0), (6.0, 4.0), (6.0, 6.0), (4.0, 6.0), (4.0, 4.0)]]
    assert float(R.distance(PG, inner, PG, outer)[0]) == 1.0
    touch = [[(3.0, 4.0), (6.0, 4.0), (6.0, 6.0), (3.0, 6.0), (3.0, 4.0)]]
    assert R.distance(PG, touch, PG, outer)[0] == 0
