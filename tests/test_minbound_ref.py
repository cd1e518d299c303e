"""The exact reference of the minimum rotated rectangle and the minimum bounding circle (tests/minbound_ref.py) against itself and its
fixture: the fixture regenerates byte for byte, Welzl's algorithm agrees with brute force, and the rows pinned by hand hold."""
from fractions import Fraction

import numpy as np

from tests import minbound_ref as M
from tests.golden import make_minbound_golden


def test_fixture_is_reproducible_and_small(tmp_path):
    out = tmp_path / "minbound_lattice.npz"
    make_minbound_golden.main(str(out))
    assert out.read_bytes() == open(M.GOLDEN, "rb").read()
    assert out.stat().st_size < 400 * 1024
    z = np.load(M.GOLDEN)
    for fam in M.FAMILIES:
        xy = z[f"{fam}_xy"]
        ok = ~np.isnan(xy)
        assert (xy[ok] == np.round(xy[ok])).all(), fam  # integer coordinates only


def test_smallest_circle_agrees_with_brute_force():
    rng = np.random.default_rng(7)
    for _ in range(300):
        pts = [tuple(int(v) for v in p) for p in rng.integers(-20, 21, size=(int(rng.integers(1, 13)), 2))]
        a, b = M.smallest_circle(pts), M.smallest_circle_brute(pts)
        assert M._r2(a) == M._r2(b) and Fraction(a[0], a[2]) == Fraction(b[0], b[2]) and Fraction(a[1], a[2]) == Fraction(b[1], b[2]), pts


def test_pinned_rows():
    ref = M.row_reference([(0, 0), (4, 0), (1, 3)])  # acute: all three edges tie at twice the triangle's area
    assert ref["areas"] == [12, 12, 12] and ref["best_edge"] == 0
    ref = M.row_reference([(0, 0), (4, 0), (0, 3)])  # right: between two and three support points
    assert ref["centre"] == (2, Fraction(3, 2)) and ref["r2"] == Fraction(25, 4)
    ref = M.row_reference(M.CIRCLE5)
    assert ref["centre"] == (0, 0) and ref["radius"] == 5 and len(ref["hull"]) == 12
    ref = M.row_reference(M.IN_TRIANGLE)
    assert len(ref["hull"]) == 3
    for n in M.CONVEX_SIZES[:6]:
        assert len(M.row_reference(M.parabola(n))["hull"]) == n
    assert M.hull_ring([(4, 3), (1, 5), (0, 0), (4, 0), (2, 0)]) == [(0, 0), (4, 0), (4, 3), (1, 5)]


def test_acceptance_takes_the_exact_answer_and_refuses_a_wrong_one():
    import pytest

    pts = [(0.0, 0.0), (4.0, 0.0), (4.0, 3.0), (1.0, 5.0)]
    ref = M.row_reference(pts)
    ring = [(float(x), float(y)) for x, y in M.edge_rectangle(ref["hull"], ref["best_edge"], ref["ext"][ref["best_edge"]], ref["scale"])]
    assert M.check_rectangle(pts, ring + ring[:1]) <= 1.0
    assert M.check_circle(pts, float(ref["centre"][0]), float(ref["centre"][1]), float(ref["radius"])) <= 1.0
    with pytest.raises(AssertionError):
        M.check_rectangle(pts, [(0.0, 0.0), (4.0, 0.0), (4.0, 5.001), (0.0, 5.001), (0.0, 0.0)])  # a corner off by 1e-3
    with pytest.raises(AssertionError):
        M.check_rectangle([(0.0, 0.0), (6.0, 0.0), (1.0, 1.0)], [(3.0, 3.0), (0.0, 0.0), (3.0, -3.0), (6.0, 0.0), (3.0, 3.0)])  # exact, on an edge of larger area
    with pytest.raises(AssertionError):
        M.check_circle(pts, float(ref["centre"][0]), float(ref["centre"][1]), float(ref["radius"]) * 1.001)
