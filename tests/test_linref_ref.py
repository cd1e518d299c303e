"""The exact reference of linear referencing (tests/linref_ref.py) on hand-made answers, and the accuracy bounds of the kernel's
formulas: a Python f64 mirror of gpk_linref.h (segment_dist2's branches, q, the measure) against the exact reference on the
random columns the GPU test uses.  No GPU."""
import decimal
from fractions import Fraction

import numpy as np

from geopolars_amd import _abi
from tests import linref_ref as R

LS, MLS, PG, MPG, MP, PT = (_abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON,
                            _abi.GEOM_MULTIPOINT, _abi.GEOM_POINT)
D = decimal.Decimal


def test_345_triangle_interior_of_a_segment():
    line = [(0.0, 0.0), (10.0, 0.0), (10.0, 10.0)]
    r = R.closest((3.0, 4.0), LS, line)
    assert (r["seg"], r["end"]) == (0, 1) and r["d2"] == 16 and r["t"] == Fraction(3, 10) and r["q"] == (3, 0)
    assert R.measure(LS, line, r) == D(3) and R.measure(LS, line, r, normalized=True) == D(3) / D(20)
    r = R.closest((13.0, 6.0), LS, line)  # nearest to the second segment
    assert r["seg"] == 1 and r["d2"] == 9 and r["q"] == (10, 6) and R.measure(LS, line, r) == D(16)
    # the hypotenuse: (0,0) -> (3,4), a point at right angles from its middle
    r = R.closest((1.5 + 4.0, 2.0 - 3.0), LS, [(0.0, 0.0), (3.0, 4.0)])
    assert r["d2"] == 25 and r["t"] == Fraction(1, 2) and r["q"] == (Fraction(3, 2), 2) and R.locate((5.5, -1.0), LS, [(0.0, 0.0), (3.0, 4.0)]) == D("2.5")


def test_point_beyond_either_end():
    line = [(0.0, 0.0), (3.0, 4.0), (6.0, 0.0)]
    r = R.closest((-3.0, -4.0), LS, line)
    assert r["seg"] == 0 and r["t"] == 0 and r["q"] == (0, 0) and r["d2"] == 25 and R.measure(LS, line, r) == 0
    r = R.closest((9.0, -4.0), LS, line)
    assert r["seg"] == 1 and r["t"] == 1 and r["q"] == (6, 0) and R.measure(LS, line, r) == D(10)
    assert R.measure(LS, line, r, normalized=True) == D(1)


def test_shared_vertex_goes_to_the_lower_segment_and_is_not_ambiguous():
    line = [(0.0, 0.0), (4.0, 0.0), (4.0, 4.0)]
    p = (6.0, -2.0)  # nearest to the shared vertex (4, 0): both segments tie
    r = R.closest(p, LS, line)
    assert r["seg"] == 0 and r["t"] == 1 and r["q"] == (4, 0) and len(r["near"]) == 2
    assert not R.ambiguous(p, r)
    assert R.measure(LS, line, r) == D(4)


def test_point_equidistant_from_two_far_segments_is_ambiguous_and_takes_the_lowest_index():
    line = [(0.0, 0.0), (10.0, 0.0), (10.0, 6.0), (0.0, 6.0)]
    p = (2.0, 3.0)
    r = R.closest(p, LS, line)
    assert r["seg"] == 0 and r["q"] == (2, 0) and r["d2"] == 9
    assert R.ambiguous(p, r)
    assert R.on_some_segment((2.0, 6.0), LS, line, 1e-12) and not R.on_some_segment((2.0, 5.0), LS, line, 1e-12)
    assert not R.ambiguous((2.0, 2.0), R.closest((2.0, 2.0), LS, line))


def test_closed_ring_and_polygon_positions():
    ring = [(0.0, 0.0), (8.0, 0.0), (8.0, 8.0), (0.0, 8.0), (0.0, 0.0)]
    hole = [(2.0, 2.0), (2.0, 6.0), (6.0, 6.0), (6.0, 2.0), (2.0, 2.0)]
    r = R.closest((4.0, 1.0), LS, ring)  # a ring as a linestring: its inside is not part of it
    assert r["seg"] == 0 and r["q"] == (4, 1 - 1) and not r["inside"]
    assert R.locate((-1.0, 4.0), LS, ring) == D(28) and R.locate((0.0, 0.0), LS, ring) == 0  # the closing vertex: the start wins
    poly = [ring, hole]
    r = R.closest((1.0, 1.0), PG, poly)
    assert r["inside"] and r["seg"] == -1 and r["q"] == (1, 1) and r["d2"] == 0
    assert R.closest((8.0, 3.0), PG, poly)["inside"] and R.closest((2.0, 3.0), PG, poly)["inside"]  # on either boundary
    r = R.closest((4.0, 3.0), PG, poly)  # in the hole: outside; the hole's ring starts at local coordinate 5
    assert not r["inside"] and r["seg"] == 5 + 3 and r["q"] == (4, 2) and r["d2"] == 1
    r = R.closest((11.0, 4.0), MPG, [[ring], [[(14.0, 0.0), (20.0, 0.0), (20.0, 8.0), (14.0, 8.0), (14.0, 0.0)]]])
    assert r["seg"] == 1 and r["q"] == (8, 4) and r["d2"] == 9  # 3 from both parts: the lower index
    assert R.ambiguous((11.0, 4.0), r)


def test_points_and_multipoints_are_degenerate_segments():
    r = R.closest((0.0, 0.0), MP, [(3.0, 4.0), (-3.0, 4.0), (1.0, 1.0)])
    assert r["seg"] == 2 and r["end"] == 2 and r["q"] == (1, 1) and r["d2"] == 2
    r = R.closest((0.0, 0.0), MP, [(3.0, 4.0), (-3.0, 4.0)])
    assert r["seg"] == 0 and R.ambiguous((0.0, 0.0), r)
    assert R.closest((0.0, 0.0), PT, (3.0, 4.0))["d2"] == 25
    assert R.closest((0.0, 0.0), PT, None) is None and R.closest((0.0, 0.0), MP, []) is None and R.closest((0.0, 0.0), MLS, [[], []]) is None


def test_multilinestring_gaps_have_no_length():
    row = [[(0.0, 0.0), (3.0, 0.0)], [], [(100.0, 0.0), (100.0, 4.0)], [(7.0, 7.0)], [(200.0, 0.0), (203.0, 4.0)]]
    assert R.total_length(MLS, row) == D(12)
    r = R.closest((101.0, 1.0), MLS, row)
    assert r["seg"] == 2 and r["q"] == (100, 1) and R.measure(MLS, row, r) == D(4)
    r = R.closest((7.0, 8.0), MLS, row)  # the one-coordinate member: a degenerate segment at measure 7
    assert (r["seg"], r["end"]) == (4, 4) and R.measure(MLS, row, r) == D(7)
    assert R.locate((204.0, 5.0), MLS, row) == D(12) and R.locate((204.0, 5.0), MLS, row, normalized=True) == D(1)
    # interpolate: a measure on a member boundary is the end of the earlier member
    assert R.interpolate(MLS, row, 3.0) == (D(3), D(0))
    assert R.interpolate(MLS, row, 3.5) == (D(100), D("0.5"))
    assert R.interpolate(MLS, row, 7.0) == (D(100), D(4))
    assert R.interpolate(MLS, row, 9.5) == (D("201.5"), D(2))


def test_zero_length_lines():
    assert R.locate((5.0, 5.0), LS, [(1.0, 2.0), (1.0, 2.0)]) == 0
    assert R.locate((5.0, 5.0), LS, [(1.0, 2.0), (1.0, 2.0)], normalized=True) == 0
    assert R.interpolate(LS, [(1.0, 2.0), (1.0, 2.0)], 3.0) == (D(1), D(2))
    assert R.interpolate(MLS, [[(1.0, 2.0)], [(5.0, 5.0)]], 0.5, normalized=True) == (D(1), D(2))
    assert R.interpolate(LS, [], 1.0) is None and R.interpolate(LS, [(0.0, 0.0), (1.0, 0.0)], float("nan")) is None


def test_interpolate_negative_and_overshooting_distances():
    line = [(0.0, 0.0), (3.0, 4.0), (3.0, 10.0)]  # lengths 5 and 6
    assert R.interpolate(LS, line, 0.0) == (D(0), D(0))
    assert R.interpolate(LS, line, 2.5) == (D("1.5"), D(2))
    assert R.interpolate(LS, line, 5.0) == (D(3), D(4))  # exactly a vertex
    assert R.interpolate(LS, line, 8.0) == (D(3), D(7))
    assert R.interpolate(LS, line, -3.0) == (D(3), D(7))  # from the end
    assert R.interpolate(LS, line, -11.0) == (D(0), D(0)) and R.interpolate(LS, line, -40.0) == (D(0), D(0))
    assert R.interpolate(LS, line, 11.0) == (D(3), D(10)) and R.interpolate(LS, line, 1e9) == (D(3), D(10))
    assert R.interpolate(LS, line, 0.5, normalized=True) == (D(3), D("4.5"))
    assert R.interpolate(LS, line, -0.5, normalized=True) == (D(3), D("4.5"))
    assert R.interpolate(LS, line, 2.0, normalized=True) == (D(3), D(10))


def test_rows_of_and_coord_base_follow_the_column_layout():
    cols = R.random_columns()
    for name, (col, pts) in cols.items():
        kind, rows = R.rows_of(col)
        assert kind == col.geom_type and len(rows) == len(col) == len(pts)
        j = len(rows) // 2
        first = R.sequences(kind, rows[j])[0][1][0]
        assert tuple(col.xy[R.coord_base(col, j)]) == first, name


def test_f64_mirror_of_the_kernel_formulas_is_within_the_bounds_on_the_random_columns():
    """The bounds of the issue, checked on the CPU before any GPU run: on every unambiguous row the sequential f64 evaluation of the
    kernel's formulas picks the reference's segment, q is within 2^-48 max(|p|, |s|, |e|) per component and the measure within
    1e-9 x length; ambiguous rows are at most 1 % of every column."""
    for name, (col, pts) in R.random_columns().items():
        kind, rows = R.rows_of(col)
        n_amb = 0
        for i, row in enumerate(rows):
            p = (float(pts[i, 0]), float(pts[i, 1]))
            ex, mi = R.closest(p, kind, row), R.mirror_closest(p, kind, row)
            assert (ex is None) == (mi is None), (name, i)
            if ex is None:
                continue
            if R.ambiguous(p, ex):
                n_amb += 1
                continue
            q, seg, m, total = mi
            assert seg == ex["seg"], (name, i, seg, ex["seg"])
            if ex["inside"]:
                assert q == p
                continue
            b = R.q_bound(p, ex["s"], ex["e"])
            assert R.dec_err(q[0], ex["q"][0]) <= b and R.dec_err(q[1], ex["q"][1]) <= b, (name, i, q, ex["q"], b)
            if kind in (LS, MLS):
                L = R.total_length(kind, row)
                assert R.dec_err(m, R.measure(kind, row, ex)) <= R.M_REL * float(L), (name, i, m)
                assert abs(total - float(L)) <= R.M_REL * float(L)
        assert n_amb <= 0.01 * len(rows), (name, n_amb, len(rows))


def test_mirror_takes_the_lowest_index_among_exact_ties():
    row = [(0.0, 0.0), (8.0, 0.0), (8.0, 6.0), (0.0, 6.0), (0.0, 0.0), (8.0, 0.0)]  # the first segment twice
    q, seg, m, total = R.mirror_closest((4.0, 3.0), LS, row)
    assert seg == 0 == R.closest((4.0, 3.0), LS, row)["seg"] and q == (4.0, 0.0) and m == 4.0 and total == 36.0
    assert np.isclose(float(R.locate((4.0, 3.0), LS, row)), 4.0)
