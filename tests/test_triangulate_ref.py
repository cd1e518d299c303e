"""The exact checker of tests/triangulate_ref.py against hand-made triangulations: it accepts the right ones and rejects each planted
defect.  (The checker against the rule itself — csrc/gpk_triangulate.h run on the CPU — is tests/test_triangulate_host.py.)"""
import numpy as np
import pytest

from tests import triangulate_ref as T
from tests import validity_ref as V

PG, MPG = V.PG, V.MPG
SQUARE = [[(0, 0), (4, 0), (4, 4), (0, 4), (0, 0)]]
# a hole that touches the shell's bottom edge mid-segment, at (2, 0): coordinates 0 - 3 the shell, 5 - 7 the hole, 4 and 8 closing
TOUCH = [[(0, 0), (4, 0), (4, 4), (0, 4), (0, 0)], [(2, 0), (1, 2), (3, 2), (2, 0)]]
TOUCH_TRIS = [(0, 5, 6), (5, 1, 7), (1, 2, 7), (2, 3, 7), (3, 6, 7), (3, 0, 6)]


def rejected(kind, row, tris, what, base=0):
    with pytest.raises(T.TriangulationError, match=what):
        T.check_row(kind, row, np.array(tris) + base, base)


def test_fixture_rows_are_what_they_claim():
    assert V.validity(PG, SQUARE)[0] == V.VALID and V.validity(PG, TOUCH)[0] == V.VALID


@pytest.mark.parametrize("base", [0, 37])
def test_accepts_right_answers(base):
    T.check_row(PG, SQUARE, np.array([(0, 1, 2), (0, 2, 3)]) + base, base)
    T.check_row(PG, SQUARE, np.array([(1, 2, 3), (1, 3, 0)]) + base, base)
    T.check_row(PG, TOUCH, np.array(TOUCH_TRIS) + base, base)
    T.check_row(MPG, [[], TOUCH, [V.sq(10, 0, 14, 4)]], np.array(TOUCH_TRIS + [(9, 10, 11), (9, 11, 12)]) + base, base)
    T.check_row(PG, [], np.zeros((0, 3)), base)


def test_rejects_a_dropped_triangle():
    rejected(PG, TOUCH, TOUCH_TRIS[:-1], r"\(d\)")
    rejected(PG, SQUARE, [(0, 1, 2)], r"\(d\)")


def test_rejects_a_flipped_triangle():
    rejected(PG, TOUCH, [(0, 6, 5)] + TOUCH_TRIS[1:], r"\(b\)")
    rejected(PG, SQUARE, [(0, 1, 2), (0, 2, 2)], r"\(b\)")  # (and a zero-area one)


def test_rejects_a_closing_coordinate():
    rejected(PG, SQUARE, [(4, 1, 2), (0, 2, 3)], r"\(a\) index of a closing")
    rejected(PG, TOUCH, [(0, 8, 6)] + TOUCH_TRIS[1:], r"\(a\) index of a closing")


def test_rejects_an_index_of_another_row():
    with pytest.raises(T.TriangulationError, match=r"\(a\) an index outside"):
        T.check_row(PG, SQUARE, np.array([(10, 11, 12), (10, 12, 9)]), 10)  # 9: the row before
    with pytest.raises(T.TriangulationError, match=r"\(a\) an index outside"):
        T.check_row(PG, SQUARE, np.array([(10, 11, 12), (10, 12, 15)]), 10)  # 15: the row behind


def test_rejects_a_t_junction():
    """(0, 4) (0, 0) (2, 0) in place of the two triangles it covers: the same area, but the hole's vertex (1, 2) lies inside its edge (2, 0) - (0, 4)"""
    assert T._strictly_inside((1, 2), (2, 0), (0, 4))
    rejected(PG, TOUCH, [(3, 0, 5)] + TOUCH_TRIS[1:5], r"\(c\)")
    # and on the boundary: a collinear shell vertex left out
    rejected(PG, [[(0, 0), (2, 0), (4, 0), (4, 4), (0, 4), (0, 0)]], [(0, 2, 3), (0, 3, 4)], r"\(c\)")
    # the touch point left out: the triangle on the whole bottom edge is not even inside
    rejected(PG, TOUCH, [(0, 1, 6)] + TOUCH_TRIS[2:], r"\(d\)|\(c\)")


def test_rejects_overlapping_triangles_whose_areas_sum_right():
    """a hexagon as two triangles through alternate corners: each half the area, six distinct directed edges"""
    hexagon = [[(2, 0), (4, 0), (6, 2), (4, 4), (2, 4), (0, 2), (2, 0)]]
    assert V.validity(PG, hexagon)[0] == V.VALID
    I = T._ints([tuple(map(float, p)) for p in hexagon[0]])
    star = [(I[0], I[2], I[4]), (I[1], I[3], I[5])]
    assert sum(abs(T._area2(list(t))) for t in star) == abs(T._area2(I[:-1]))
    assert T.first_overlap(star) == (0, 1)
    assert T.first_overlap([(I[0], I[1], I[2]), (I[0], I[2], I[5])]) is None  # (sharing an edge is no overlap)
    rejected(PG, hexagon, [(0, 2, 4), (1, 3, 5)], None)
    # a square as two triangles over the same diagonal side: a directed edge twice
    rejected(PG, SQUARE, [(0, 1, 2), (1, 2, 3)], r"\(c\) the directed edge")


def test_counts():
    """(e): exactly N' + 2 h - 2 where no rings share a point, at most N' + s + 2 h - 2 where they do"""
    donut = [V.BIG, V.sq(5, 5, 9, 9, cw=True)]
    fan = [(0, 1, 8), (0, 8, 5), (1, 2, 7), (1, 7, 8), (2, 3, 6), (2, 6, 7), (3, 0, 5), (3, 5, 6)]  # hole 5 (5,5) 6 (5,9) 7 (9,9) 8 (9,5)
    T.check_row(PG, donut, np.array(fan))
    rejected(PG, SQUARE + [], [(0, 1, 2), (0, 2, 3), (0, 1, 2)], r"\(d\)|\(c\)")
    assert T.share(PG, donut) == 10 + 6 and T.share(MPG, [[], TOUCH]) == 9 + 6
