"""The exact reference of gpk_validity / gpk_is_simple (tests/validity_ref.py) against hand-written answers, and its two decisions of
code 8 against each other."""
import numpy as np
import pytest

from tests import validity_ref as V


@pytest.mark.parametrize("name,kind,row,code", V.KNOWN, ids=[k[0] for k in V.KNOWN])
def test_known_answers(name, kind, row, code):
    assert V.validity(kind, row, row is not None)[0] == code
    if kind == V.PG:  # the same figure as a MULTIPOLYGON with an empty member in front
        assert V.validity(V.MPG, V.as_kind(V.PG, row, V.MPG), row is not None)[0] == code


def test_every_code_has_a_known_row():
    assert {k[3] for k in V.KNOWN} == set(range(10))


def test_where_of_the_known_rows():
    w = {k[0]: V.validity(k[1], k[2], k[2] is not None, base=100) for k in V.KNOWN}
    assert w["square"] == (V.VALID, -1) and w["null row"] == (V.NULL, -1)
    assert w["NaN coordinate"] == (V.COORDINATE, 107)  # the third coordinate of the hole
    assert w["short hole"] == (V.RING_SHAPE, 105)  # the hole's first coordinate
    assert w["bow-tie"] == (V.SELF_INTERSECTION, 100)
    assert w["spike A-B-A"] == (V.SELF_INTERSECTION, 101)  # (4, 0) -> (4, 4) meets (7, 7) -> (4, 4), not its neighbour
    assert w["one point"] == (V.SELF_INTERSECTION, 100)
    assert w["hole crossing the shell"] == (V.RINGS_CROSS, 101)  # the shell's right edge
    assert w["hole outside the shell"] == (V.HOLE_OUTSIDE, 105)
    assert w["hole in a hole"] == (V.NESTED_HOLES, 110)
    assert w["member inside a member"] == (V.NESTED_MEMBERS, 105)
    assert w["member around a member"] == (V.NESTED_MEMBERS, 110)
    assert w["a chain of holes from shell to shell"] == (V.DISCONNECTED, 100)


@pytest.mark.parametrize("name,kind,row,simple", V.KNOWN_SIMPLE, ids=[k[0] for k in V.KNOWN_SIMPLE])
def test_known_simplicity(name, kind, row, simple):
    assert V.is_simple(kind, row, row is not None) == simple
    if kind == V.LS and row is not None:
        assert V.is_simple(V.MLS, [[], row]) == simple


def test_placements_keep_the_reference_answers():
    rows, valid, codes, where = V.known_column(V.MPG)
    finite = [i for i, c in enumerate(codes) if c != V.COORDINATE]
    for scale, shift in V.PLACEMENTS:
        c, w = V.validity_column(V.MPG, V.placed(V.MPG, [rows[i] for i in finite], scale, shift), [valid[i] for i in finite])
        assert np.array_equal(c, codes[finite])


def test_flood_fill_agrees_with_the_touch_graph():
    """random rectilinear members: a 16 x 16 shell with 2 x 2 holes at even positions that may touch each other at corners (sets in
    which two holes share an edge are discarded: code 4 comes first), half of them grown from four holes round a cell; both decisions
    of `disconnected` must agree"""
    rng = np.random.default_rng(3)
    seen = {False: 0, True: 0}
    for k in range(60):
        rings = [V.sq(0, 0, 16, 16)]
        spots = set()
        if k % 2:
            x, y = int(rng.integers(1, 4)) * 2, int(rng.integers(1, 4)) * 2
            spots |= {(x, y + 2), (x + 2, y + 4), (x + 4, y + 2), (x + 2, y)}
        for _ in range(int(rng.integers(1, 4))):
            spots.add((int(rng.integers(1, 7)) * 2, int(rng.integers(1, 7)) * 2))
        rings += [V.sq(x, y, x + 2, y + 2, cw=True) for x, y in sorted(spots)]
        code, _ = V.validity(V.PG, rings)
        if code not in (V.VALID, V.DISCONNECTED):
            continue
        cut = V.flood_fill_cut(rings)
        assert cut == (code == V.DISCONNECTED), rings
        seen[cut] += 1
    assert seen[False] >= 8 and seen[True] >= 8, seen
    for name, kind, row, code in V.KNOWN:  # and on the rectilinear known answers
        if kind == V.PG and row and code in (V.VALID, V.DISCONNECTED) and all(x0 == x1 or y0 == y1 for r in row for (x0, y0), (x1, y1) in zip(r, r[1:])):
            assert V.flood_fill_cut(row) == (code == V.DISCONNECTED), name


def test_random_fixture_holds_every_code():
    for kind in (V.PG, V.MPG):
        codes = V.random_column(kind)[2]
        count = np.bincount(codes, minlength=10)
        for c in range(9):
            if c == V.NESTED_MEMBERS and kind == V.PG:
                continue  # (one member only)
            assert count[c] >= 3, (kind, c, count.tolist())
