"""No GPU, no library: tests/pointrel_ref.py pinned — its hand-derived answers, its agreement with the references of the sibling
relations where they make the same statement, the list of masks that can occur, and the condition that keeps the random tests honest."""
import itertools

import numpy as np
import pytest

from tests import linerel_ref as L
from tests import pointrel_ref as P
from tests import relation_ref as R

PT, MPT, LS, MLS, PG, MPG = P.PT, P.MPT, P.LS, P.MLS, P.PG, P.MPG
FAMILY_IDS = [f"{P.NAMES[a]}-{P.NAMES[b]}" for a, b in P.FAMILIES]


def test_families_and_names():
    assert len(P.FAMILIES) == 12 and {a for a, _ in P.FAMILIES} == {PT, MPT} and {b for _, b in P.FAMILIES} == {PT, MPT, LS, MLS, PG, MPG}
    assert set(P.PREDICATES) == {"intersects", "disjoint", "within", "covered_by", "contains", "covers", "touches", "equals", "crosses", "overlaps"}
    assert P.PRED_IDS == L.PRED_IDS


@pytest.mark.parametrize("ka,kb", P.FAMILIES, ids=FAMILY_IDS)
def test_known_answers(ka, kb):
    seen = 0
    for cases in (P.KNOWN, P.TIES):
        for pad in (0, 40):
            a, b, want, names = P.case_columns(cases, ka, kb, pad)
            got = P.masks(ka, a, kb, b)
            assert np.array_equal(got, want), [(n, int(g), int(w)) for n, g, w in zip(names, got, want) if g != w]
            seen += len(a)
    assert seen >= 4


def test_every_tie_the_issue_names_is_there():
    names = " | ".join(c[0] for c in P.TIES)
    for part in ("on a vertex", "inside an edge", "on a hole ring", "strictly in a hole", "where a hole touches its shell", "at a line's end",
                 "two members end: interior", "three members end: boundary", "closed ring line", "self-crossing that is no coordinate",
                 "degenerate member", "equal as sets, duplicates and another order", "a proper subset", "a proper superset"):
        assert part in names, part
    assert P.as_b(MLS, [P.SEG])[0] == [] and P.as_b(MPG, [P.SQ4])[0] == []  # rows with empty members


@pytest.mark.parametrize("offset,scale", P.PLACEMENTS, ids=["utm", "web-mercator", "tiny", "huge"])
def test_placement_does_not_change_the_reference(offset, scale):
    for ka, kb in ((MPT, MPT), (MPT, MLS), (MPT, MPG)):
        a, b, want, _ = P.case_columns(P.TIES, ka, kb)
        got = P.masks(ka, [P.placed(ka, r, offset, scale) for r in a], kb, [P.placed(kb, r, offset, scale) for r in b])
        assert np.array_equal(got, want)


def test_a_point_against_a_line_is_the_line_relation_of_a_degenerate_line():
    """mask(p, line) against linerel_ref.mask with the point written as the LINESTRING [p, p]: II -> 1, an interior point of A on B's
    boundary -> 2, A off B -> 4, B off A -> 8; a point has no boundary, so the BND bits never occur"""
    checked = 0
    for kb in (LS, MLS):
        A, B, want = P.random_columns(PT, kb)
        cases = P.case_columns(P.TIES, PT, kb)
        for p, b, m in list(zip(A, B, want)) + list(zip(cases[0], cases[1], cases[2])):
            ll = L.mask(LS, [p, p], kb, b)
            assert not ll & (L.SHARED_PIECE | L.BND_INT | L.BND_BND)
            mapped = (1 if ll & L.INTERIORS else 0) | (2 if ll & L.INT_BND else 0) | (4 if ll & L.A_OUTSIDE else 0) | (8 if ll & L.B_OUTSIDE else 0)
            assert mapped == m, (p, b, ll, m)
            checked += 1
    assert checked > 200


def test_a_point_against_a_polygon_is_the_line_polygon_relation_of_a_degenerate_line():
    """relation_ref.mask of the LINESTRING [p, p] is the position of p: the bits 1, 2, 4 of the point mask"""
    checked = 0
    for kb in (PG, MPG):
        A, B, want = P.random_columns(PT, kb)
        cases = P.case_columns(P.TIES, PT, kb)
        for p, b, m in list(zip(A, B, want)) + list(zip(cases[0], cases[1], cases[2])):
            assert R.mask(LS, [p, p], kb, b) == (m & 7) and m & 8, (p, b, m)
            checked += 1
    assert checked > 200


def test_two_punctual_rows_swap_the_bits_4_and_8():
    for ka, kb in ((PT, PT), (PT, MPT), (MPT, PT), (MPT, MPT)):
        A, B, want = P.random_columns(ka, kb)
        assert np.array_equal(P.masks(kb, B, ka, A), P.swapped(want))
    assert P.swapped([1, 5, 9, 12, 13]).tolist() == [1, 9, 5, 12, 13]


def _subsets(points, most):
    for k in range(1, most + 1):
        yield from (list(c) for c in itertools.combinations(points, k))


def test_the_masks_that_can_occur():
    """by brute force over a small lattice: exactly 1, 5, 9, 12, 13 for a punctual B; 9 .. 15 for a polygonal B; 9 .. 15 for a lineal
    B, and for rows all of whose members are degenerate additionally 1 and 5"""
    grid = [(x, y) for x in range(3) for y in range(3)]
    seen = {P.mask(MPT, a, MPT, b) for a in _subsets(grid[:5], 3) for b in _subsets(grid[:5], 3)}
    assert seen == set(P.REACHABLE[0]) == {1, 5, 9, 12, 13}
    lines = [[p, q] for p in grid[:6] for q in grid[:6]] + [[(0, 0), (2, 0), (2, 2)], [(0, 0), (2, 0), (2, 2), (0, 0)], [(1, 1)]]
    rows = [[m] for m in lines] + [[[(0, 0), (1, 1)], [(1, 1), (2, 0)]], [[(1, 1)], [(2, 2), (2, 2)]], [[(0, 0), (1, 1)], [(1, 1), (2, 0)], [(1, 1), (1, 2)]]]
    proper, degenerate = set(), set()
    for b in rows:
        all_degenerate = all(len(set(m)) == 1 for m in b)
        for a in _subsets(grid, 3):
            (degenerate if all_degenerate else proper).add(P.mask(MPT, a, MLS, b))
    assert proper == set(range(9, 16)) and degenerate == {1, 5, 9, 12, 13} and proper | degenerate == set(P.REACHABLE[1])
    polys = [[P.sq(0, 0, 2, 2)], [[(0, 0), (2, 0), (0, 2), (0, 0)]]]
    seen = {P.mask(MPT, a, PG, b) for b in polys for a in _subsets(grid + [(3, 3)], 3)}
    assert seen == set(P.REACHABLE[2]) == set(range(9, 16))
    # one point has one of the bits 1, 2, 4
    for ka, kb in P.FAMILIES:
        assert set(P.reachable(ka, kb)) <= set(P.REACHABLE[P.DIM[kb]])
        if ka == PT:
            assert all(bin(m & 7).count("1") == 1 for m in P.reachable(ka, kb))


@pytest.mark.parametrize("ka,kb", P.FAMILIES, ids=FAMILY_IDS)
def test_the_random_columns_are_honest(ka, kb):
    """every mask the pair of kinds can have occurs in at least 3 of the 96 rows and none fills more than half of them; no row is
    unusable; the generator is deterministic"""
    A, B, want = P.random_columns(ka, kb)
    assert len(A) == len(B) == len(want) == 96 and want.all()
    values, counts = np.unique(want, return_counts=True)
    assert set(values.tolist()) == set(P.reachable(ka, kb)), values
    assert counts.min() >= 3 and counts.max() <= 48, dict(zip(values.tolist(), counts.tolist()))
    assert P.honest(ka, kb, want) and not P.honest(ka, kb, np.full(96, want[0]))
    assert np.array_equal(P.masks(ka, A, kb, B), want)
    assert np.array_equal(P.masks(ka, [P.padded(ka, r, 40) for r in A], kb, [P.padded(kb, r, 40) for r in B]), want)


def test_join_fixture_and_expected_pairs():
    A, av, B, bv, table, self_table = P.join_fixture(MPT, MLS)
    assert table.shape == (300, 300) and not table[23].any() and not table[31].any() and not table[:, 40].any() and not table[:, 52].any()
    assert set(np.unique(table).tolist()) >= {0, 9, 10, 12, 13}
    for pred in P.PRED_IDS:
        pairs, counts, masks = P.expected_pairs(table, pred, 1)
        assert counts.sum() == len(pairs) == len(masks) and all(P.PREDICATES[pred](int(m), 1) for m in masks)
        t_pairs, _, t_masks = P.expected_pairs(table, pred, 1, transpose=True)
        name = P.TRANSPOSED.get(pred, pred)
        assert all(P.PREDICATES[name](int(m), 1) for m in t_masks) and np.all(t_pairs[:-1, 0] <= t_pairs[1:, 0])
    assert len(P.expected_pairs(table, "overlaps", 1)[0]) == 0 and len(P.expected_pairs(table, "touches", 1)[0]) > 10
    diag = np.nonzero(self_table.diagonal())[0]
    assert len(diag) == 298 and (self_table.diagonal()[diag] == 1).all()
    assert (self_table == 1).sum() > 298 + 10  # duplicates beyond the diagonal
