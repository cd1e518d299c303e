"""The exact reference of the polygon x polygon relation mask (tests/polyrel_ref.py) against hand-written answers, its own symmetries,
and a second derivation — the combination csrc/gpk_polyrel.h uses (the rings of one geometry walked as lines against the other, both
ways, plus the side of shared boundary pieces), evaluated on rationals — so that the kernel's argument is checked before any GPU runs."""
from fractions import Fraction

import numpy as np
import pytest

from tests import exact_predicates as E
from tests import polyrel_ref as P
from tests import relation_ref as R

PG, MPG = P.PG, P.MPG
CASES = P.KNOWN + P.TIES


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_written_answers(case):
    _, a, b, want = case
    assert P.mask(MPG, a, MPG, b) == want
    assert P.mask(MPG, b, MPG, a) == int(P.swapped(want))
    assert P.mask_by_walks(MPG, a, MPG, b) == want
    if len(a) == 1 and len(b) == 1:
        assert P.mask(PG, a[0], PG, b[0]) == want


def test_the_cases_cover_every_reachable_mask_and_the_predicate_table():
    assert {c[3] for c in CASES} == set(P.REACHABLE)
    for m in range(16):
        assert int(P.swapped(m)) == (m & 3) | (4 if m & 8 else 0) | (8 if m & 4 else 0)
        assert P.PREDICATES["within"](m) == P.PREDICATES["contains"](int(P.swapped(m)))
        assert P.PREDICATES["equals"](m) == (P.PREDICATES["within"](m) and P.PREDICATES["contains"](m))
        assert P.PREDICATES["touches"](m) == (P.PREDICATES["intersects"](m) and not (m & 1))
    named = {m: [n for n in ("equals", "touches", "overlaps", "disjoint") if P.PREDICATES[n](m)] for m in P.REACHABLE}
    assert named == {3: ["equals"], 5: [], 7: [], 9: [], 11: [], 12: ["disjoint"], 13: ["overlaps"], 14: ["touches"], 15: ["overlaps"]}


def test_every_fixture_row_is_a_valid_polygon():
    n = 0
    for kind, row in P.all_fixture_rows():
        assert R.polygon_valid(kind, row), (kind, row)
        n += 1
    assert n > 1500


def test_sample_points_agree_with_the_rational_point_location():
    """the even-odd count along a slab's middle line is the position exact_predicates gives the same sample point"""
    for _, a, b, _ in CASES:
        pa, pb = P.usable(MPG, a), P.usable(MPG, b)
        _, samples = P.area_samples(E._edges([r for p in pa for r in p]), E._edges([r for p in pb for r in p]))
        assert samples
        pts = [(Fraction(x), Fraction(y)) for x, y, _, _ in samples]
        for polys, k in ((pa, 2), (pb, 3)):
            pos = np.stack([E._rational_pos(pts, rings) for rings in polys], axis=1)
            assert not (pos == E.BOUNDARY).any()
            assert np.array_equal((pos == E.INSIDE).any(axis=1), np.array([s[k] for s in samples]))


@pytest.mark.parametrize("ka,kb", P.FAMILIES, ids=[f"{P.NAMES[a]}-{P.NAMES[b]}" for a, b in P.FAMILIES])
def test_random_columns(ka, kb):
    A, B, want = P.random_columns(ka, kb)
    assert set(want.tolist()) <= set(P.REACHABLE) and len(set(want.tolist())) >= 6
    assert np.array_equal(P.masks(kb, B, ka, A), P.swapped(want))
    got = np.array([P.mask_by_walks(ka, a, kb, b) for a, b in zip(A, B)], dtype=np.uint8)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (bad[:5], got[bad[:5]], want[bad[:5]])


def test_padding_keeps_the_answers():
    for cases in (P.KNOWN, P.TIES):
        a, b, want, _ = P.case_columns(cases, MPG, MPG, pad=2)
        assert np.array_equal(P.masks(MPG, a, MPG, b), want)


def test_unusable_rows():
    sq = P.S10
    open_ring = [(0, 0), (12, 0), (12, 12), (0, 12)]
    assert P.mask(PG, [sq], PG, [sq]) == 3
    for bad in ([], [open_ring], [[(0, 0), (5, 0), (0, 0)]], [sq, [(4, 4), (8, 4), (4, 4)]], [[(0, 0), (float("nan"), 1), (3, 3), (0, 0)]]):
        assert P.mask(PG, bad, PG, [sq]) == 0 and P.mask(PG, [sq], PG, bad) == 0
    assert P.mask(PG, [sq], PG, [sq], a_valid=False) == 0 and P.mask(PG, [sq], PG, [sq], b_valid=False) == 0
    assert P.mask(MPG, [[], [sq]], MPG, [[sq], []]) == 3 and P.mask(MPG, [[]], MPG, [[sq]]) == 0
    assert P.mask(MPG, [[sq], [open_ring]], PG, [sq]) == 0


def test_join_fixture_holds_every_predicate():
    left, lv, right, rv, table, self_table = P.join_fixture(PG, PG)
    assert table.shape == (300, 300) and set(np.unique(table).tolist()) <= {0, *P.REACHABLE}
    for pred in P.PRED_IDS:
        pairs, counts, m = P.expected_pairs(table, pred)
        assert len(pairs) >= 5 and counts.sum() == len(pairs), pred
    assert not table[31].any() and not table[23].any() and not table[:, 52].any() and not table[:, 40].any()
    assert np.array_equal(self_table, P.swapped(self_table).T)
    ok = np.nonzero(self_table.diagonal())[0]
    assert len(ok) == 298 and (self_table.diagonal()[ok] == 3).all()
    assert len(P.expected_pairs(self_table, "touches")[0]) >= 2 * 60  # the tiles' shared edges, both orders
