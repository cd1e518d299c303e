"""CPU: the exact reference of the line x line relation mask (tests/linerel_ref.py) held against independent answers: the hand-derived
cases, the kernel's formulation restated in plain Python, the exact distance reference, the argument swap and validity_ref.is_simple."""
from fractions import Fraction

import numpy as np
import pytest

from tests import linerel_ref as L
from tests import pair_distance_ref as D
from tests import validity_ref as V

LS, MLS = L.LS, L.MLS
FAMILY_IDS = [f"{L.NAMES[a]}-{L.NAMES[b]}" for a, b in L.FAMILIES]


@pytest.mark.parametrize("cases", [L.KNOWN, L.TIES], ids=["known", "ties"])
def test_hand_answers(cases):
    for name, a, b, want in cases:
        assert L.mask(MLS, a, MLS, b) == want, name
        assert L.mask_by_rules(MLS, a, MLS, b) == want, name
        assert L.mask(MLS, b, MLS, a) == int(L.swapped(want)), name
    for pad in (0, 3):
        for ka, kb in L.FAMILIES:
            ra, rb, want, names = L.case_columns(cases, ka, kb, pad)
            assert len(ra) >= 5 and np.array_equal(L.masks(ka, ra, kb, rb), want), (ka, kb, pad)


def test_predicates_of_the_hand_cases():
    by_name = {c[0]: c[3] for c in L.KNOWN + L.TIES}
    expect = {"an X": "crosses", "end on end": "touches", "T-junction": "touches", "the same line": "equals", "a stretch of B": "within",
              "partial overlap": "overlaps", "apart": "disjoint", "reversed, with extra collinear vertices": "equals",
              "covered by two members that abut": "within", "covered except for a gap": "overlaps", "point member inside B": "within",
              "an end of another member at the crossing": "touches", "two members meet (even)": "crosses"}
    for name, pred in expect.items():
        assert L.PREDICATES[pred](by_name[name]), (name, pred)
    m = by_name["point member (equal coordinates) on B's end"]
    assert L.PREDICATES["covered_by"](m) and not L.PREDICATES["within"](m) and L.PREDICATES["touches"](m)
    assert not any(f(0) for f in L.PREDICATES.values())


@pytest.mark.parametrize("ka,kb", L.FAMILIES, ids=FAMILY_IDS)
def test_kernel_formulation_agrees_with_the_arrangement(ka, kb):
    A, B, want = L.random_columns(ka, kb)
    got = np.array([L.mask_by_rules(ka, a, kb, b) for a, b in zip(A, B)], dtype=np.uint8)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    assert (want != 0).all() and ((want & 2 == 0) | (want & 1 == 1)).all()  # usable pairs; SHARED_PIECE comes with INTERIORS


@pytest.mark.parametrize("ka,kb", L.FAMILIES, ids=FAMILY_IDS)
def test_intersects_is_distance_zero_and_swap(ka, kb):
    A, B, want = L.random_columns(ka, kb)
    for a, b, m in zip(A, B, want):
        assert bool(m & 31) == (D.distance2(ka, a, kb, b) == Fraction(0))
    assert np.array_equal(L.masks(kb, B, ka, A), L.swapped(want))


@pytest.mark.parametrize("ka,kb", [(LS, LS), (MLS, MLS)], ids=["ls-ls", "mls-mls"])
def test_random_columns_reach_every_bit_and_predicate(ka, kb):
    _, _, want = L.random_columns(ka, kb)
    for bit in (1, 2, 4, 8, 16):
        assert int(np.count_nonzero(want & bit)) >= 5, bit
    for pred in ("crosses", "touches", "overlaps", "within", "equals"):
        assert sum(L.PREDICATES[pred](int(m)) for m in want) >= 5, pred
    assert sum(L.PREDICATES["disjoint"](int(m)) for m in want) <= len(want) // 2


def test_simple_multilinestrings_share_no_interior_point_between_members():
    """a MULTILINESTRING of two members that is_simple accepts: its members meet at ends of both only, so no INTERIORS bit"""
    A, B, _ = L.random_columns(LS, LS)
    seen = 0
    for a, b in zip(A, B):
        if V.is_simple(MLS, [a, b]):
            seen += 1
            assert not L.mask(LS, a, LS, b) & L.INTERIORS
    assert seen >= 10


def test_join_fixture_has_every_predicate():
    left, lv, right, rv, table, self_table = L.join_fixture(LS, LS)
    assert table.shape == (300, 300) and not table[23].any() and not table[31].any() and not table[:, 40].any() and not table[:, 52].any()
    for pred in L.PRED_IDS:
        assert len(L.expected_pairs(table, pred)[0]) > 0, pred
    assert len(L.expected_pairs(table, "intersects")[0]) > 300
    usable = np.nonzero(self_table.diagonal())[0]
    assert all(L.PREDICATES["equals"](int(self_table[i, i])) for i in usable)
    assert np.array_equal(self_table.T, L.swapped(self_table))


def test_zigzag_rows():
    a, b = L.zigzag_pair()
    assert len(a) == 600 and len(b) == 300
    m = L.mask(LS, a, LS, b)
    assert m == 117  # the kept vertices and every second segment's... shared stretches: II, IB, BB; both stick out
