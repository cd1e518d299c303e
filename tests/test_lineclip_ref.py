"""The exact reference of the line clip (tests/lineclip_ref.py) checked against itself and against the references it stands on: the
fixture regenerates byte for byte, INSIDE and OUTSIDE partition every segment, the kept length is overlay_ref.exact_length, and the
parts agree with relation_ref's mask.  No device."""
from fractions import Fraction

import numpy as np
import pytest

from tests import lineclip_ref as L
from tests import overlay_ref as O
from tests import relation_ref as R


def test_fixture_regenerates_byte_for_byte():
    assert L.fixture_bytes() == open(L.GOLDEN, "rb").read()
    assert len(open(L.GOLDEN, "rb").read()) < 200 * 1024


@pytest.mark.parametrize("kl,kp", L.FAMILIES)
def test_hand_cases_have_the_stated_parts(kl, kp):
    lines, polys, lv, pv, names = L.rows(kl, kp)
    want = L.hand_expectations(kl, kp)
    assert len(want) >= 18
    for i, (n_in, n_out) in want.items():
        got = tuple(len(L.clip(kl, lines[i], kp, polys[i], mode)[0]) for mode in (L.INSIDE, L.OUTSIDE))
        assert got == (n_in, n_out), (names[i], got)
    for name in ("a null line", "a null polygon", "an empty line", "an empty polygon"):
        i = names.index(name)
        assert L.clip(kl, lines[i], kp, polys[i], L.INSIDE, bool(lv[i]), bool(pv[i])) is None


def test_three_inside_parts_from_one_segment_with_their_coordinates():
    parts, crossings, gap = L.clip(L.LS, [(-2, 6), (22, 6)], L.PG, L.TWO_WINDOWS, L.INSIDE)
    assert [[t for t, _ in p] for p in parts] == [[L.TAG_X, L.TAG_X]] * 3
    assert [(c[0], c[1]) for c in crossings] == [(x, 6) for x in (0, 4, 8, 12, 16, 20)] and gap == Fraction(4, 24)
    parts, _, _ = L.clip(L.LS, [(-2, -2), (3, 3)], L.PG, [L.S10], L.OUTSIDE)
    assert parts == [[(L.TAG_L, 0), (L.TAG_P, 0)]]  # through the ring vertex (0, 0): the polygon's own coordinate


@pytest.mark.parametrize("kl,kp", L.FAMILIES)
def test_modes_partition_every_segment_and_sum_to_the_exact_length(kl, kp):
    """per non-degenerate segment the kept shares of INSIDE and OUTSIDE add up to exactly 1; the sum of |pq| * share(INSIDE) is
    overlay_ref.exact_length; OUTSIDE has a part <=> mask & EXTERIOR, and mask & INTERIOR => INSIDE has a part"""
    import mpmath as mp

    lines, polys, lv, pv, names = L.rows(kl, kp)
    for i, (a, b) in enumerate(zip(lines, polys)):
        pieces = L.analyse(kl, a, kp, b, bool(lv[i]), bool(pv[i]))
        exact = O.exact_length(kl, a, kp, b, bool(lv[i]), bool(pv[i]))
        assert (pieces is None) == (exact is None), names[i]
        if pieces is None:
            continue
        m_in, m_out = L.measures(pieces, L.INSIDE), L.measures(pieces, L.OUTSIDE)
        assert all(x[2] + y[2] == 1 for x, y in zip(m_in, m_out)), names[i]
        with mp.workdps(40):
            total = mp.mpf(0)
            for p, q, share in m_in:
                total += mp.sqrt((q[0] - p[0]) ** 2 + (q[1] - p[1]) ** 2) * share.numerator / share.denominator
            assert abs(total - exact) <= mp.mpf(10) ** -30 * (1 + abs(exact)), names[i]
        mask = R.mask(kl, a, kp, b, bool(lv[i]), bool(pv[i]))
        n_in, n_out = (len(L.clip(kl, a, kp, b, mode, pieces=pieces)[0]) for mode in (L.INSIDE, L.OUTSIDE))
        if all(len({tuple(c) for c in s}) > 1 for s in R.line_seqs(kl, a) if len(s)):  # non-degenerate: every sequence has a segment
            assert (n_out > 0) == bool(mask & R.EXTERIOR), (names[i], mask, n_out)
            if mask & R.INTERIOR:
                assert n_in > 0, names[i]
        if not m_in:
            assert n_in == 0 and n_out == 0


def test_fixture_rows_keep_the_gap_condition_and_every_part_has_two_coordinates():
    z = np.load(L.GOLDEN)
    for kl, kp in L.FAMILIES:
        for mode in L.MODES.values():
            key = L.fixture_key(kl, kp) + mode + "_"
            assert (np.diff(z[key + "part_offsets"]) >= 2).all()
            assert z[key + "geom_offsets"][-1] == len(z[key + "part_offsets"]) - 1 and z[key + "part_offsets"][-1] == len(z[key + "xy"])
            assert (z[key + "tag"] == L.TAG_X).sum() == len(z[key + "cross"]) > 100
