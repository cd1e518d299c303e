"""The exact line x polygon reference (tests/relation_ref.py) pinned on hand-made answers, and its fixtures checked: every fixture
polygon is valid by the reference's own check, the random columns reach every mask value, the padded and placed forms keep their
answers.  CPU only."""
import numpy as np
import pytest

from tests import relation_ref as R

LS, MLS, PG, MPG = R.LS, R.MLS, R.PG, R.MPG


@pytest.mark.parametrize("name,line,want", R.KNOWN, ids=[k[0] for k in R.KNOWN])
def test_known_answer(name, line, want):
    assert R.mask(LS, line, PG, R.DONUT) == want
    assert R.mask(MLS, [[], line], MPG, [[], R.DONUT, [R.sq(40, 40, 44, 44)]]) == want
    assert R.mask(LS, line[::-1], PG, [r[::-1] for r in R.DONUT]) == want  # neither direction nor ring orientation matters


def test_known_answers_cover_every_mask_value():
    assert {k[2] for k in R.KNOWN} | {R.KNOWN_MULTI[2]} == {1, 2, 3, 4, 5, 6, 7}
    assert R.mask(MLS, R.KNOWN_MULTI[1], PG, R.DONUT) == 5
    for kl, kp in R.FAMILIES:
        lines, polys, want = R.known_columns(kl, kp)
        assert np.array_equal(R.masks(kl, lines, kp, polys), want)


@pytest.mark.parametrize("tie", R.TIES, ids=[t[0] for t in R.TIES])
def test_ring_touch_answer(tie):
    _, kp, poly, line, want = tie
    assert R.polygon_valid(kp, poly)
    assert R.mask(LS, line, kp, poly) == want
    assert R.mask(LS, line[::-1], kp, poly) == want
    assert R.mask(LS, R.scaled_line(LS, line, 7), kp, R.padded(kp, poly, 7)) == want


def test_row_rules():
    nan = float("nan")
    inside = [(1, 1), (3, 2)]
    assert R.mask(LS, inside, PG, R.DONUT) == 1
    assert R.mask(LS, [], PG, R.DONUT) == 0 and R.mask(MLS, [[], []], PG, R.DONUT) == 0
    assert R.mask(LS, [(1, 1), (nan, 0)], PG, R.DONUT) == 0
    assert R.mask(LS, inside, PG, []) == 0 and R.mask(LS, inside, MPG, [[], []]) == 0
    assert R.mask(LS, inside, PG, R.DONUT, line_valid=False) == 0 and R.mask(LS, inside, PG, R.DONUT, poly_valid=False) == 0
    assert R.mask(LS, inside, PG, [R.DONUT[0][:-1]]) == 0  # an unclosed ring
    assert R.mask(LS, inside, PG, [R.DONUT[0], [(4, 4), (8, 4), (4, 4)]]) == 0  # a hole of three coordinates
    assert R.mask(LS, inside, PG, [[(0, 0), (5, 0), (9, 0), (0, 0)]]) == 0  # no turning vertex
    assert R.mask(LS, inside, PG, [R.DONUT[0], []]) == 1  # an empty hole is skipped
    assert np.array_equal(R.masks(LS, [inside] * 3, PG, [R.DONUT], rows=[0, 1, 7]), [1, 0, 0])


def test_validity_check_refuses_invalid_polygons():
    assert R.polygon_valid(PG, R.DONUT)
    assert not R.polygon_valid(PG, [[(0, 0), (4, 4), (4, 0), (0, 4), (0, 0)]])  # a bow tie
    assert not R.polygon_valid(PG, [R.sq(0, 0, 12, 12), R.sq(10, 10, 14, 14)])  # a hole poking out
    assert not R.polygon_valid(PG, [R.sq(0, 0, 12, 12), R.sq(20, 20, 22, 22)])  # a hole outside
    assert not R.polygon_valid(PG, [R.sq(0, 0, 12, 12), R.sq(2, 2, 6, 6), R.sq(4, 4, 8, 8)])  # overlapping holes
    assert not R.polygon_valid(PG, [R.sq(0, 0, 12, 12), R.sq(0, 2, 4, 6)])  # a hole sharing a stretch of the shell
    assert not R.polygon_valid(MPG, [[R.sq(0, 0, 12, 12)], [R.sq(6, 6, 20, 20)]])  # overlapping members
    assert not R.polygon_valid(PG, [[(0, 0), (4, 0), (2, 0), (2, 3), (0, 0)]])  # a ring folding back on itself


@pytest.mark.parametrize("kl,kp", R.FAMILIES, ids=[f"{R.NAMES[a]}-{R.NAMES[b]}" for a, b in R.FAMILIES])
def test_random_fixture_polygons_are_valid(kl, kp):
    lines, polys, masks = R.random_columns(kl, kp)
    assert all(R.polygon_valid(kp, p) for p in polys)
    n_l = [sum(len(s) for s in R.line_seqs(kl, r)) for r in lines]
    n_p = [sum(len(r) for p in R.row_polys(kp, row) for r in p) for row in polys]
    assert min(n_l) >= 2 and max(n_l) >= 40 and min(n_p) >= 4 and max(n_p) >= 60
    assert (masks != 0).all()


def test_random_fixtures_reach_every_mask_value():
    counts = sum(np.bincount(R.random_columns(kl, kp)[2], minlength=8) for kl, kp in R.FAMILIES)
    assert counts[0] == 0 and (counts[1:] >= 5).all(), counts
    assert sum(len(R.random_columns(kl, kp)[0]) for kl, kp in R.FAMILIES) >= 300


def test_padding_and_placement_keep_the_figure():
    lines, polys, masks = R.random_columns(LS, PG)
    for i in range(0, len(lines), 7):
        assert R.mask(LS, R.scaled_line(LS, lines[i], 1), PG, R.padded(PG, polys[i], 1)) == masks[i]
    ring = R.pad_ring(R.sq(0, 0, 2, 3), 2)
    assert len(ring) == 13 and ring[0] == ring[-1] == (0, 0) and ring[1] == (2, 0) and ring[3] == (6, 0)
    assert R.placed(LS, [(1, 2)], (10, 20), 0.5) == [(5.5, 11.0)]
    for offset, scale in R.PLACEMENTS:  # exact in doubles: translate, then scale by a power of two
        x = (40 + offset[0]) * scale
        assert float(x) == x and np.log2(scale) == int(np.log2(scale)) and abs(x) < 2.0**63


def test_join_fixture_and_expected_pairs():
    lines, lv, polys, pv, table = R.join_fixture()
    assert table.shape == (300, 300)
    assert all(R.polygon_valid(PG, p) for j, p in enumerate(polys) if len(p))
    assert not table[23].any() and not table[31].any() and not table[:, 40].any() and not table[:, 52].any()
    assert (table[:, 17] != 0).sum() >= 295  # the polygon over the whole domain
    counts = np.bincount(table.ravel(), minlength=8)
    assert (counts[[1, 2, 3, 4, 6, 7]] >= 5).all(), counts
    # the shortcut for far pairs against the full machinery on a sample
    for i in range(0, 300, 37):
        for j in range(0, 300, 41):
            assert table[i, j] == R.mask(LS, lines[i], PG, polys[j], lv[i], pv[j])
    pairs, cnt, masks = R.expected_pairs(table, "intersects")
    assert len(pairs) == ((table & 3) != 0).sum() == cnt.sum() and (masks & 3).all()
    assert np.array_equal(pairs, pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))])
    tp, tc, tm = R.expected_pairs(table, "intersects", transpose=True)
    assert {(int(a), int(b)) for a, b in pairs} == {(int(b), int(a)) for a, b in tp} and len(tc) == 300
