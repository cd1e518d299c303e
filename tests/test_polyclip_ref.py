"""The exact reference of the polygon clip (tests/polyclip_ref.py) and its fixture, pinned by identities the reference shares no code
with: the exact area of the intersection is overlay_ref.exact_area (an independent derivation of the shared area), the area of the
difference is area(a) minus that, and sampled rational points lie in the result exactly when exact_predicates places them in both
interiors (or in a's and not in closed b).  The hand cases carry their part and ring counts stated by hand."""
from fractions import Fraction

import numpy as np
import pytest

from tests import overlay_ref as O
from tests import polyclip_ref as L
from tests import relation_ref as R

FAMILY_IDS = [f"{L.NAMES[a]}-{L.NAMES[b]}" for a, b in L.FAMILIES]


def test_regeneration_reproduces_the_committed_fixture():
    """tests/golden/make_polyclip_golden.py is deterministic, array for array (the container's bytes depend on the zlib at hand)"""
    z, fresh = np.load(L.GOLDEN), L.build_arrays()
    assert sorted(z.files) == sorted(fresh)
    for k, v in fresh.items():
        assert z[k].dtype == v.dtype and z[k].shape == v.shape and z[k].tobytes() == v.tobytes(), k


@pytest.mark.parametrize("ka,kb", L.FAMILIES, ids=FAMILY_IDS)
def test_hand_cases_have_the_counts_stated_by_hand(ka, kb):
    A, B, av, bv, names = L.rows(ka, kb)
    want = L.hand_expectations(ka, kb)
    assert len(want) >= 17
    for i, (wi, wd) in want.items():
        got = []
        for mode in (L.INTERSECTION, L.DIFFERENCE):
            parts, status, gap = L.clip(ka, A[i], kb, B[i], mode)
            got.append((len(parts), sum(len(p) for p in parts)))
            assert status == (L.ST_EMPTY if not parts else status) and (gap is None or gap >= L.MIN_GAP)
        assert tuple(got) == (wi, wd), (names[i], got, wi, wd)
    for name in ("a null a", "a null b", "an empty a", "an empty b", "an invalid ring in a", "an invalid ring in b"):
        i = names.index(name)
        assert L.clip(ka, A[i], kb, B[i], L.INTERSECTION, bool(av[i]), bool(bv[i]))[:2] == (None, L.ST_NULL), name


def test_the_named_shapes():
    sq, S10 = L.sq, L.S10
    parts, st, _ = L.clip(L.PG, [S10], L.PG, [[(10, 0), (10, 10), (0, 10), (0, 0), (10, 0)]], L.INTERSECTION)
    assert st == L.ST_OK and parts == [[[(Fraction(x), Fraction(y)) for x, y in S10]]]  # equal polygons intersect to a, from a's start
    parts, st, _ = L.clip(L.PG, [S10], L.PG, [[(5, 0), (8, 4), (2, 4), (5, 0)]], L.DIFFERENCE)
    assert st == L.ST_TOUCH and len(parts) == 1 and len(parts[0]) == 1 and parts[0][0][:-1].count((5, 0)) == 2  # the hole fused into the shell
    parts, st, _ = L.clip(L.PG, [S10], L.PG, [L.APEX], L.DIFFERENCE)
    assert st == L.ST_OK and len(parts) == 2 and all((5, 10) in p[0] for p in parts)  # two rings that touch at the apex
    parts, st, _ = L.clip(L.PG, [L.THIN_A], L.PG, [L.THIN_B], L.INTERSECTION)
    ra, rb = L.row_rings(L.PG, [L.THIN_A]), L.row_rings(L.PG, [L.THIN_B])
    assert [L.tag_point(pt, ra, rb)[0] for pt in parts[0][0]] == [L.TAG_X] * 5  # all four vertices computed (and the closing one)
    parts, st, _ = L.clip(L.PG, [sq(0, 0, 10, 10, cw=True)], L.PG, [sq(5, 5, 15, 15)], L.INTERSECTION)
    assert L.area_of(parts) == 25 and parts[0][0][0] == (10, 5)  # walked backwards: the first crossing met is the one on x = 10


@pytest.mark.parametrize("ka,kb", L.FAMILIES, ids=FAMILY_IDS)
def test_areas_match_the_independent_exact_area(ka, kb):
    A, B, av, bv, _names = L.rows(ka, kb)
    n = 0
    for i, (a, b) in enumerate(zip(A, B)):
        shared = O.exact_area(ka, a, kb, b, bool(av[i]), bool(bv[i]))
        inter, diff = L.clip(ka, a, kb, b, L.INTERSECTION, bool(av[i]), bool(bv[i]))[0], L.clip(ka, a, kb, b, L.DIFFERENCE, bool(av[i]), bool(bv[i]))[0]
        assert (shared is None) == (inter is None) == (diff is None)
        if shared is None:
            continue
        n += 1
        assert L.area_of(inter) == shared, i
        assert L.area_of(diff) == L.row_area(ka, a) - shared, i
        for parts in (inter, diff):  # shells counter-clockwise, holes clockwise, rings closed
            for p in parts:
                assert L._shoelace2(p[0]) > 0 and all(L._shoelace2(h) < 0 for h in p[1:]) and all(r[0] == r[-1] for r in p)
    assert n > 100


def _in_result(pt, parts):
    """+1 inside, 0 on a ring, -1 outside the parts of a result"""
    pos = [[L.ring_position(pt, r) for r in p] for p in parts]
    if any(v == 0 for p in pos for v in p):
        return 0
    return 1 if any(p[0] > 0 and all(h < 0 for h in p[1:]) for p in pos) else -1


@pytest.mark.parametrize("ka,kb", L.FAMILIES, ids=FAMILY_IDS)
def test_point_membership_of_sampled_rational_points(ka, kb):
    """rational points over the pair's box (none of them on a lattice line): in the intersection iff INTERIOR to both rows by
    relation_ref._positions, in the difference iff INTERIOR to a and EXTERIOR to b"""
    from tests import polyrel_ref as P

    A, B, av, bv, _names = L.rows(ka, kb)
    rng = np.random.default_rng(17)
    checked = 0
    for i, (a, b) in enumerate(zip(A, B)):
        pa, pb = P.usable(ka, a, bool(av[i])), P.usable(kb, b, bool(bv[i]))
        if pa is None or pb is None:
            continue
        inter, diff = L.clip(ka, a, kb, b, L.INTERSECTION)[0], L.clip(ka, a, kb, b, L.DIFFERENCE)[0]
        both = np.concatenate([r for p in pa + pb for r in p])
        lo, hi = both.min(axis=0), both.max(axis=0)
        pts = [(Fraction(int(rng.integers(lo[0] - 1, hi[0] + 1))) + Fraction(int(rng.integers(1, 7)), 7),
                Fraction(int(rng.integers(lo[1] - 1, hi[1] + 1))) + Fraction(int(rng.integers(1, 11)), 11)) for _ in range(12)]
        in_a, in_b = R._positions(pts, pa), R._positions(pts, pb)
        for pt, wa, wb in zip(pts, in_a, in_b):
            if wa == R.BOUNDARY or wb == R.BOUNDARY:
                continue
            checked += 1
            assert (_in_result(pt, inter) > 0) == (wa == R.INTERIOR and wb == R.INTERIOR), (i, pt)
            assert (_in_result(pt, diff) > 0) == (wa == R.INTERIOR and wb == R.EXTERIOR), (i, pt)
    assert checked > 1000
