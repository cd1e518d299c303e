"""The exact reference of the polygon symmetric difference (tests/polysymdiff_ref.py) and its fixture, pinned by identities the
reference shares no code with: the exact area of the result is area(a) + area(b) minus twice overlay_ref.exact_area of the pair, and
one rational sample point strictly inside every face of the arrangement of the two rows' edges lies in the result exactly when crossing
numbers place it in the interior of exactly one row.  The hand cases carry their parts, rings, coordinates per ring and status stated
by hand; the result for (b, a) has the rings of the result for (a, b)."""
import os

import numpy as np
import pytest

from tests import overlay_ref as O
from tests import polyclip_ref as L
from tests import polysymdiff_ref as S

FAMILY_IDS = [f"{S.NAMES[a]}-{S.NAMES[b]}" for a, b in S.FAMILIES]


def test_regeneration_reproduces_the_committed_fixture():
    """the fixture is deterministic: array for array first (the message names the array that moved), then the committed bytes are
    fixture_bytes(); its input rows after the hand cases are those of polyunion_lattice.npz; it stays at the size of its siblings"""
    from tests.golden import make_polysymdiff_golden as G

    G.check_union_rows()
    z, fresh = np.load(S.GOLDEN), S.build_arrays()
    assert sorted(z.files) == sorted(fresh)
    for k, v in fresh.items():
        assert z[k].dtype == v.dtype and z[k].shape == v.shape and z[k].tobytes() == v.tobytes(), k
    assert open(S.GOLDEN, "rb").read() == S.fixture_bytes()
    assert os.path.getsize(S.GOLDEN) <= 2 * os.path.getsize(L.GOLDEN)


def test_no_fixture_row_is_unresolved_and_every_row_clears_the_gap():
    z = np.load(S.GOLDEN)
    for ka, kb in S.FAMILIES:
        status = z[S.fixture_key(ka, kb) + S.MODES[S.SYMDIFF] + "_status"]
        assert (status != S.ST_UNRESOLVED).all() and len(status) == len(S.rows(ka, kb)[0])
        assert all(gap is None or gap >= S.MIN_GAP for _parts, _st, gap in S.results(ka, kb))


@pytest.mark.parametrize("ka,kb", S.FAMILIES, ids=FAMILY_IDS)
def test_hand_cases_have_the_structure_stated_by_hand(ka, kb):
    A, B, av, bv, names = S.rows(ka, kb)
    want = S.hand_expectations(ka, kb)
    assert len(want) >= 16
    for i, w in want.items():
        parts, status, gap = S.results(ka, kb)[i]
        assert gap is None or gap >= S.MIN_GAP
        assert ([len(p) for p in parts], [len(r) for p in parts for r in p], status) == w, (names[i], w)
    for name in ("a null a", "a null b", "an empty a", "an empty b", "an invalid ring in a", "an invalid ring in b"):
        i = names.index("union: clip: " + name)
        assert S.results(ka, kb)[i][:2] == (None, S.ST_NULL), name


def test_the_consequences_the_header_names():
    """equal polygons: empty; neighbours: their union; b inside a: a hole; a hole of b: a shell inside that hole, its own part"""
    row = lambda name: S.hand_row(S.PG, S.PG, name)  # noqa: E731
    res = S.results(S.PG, S.PG)
    assert res[row("equal polygons")][:2] == ([], S.ST_EMPTY)
    parts = res[row("edge neighbours")][0]
    assert [abs(L._shoelace2(r)) // 2 for p in parts for r in p] == [200]
    parts = res[row("b inside a: a hole")][0]
    assert [L._shoelace2(r) // 2 for p in parts for r in p] == [100, -9]
    parts = res[row("annulus b inside a")][0]
    assert [[L._shoelace2(r) // 2 for r in p] for p in parts] == [[400, -64], [16]]
    parts = res[row("two triangles crossing six times")][0]
    assert len(parts) == 6 and len({pt for p in parts for pt in p[0]}) == 12  # six parts that share the six crossings, two by two


@pytest.mark.parametrize("ka,kb", S.FAMILIES, ids=FAMILY_IDS)
def test_exact_area_identity_on_every_fixture_row(ka, kb):
    """area(result) = area(a) + area(b) - 2 area(a ∩ b), in exact rationals, the intersection's area being overlay_ref.exact_area's"""
    A, B, av, bv, names = S.rows(ka, kb)
    for i, (a, b) in enumerate(zip(A, B)):
        parts, status, _gap = S.results(ka, kb)[i]
        shared = O.exact_area(ka, a, kb, b, bool(av[i]), bool(bv[i]))
        assert (parts is None) == (shared is None)
        if parts is None:
            continue
        assert status in (S.ST_OK, S.ST_TOUCH, S.ST_EMPTY), (names[i], status)
        assert S.area_of(parts) == S.row_area(ka, a) + S.row_area(kb, b) - 2 * shared, names[i]


@pytest.mark.parametrize("ka,kb", S.FAMILIES, ids=FAMILY_IDS)
def test_exact_point_membership_of_every_face(ka, kb):
    """a sample point of every face of the arrangement is in the result exactly when it is in int(a) xor in int(b) (every hand case,
    every third of the other rows)"""
    A, B, av, bv, names = S.rows(ka, kb)
    n_hand, checked = len(S.hand_expectations(ka, kb)), 0
    for i, (a, b) in enumerate(zip(A, B)):
        if i >= n_hand and i % 3:
            continue
        parts = S.results(ka, kb)[i][0]
        if parts is None:
            continue
        ra, rb = L.row_rings(ka, a), L.row_rings(kb, b)
        for t in S.face_samples(ra, rb):
            want = (L.row_position(t, ra) == L.INT) != (L.row_position(t, rb) == L.INT)
            assert S.in_parts(t, parts) == want, (names[i], t)
            checked += 1
    assert checked > 500


def test_swap_gives_the_same_rings():
    """the result for (b, a) has the rings of the result for (a, b), up to ring rotation and part order (every hand case, every fourth
    of the other rows of the mixed family)"""
    ka, kb = S.PG, S.MPG
    A, B, av, bv, names = S.rows(ka, kb)
    n_hand = len(S.hand_expectations(ka, kb))
    for i, (a, b) in enumerate(zip(A, B)):
        if i >= n_hand and i % 4:
            continue
        back = S.symdiff(kb, b, ka, a, S.SYMDIFF, bool(bv[i]), bool(av[i]))
        assert back[1] == S.results(ka, kb)[i][1] and S.canonical(back[0]) == S.canonical(S.results(ka, kb)[i][0]), names[i]
