"""The exact reference of the polygon union (tests/polyunion_ref.py) and its fixture, pinned by identities the reference shares no code
with: the exact area of a union is area(a) + area(b) minus the exact area of polyclip_ref's intersection, and one rational sample point
strictly inside every face of the arrangement of the two rows' edges lies in the result exactly when crossing numbers place it in the
interior of a or of b.  The hand cases carry their parts, rings, coordinates per ring and status stated by hand."""
import os

import numpy as np
import pytest

from tests import polyclip_ref as L
from tests import polyunion_ref as U

FAMILY_IDS = [f"{U.NAMES[a]}-{U.NAMES[b]}" for a, b in U.FAMILIES]


def test_regeneration_reproduces_the_committed_fixture():
    """polyunion_ref.regenerate() is deterministic: array for array first (the message names the array that moved), then the committed
    bytes are fixture_bytes(); the fixture stays in the size range of polyclip_lattice.npz"""
    z, fresh = np.load(U.GOLDEN), U.build_arrays()
    assert sorted(z.files) == sorted(fresh)
    for k, v in fresh.items():
        assert z[k].dtype == v.dtype and z[k].shape == v.shape and z[k].tobytes() == v.tobytes(), k
    assert open(U.GOLDEN, "rb").read() == U.fixture_bytes()
    assert os.path.getsize(U.GOLDEN) <= 2 * os.path.getsize(L.GOLDEN)


def test_no_fixture_row_is_unresolved_and_every_row_clears_the_gap():
    z = np.load(U.GOLDEN)
    for ka, kb in U.FAMILIES:
        for mname in U.MODES.values():
            status = z[U.fixture_key(ka, kb) + mname + "_status"]
            assert (status != U.ST_UNRESOLVED).all() and len(status) == len(U.rows(ka, kb)[0])


@pytest.mark.parametrize("ka,kb", U.FAMILIES, ids=FAMILY_IDS)
def test_hand_cases_have_the_structure_stated_by_hand(ka, kb):
    A, B, _av, _bv, names = U.rows(ka, kb)
    want = U.hand_expectations(ka, kb)
    assert len(want) >= 19
    for i, per_mode in want.items():
        for mode, w in per_mode.items():
            parts, status, gap = U.union(ka, A[i], kb, B[i], mode)
            got = ([len(p) for p in parts], [len(r) for p in parts for r in p], status)
            assert gap is None or gap >= U.MIN_GAP
            if w is not None:
                assert got == w, (names[i], got, w)
    # the one case left to the reference: the gap closed by a point touch fuses into the shell, which then touches itself there
    i = names.index("a C closed by a wedge that overlaps one end and touches the other at a point")
    parts, status, _gap = U.union(ka, A[i], kb, B[i], U.UNION)
    assert ([len(p) for p in parts], [len(r) for p in parts for r in p], status) == ([1], [12], U.ST_TOUCH)
    for name in ("clip: a null a", "clip: a null b", "clip: an empty a", "clip: an empty b", "clip: an invalid ring in a", "clip: an invalid ring in b"):
        i = names.index(name)
        _A, _B, av, bv, _n = U.rows(ka, kb)
        assert U.union(ka, A[i], kb, B[i], U.UNION, bool(av[i]), bool(bv[i]))[:2] == (None, U.ST_NULL), name


def test_the_innermost_shell_gets_the_hole_where_the_first_in_key_order_would_not():
    """annulus b inside the hole of annulus a: both shells enclose b's hole, a's comes first in key order, b's is the innermost"""
    parts, status, _gap = U.union(U.PG, U.BIG_RING, U.PG, U.SMALL_RING)
    assert status == U.ST_OK and [len(p) for p in parts] == [2, 2]
    assert [abs(L._shoelace2(r)) // 2 for p in parts for r in p] == [400, 144, 64, 16]
    first, _st = L.stitch(U._walk_arcs(L.row_rings(U.PG, U.BIG_RING), L.row_rings(U.PG, U.SMALL_RING), U.WALK_A, U.UNION, []) +
                          U._walk_arcs(L.row_rings(U.PG, U.SMALL_RING), L.row_rings(U.PG, U.BIG_RING), U.WALK_B, U.UNION, []))
    assert [len(p) for p in first] == [3, 1]  # (what rule 5 of gpk_polyclip.h, made for results without nested shells, would give)


@pytest.mark.parametrize("ka,kb", U.FAMILIES, ids=FAMILY_IDS)
def test_exact_area_identity_on_every_fixture_row(ka, kb):
    """area(a ∪ b) = area(a) + area(b) - area(a ∩ b), in exact rationals, the intersection being polyclip_ref's"""
    A, B, av, bv, names = U.rows(ka, kb)
    for i, (a, b) in enumerate(zip(A, B)):
        parts, status, _gap = U.union(ka, a, kb, b, U.UNION, bool(av[i]), bool(bv[i]))
        inter, st_i, _g = L.clip(ka, a, kb, b, L.INTERSECTION, bool(av[i]), bool(bv[i]))
        assert (parts is None) == (inter is None)
        if parts is None:
            continue
        assert status in (U.ST_OK, U.ST_TOUCH), (names[i], status)
        assert U.area_of(parts) == U.row_area(ka, a) + U.row_area(kb, b) - L.area_of(inter), names[i]


@pytest.mark.parametrize("ka,kb", U.FAMILIES, ids=FAMILY_IDS)
def test_exact_point_membership_of_every_face(ka, kb):
    """a sample point of every face of the arrangement is in the union exactly when it is in int(a) or int(b) (every hand case, every
    third of the other rows)"""
    A, B, av, bv, names = U.rows(ka, kb)
    n_hand, checked = len(U.hand_expectations(ka, kb)), 0
    for i, (a, b) in enumerate(zip(A, B)):
        if i >= n_hand and i % 3:
            continue
        parts, _status, _gap = U.union(ka, a, kb, b, U.UNION, bool(av[i]), bool(bv[i]))
        if parts is None:
            continue
        ra, rb = L.row_rings(ka, a), L.row_rings(kb, b)
        for t in U.face_samples(ra, rb):
            want = L.row_position(t, ra) == L.INT or L.row_position(t, rb) == L.INT
            assert U.in_parts(t, parts) == want, (names[i], t)
            checked += 1
    assert checked > 500
