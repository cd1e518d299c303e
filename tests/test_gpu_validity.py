"""GPU: gpk_validity and gpk_is_simple (csrc/gpk_validity.hip) against the exact reference of tests/validity_ref.py: codes, `where`
values and simplicity answers are compared exactly, on every schedule (4 and 16 lanes a row, the work-group path), at several
placements, at filter failures, and for unusable rows and refusals."""
import ctypes as C

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoseries import GeoSeries
from tests import relation_ref as R
from tests import validity_ref as V
from tests.exact_ref import column

pytestmark = pytest.mark.gpu
PG, MPG, LS, MLS = V.PG, V.MPG, V.LS, V.MLS


def series(kind, rows, valid=None):
    return GeoSeries(column(kind, rows, valid))


def device_answers(s: GeoSeries):
    """codes and where through a device output buffer"""
    import torch

    n = len(s)
    code = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    where = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    _abi.check(_abi.lib().gpk_validity(s.device().handle, code.data_ptr(), where.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    return code.cpu().numpy(), where.cpu().numpy()


def check(kind, rows, valid, codes, where, device=False):
    s = series(kind, rows, valid)
    got_c, got_w = s.is_valid_reason(return_where=True)
    bad = np.nonzero((got_c != codes) | (got_w != where))[0]
    assert len(bad) == 0, [(int(i), int(got_c[i]), int(codes[i]), int(got_w[i]), int(where[i])) for i in bad[:8]]
    assert np.array_equal(s.is_valid(), codes == 0)
    assert np.array_equal(s.is_valid_reason(), codes)  # (without out_where)
    if device:
        dc, dw = device_answers(s)
        assert np.array_equal(dc, codes) and np.array_equal(dw, where)
    return s


@pytest.mark.parametrize("kind", [PG, MPG])
def test_known_answers(kind):
    rows, valid, codes, where = V.known_column(kind)
    check(kind, rows, valid, codes, where, device=True)


@pytest.mark.parametrize("kind", [LS, MLS])
def test_known_simplicity(kind):
    import torch

    rows, valid, want = V.known_simple_column(kind)
    s = series(kind, rows, valid)
    assert np.array_equal(s.is_simple(), want)
    out = torch.full((len(s),), 9, dtype=torch.uint8, device="cuda")
    _abi.check(_abi.lib().gpk_is_simple(s.device().handle, out.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().astype(bool), want)


@pytest.mark.parametrize("kind", [PG, MPG])
def test_random_lattice_columns(kind):
    rows, valid, codes, where = V.random_column(kind)
    count = np.bincount(codes, minlength=10)
    for c in range(9):
        if not (c == V.NESTED_MEMBERS and kind == PG):  # (a POLYGON row has one member)
            assert count[c] >= 3, (c, count.tolist())
    check(kind, rows, valid, codes, where)


def _finite_rows(kind, rows, valid, codes):
    keep = [i for i, c in enumerate(codes) if c != V.COORDINATE]
    return [rows[i] for i in keep], [valid[i] for i in keep], keep


@pytest.mark.parametrize("kind", [PG, MPG])
@pytest.mark.parametrize("G", [V.VAL_G_SMALL, V.VAL_G_LARGE])
def test_padded_rows_on_every_lane_group(kind, G):
    """collinear vertices inside every edge: the codes stay and rings grow past 3 G + 1 segments, so every lane strides more than once
    and the tail is ragged.  16 lanes: every row gets 12 more vertices an edge (a triangle has 39 segments, a square 52).  4 lanes:
    3 more vertices an edge (a square has 16 > 13 segments), but only in every `every`-th row — the largest share that keeps the
    column's mean below VAL_G_MEAN — once from row 0 and once from the middle of the period"""
    rings_of = lambda row: row if kind == PG else [q for p in row for q in p]  # noqa: E731
    for src in (V.known_column, V.random_column):
        rows, valid, codes, _ = src(kind)
        rows, valid, keep = _finite_rows(kind, rows, valid, codes)
        n_of = lambda rr: sum(V.n_coords(kind, r) for r in rr)  # noqa: E731
        if G == V.VAL_G_LARGE:
            k, every = 12, 1
        else:
            k = 3
            every = min(e for e in range(1, 40) if all(V.lanes_of(n_of(V.padded(kind, rows, k, e, f)), len(rows)) == G for f in (0, e // 2)))
        for first in sorted({0, every // 2}):
            prows = V.padded(kind, rows, k, every, first)
            assert V.lanes_of(n_of(prows), len(rows)) == G
            assert max(len(r) - 1 for row in prows for r in rings_of(row)) > 3 * G + 1
            assert sum(len(r) - 1 > 3 * G + 1 for row in prows for r in rings_of(row)) >= 8  # more than a ring or two
            pc, pw = V.validity_column(kind, prows, valid)
            # the answers stay, except that a ring of fewer than 4 coordinates (code 2) grows into a spike (code 3)
            moved = np.nonzero(pc != codes[keep])[0]
            assert all(codes[keep][i] == V.RING_SHAPE and pc[i] == V.SELF_INTERSECTION for i in moved) and len(moved) <= 6
            check(kind, prows, valid, pc, pw)


def test_work_group_path():
    rows, codes, where = V.large_column()
    assert all(V.n_coords(PG, r) > V.VAL_BLOCK_COORDS for r in rows)
    assert codes.tolist() == [V.VALID, V.SELF_INTERSECTION, V.SELF_INTERSECTION, V.SELF_INTERSECTION, V.VALID, V.RINGS_CROSS]
    # the strips: 4095 segments in 511 strips of 8 units; the planted faults lie in the first strip, the last one, and across many
    assert (4096 - 1) // V.VAL_SEGS_PER_STRIP <= V.VAL_STRIPS_MAX and 4096 + 2 * V.VAL_STRIPS_MAX < V.VAL_ENTRIES
    check(PG, rows, None, codes, where, device=True)
    # among small rows too: the same column with the known answers in front
    krows, kvalid, kcodes, kwhere = V.known_column(PG)
    base = sum(V.n_coords(PG, r) for r in krows)
    check(PG, krows + rows, kvalid + [True] * len(rows), np.concatenate([kcodes, codes]), np.concatenate([kwhere, np.where(where >= 0, where + base, -1)]).astype(np.int32))


def test_fixtures_land_on_each_path():
    n = lambda kind, rows: sum(V.n_coords(kind, r) for r in rows)  # noqa: E731
    rows = V.known_column(PG)[0]
    assert V.lanes_of(n(PG, rows), len(rows)) == V.VAL_G_SMALL and max(V.n_coords(PG, r) for r in rows) <= V.VAL_BLOCK_COORDS
    rows = V.random_column(MPG)[0]
    assert max(V.n_coords(MPG, r) for r in rows) <= V.VAL_BLOCK_COORDS
    big = V.large_column()[0]
    assert V.lanes_of(n(PG, big), len(big)) == V.VAL_G_LARGE and min(V.n_coords(PG, r) for r in big) > V.VAL_BLOCK_COORDS


@pytest.mark.parametrize("kind", [PG, MPG])
def test_placements(kind):
    for src in (V.known_column, V.random_column):
        rows, valid, codes, where = src(kind)
        rows, valid, keep = _finite_rows(kind, rows, valid, codes)
        for scale, shift in V.PLACEMENTS:
            check(kind, V.placed(kind, rows, scale, shift), valid, codes[keep], _rebased(kind, rows, where[keep], src(kind)[0], keep))


def _rebased(kind, rows, where, all_rows, keep):
    """`where` of the kept rows after the others were dropped from the column"""
    old = np.concatenate([[0], np.cumsum([V.n_coords(kind, r) for r in all_rows])])[keep]
    new = np.concatenate([[0], np.cumsum([V.n_coords(kind, r) for r in rows])])[:-1]
    return np.where(where >= 0, where - old + new, -1).astype(np.int32)


def test_filter_failures():
    """a hole vertex exactly on a shell edge of slope 1/3 at coordinates with 50 significant bits, then one ulp to either side: the
    float filter cannot decide these orientations, the expansion path must, and the reference says what it decides"""
    e = 2.0**-40
    a = (1.0 + e, 1.0 + 3 * e)
    b = (a[0] + 12.0 + 3 * e, a[1] + 4.0 + e)  # b - a = (12 + 3 e, 4 + e): slope exactly 1/3
    mid = (a[0] + 6.0 + 1.5 * e, a[1] + 2.0 + 0.5 * e)
    assert V._cross(*[x - y for x, y in zip(V._fr(b), V._fr(a))], *[x - y for x, y in zip(V._fr(mid), V._fr(a))]) == 0
    shell = [a, b, (13.0, 30.0), (1.0, 30.0), a]
    rows = []
    for dy in (0.0, np.nextafter(mid[1], np.inf) - mid[1], np.nextafter(mid[1], -np.inf) - mid[1]):
        v = (mid[0], mid[1] + dy)
        rows.append([shell, [v, (6.0, 12.0), (8.0, 12.0), v]])
    codes, where = V.validity_column(PG, rows)
    assert codes.tolist() == [V.VALID, V.VALID, V.RINGS_CROSS]  # on the edge: a touch; above it: inside; below: the hole pokes out
    check(PG, rows, None, codes, where)
    lines = []
    for dy in (0.0, np.nextafter(mid[1], np.inf) - mid[1], np.nextafter(mid[1], -np.inf) - mid[1]):
        lines.append([[a, b], [(7.0, 12.0), (mid[0], mid[1] + dy)]])
    want = V.is_simple_column(MLS, lines)
    assert want.tolist() == [False, True, False]  # an end point inside the other member's segment; an ulp short of it; an ulp beyond: a crossing
    assert np.array_equal(series(MLS, lines).is_simple(), want)


def test_unusable_rows_and_refusals():
    sqr = V.sq(0, 0, 4, 4)
    nan_ring = [(0.0, 0.0), (float("nan"), 1.0), (1.0, 1.0), (0.0, 0.0)]
    inf_ring = [(0.0, 0.0), (float("-inf"), 1.0), (1.0, 1.0), (0.0, 0.0)]
    rows = [[[sqr]], [], [[], [[]]], [[sqr]], [[nan_ring]], [[inf_ring]]]  # MULTIPOLYGON rows: 5 + 0 + 0 + 5 + 4 + 4 coordinates
    valid = [True, True, True, False, True, True]
    codes, where = V.validity_column(MPG, rows, valid)
    assert codes.tolist() == [0, 0, 0, 9, 1, 1] and where.tolist() == [-1, -1, -1, -1, 11, 15]
    check(MPG, rows, valid, codes, where, device=True)
    # zero rows: nothing happens, on either call
    empty_p, empty_l = series(PG, []), series(LS, [])
    assert len(empty_p.is_valid()) == 0 and len(empty_p.is_valid_reason(return_where=True)[1]) == 0 and len(empty_l.is_simple()) == 0
    lib = _abi.lib()
    assert lib.gpk_validity(empty_p.device().handle, None, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    # wrong families through the C ABI
    out = np.zeros(8, dtype=np.uint8)
    lines = series(LS, [[(0.0, 0.0), (1.0, 1.0)]])
    pts = GeoSeries(column(_abi.GEOM_POINT, [(0.0, 0.0)]))
    polys = series(PG, [[sqr]])
    for h in (lines, pts):
        assert lib.gpk_validity(h.device().handle, out.ctypes.data, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    for h in (polys, pts):
        assert lib.gpk_is_simple(h.device().handle, out.ctypes.data, _abi.MEM_HOST, None) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    assert not out.any()


@pytest.mark.parametrize("kind", [PG, MPG])
def test_valid_rows_are_what_the_relations_need(kind):
    """a non-empty valid row equals itself; every row whose rings the relation calls reject has a code from 1 to 3"""
    for src in (V.known_column, V.random_column):
        rows, valid, codes, _ = src(kind)
        s = series(kind, rows, valid)
        got = s.is_valid_reason()
        assert np.array_equal(got, codes)
        nonempty = np.array([bool(v) and len(R.row_polys(kind, r)) > 0 for r, v in zip(rows, valid)])
        sel = nonempty & (got == 0)
        assert sel.sum() >= 3
        assert s.geom_equals(s)[sel].all() and (s.polygon_relation(s)[sel] == 3).all()
        for i, (r, v) in enumerate(zip(rows, valid)):
            if v and any(not R._ring_usable(q) for p in R.row_polys(kind, r) for q in p):
                assert 1 <= got[i] <= 3, (i, int(got[i]))
