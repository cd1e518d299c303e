"""GPU: the point relation mask and its join (gpk_point_relation / gpk_point_relation_join, csrc/gpk_pointrel.hip) against the exact
reference (tests/pointrel_ref.py; tests/test_pointrel_ref.py pins it).  Masks and pair sets are compared exactly.

  1. known answers and ties in the twelve family pairs, as-is and padded (both lane-group sizes), both argument orders, row maps, the
     ten names; 2. placements; 3. random lattice columns; 4. agreement with dwithin at 0, distance 0, gpk_predicate_rowwise, the line
     relation of [p, p], gpk_spatial_join and the dwithin join; 5. unusable rows and refused calls; 6. the join: nine predicates,
     count-only, pairs, masks, prebuilt and NULL index, left_row_base, capacity, device buffers, the punctual side on the right, both
     sides punctual, a self-join; 7. pairs for the work-group schedule, and its list loop past the first pass; 8. the table join and the sjoin router; 9. the older calls."""
import ctypes as C
import os
import re

import numpy as np
import pyarrow as pa
import pytest
import torch

from geopolars_amd import _abi
from geopolars_amd.geoseries import POINT_MASK_PREDICATES, GeoSeries
from geopolars_amd.spatial_index import (
    SpatialIndex,
    SpatialJoinRelationArgs,
    dwithin_pairs,
    join_pairs,
    point_relation_pairs,
    point_relation_pairs_device,
    sjoin,
    sjoin_pairs,
    spatial_join_point_relation,
)
from tests import exact_ref as X
from tests import linerel_ref as L
from tests import pointrel_ref as P

pytestmark = pytest.mark.gpu

PT, MPT, LS, MLS, PG, MPG = P.PT, P.MPT, P.LS, P.MLS, P.PG, P.MPG
FAMILY_IDS = [f"{P.NAMES[a]}-{P.NAMES[b]}" for a, b in P.FAMILIES]
PAD = 40  # collinear vertices put into every segment (a MULTIPOINT row repeats every point 41 times): a mean of 32 coordinates and more
NAMED = sorted(P.PREDICATES)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def series(kind, rows, validity=None):
    return GeoSeries(X.column(kind, rows, validity))


def lanes_of(a: GeoSeries, b: GeoSeries) -> int:
    """the lane-group size the launch picks (gpk_pointrel.hip group_size): 16 when a column that is no POINT column has a mean of 32
    coordinates a row"""
    mean = lambda s: 0.0 if s.array.geom_type == PT else s.array.n_coords / max(s.array.n_geoms, 1)  # noqa: E731
    return 16 if max(mean(a), mean(b)) >= 32.0 else 4


def no_empty_member(kind, row) -> bool:
    if kind == MLS:
        return all(len(m) for m in row)
    if kind == MPG:
        return all(len(p) and len(p[0]) for p in row)
    return True


def predicate_of(want, name, kb):
    return np.array([P.PREDICATES[name](int(m), P.DIM[kb]) for m in want], dtype=bool)


# ---- 1. known answers and ties ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("pad", [0, PAD], ids=["G4", "G16"])
@pytest.mark.parametrize("ka,kb", P.FAMILIES, ids=FAMILY_IDS)
def test_known_answers_and_ties(gpk, ka, kb, pad):
    for cases in (P.KNOWN, P.TIES):
        a, b, want, names = P.case_columns(cases, ka, kb, pad)
        if not len(a):
            continue
        sa, sb = series(ka, a), series(kb, b)
        assert lanes_of(sa, sb) == (16 if pad and (ka, kb) != (PT, PT) else 4)
        got = sa.point_relation(sb)
        assert np.array_equal(got, want), [(n, int(g), int(w)) for n, g, w in zip(names, got, want) if g != w]
        # the other argument order: the punctual side stays A (two punctual columns: self is A, the bits 4 and 8 change places)
        assert np.array_equal(sb.point_relation(sa), P.swapped(want) if P.DIM[kb] == 0 else want)
        # other_rows: every row of A against one row of B, against an unusable one and against an entry out of range
        one = series(kb, [None if kb == PT else [], b[0]])
        col = P.masks(ka, a, kb, [b[0]] * len(a))
        assert np.array_equal(sa.point_relation(one, other_rows=np.ones(len(a), dtype=np.uint32)), col)
        assert not sa.point_relation(one, other_rows=np.zeros(len(a), dtype=np.uint32)).any()
        assert not sa.point_relation(one, other_rows=np.full(len(a), 2, dtype=np.uint32)).any()
        for name in NAMED:
            assert np.array_equal(sa.point_predicate(sb, name), predicate_of(want, name, kb)), name
            assert np.array_equal(sa.predicate(sb, name), predicate_of(want, name, kb)), name
        if P.DIM[kb]:  # the punctual column on the right: the name is transposed
            for name in NAMED:
                assert np.array_equal(sb.point_predicate(sa, name), predicate_of(want, P.TRANSPOSED.get(name, name), kb)), name
        assert np.array_equal(sa.point_predicate(sb, "contains_properly"), predicate_of(want, "contains", kb))


def test_ties_through_the_join_refine(gpk):
    """every tie A against every tie B through the join's refine, with masks (full mask) and count-only (early stop), both group sizes"""
    for kb in (MPT, MLS, MPG):
        a0, b0, _, _ = P.case_columns(P.TIES, MPT, kb, 0)
        table = P.mask_table(MPT, a0, np.ones(len(a0), bool), kb, b0, np.ones(len(b0), bool))
        for pad in (0, PAD):
            a, b, _, _ = P.case_columns(P.TIES, MPT, kb, pad)
            sa, sb = series(MPT, a), series(kb, b)
            for pred, pid in P.PRED_IDS.items():
                p0, c0, m0 = P.expected_pairs(table, pred, P.DIM[kb])
                pairs, counts, masks = point_relation_pairs(sa, sb, pred)
                assert np.array_equal(pairs, p0) and np.array_equal(counts, c0) and np.array_equal(masks, m0), (kb, pad, pred)
                n = C.c_int64(-1)
                rc = _abi.lib().gpk_point_relation_join(sa.device().handle, sb.device().handle, None, pid, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None)
                assert rc == _abi.GPK_OK and n.value == len(p0), (kb, pad, pred)


# ---- 2. placement ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("offset,scale", P.PLACEMENTS, ids=["utm", "web-mercator", "tiny", "huge"])
def test_placement_does_not_change_the_mask(gpk, offset, scale):
    for ka, kb in ((MPT, MPT), (MPT, MLS), (MPT, MPG), (PT, LS), (PT, PG)):
        a, b, want, names = P.case_columns(P.TIES, ka, kb)
        sa = series(ka, [P.placed(ka, r, offset, scale) for r in a])
        sb = series(kb, [P.placed(kb, r, offset, scale) for r in b])
        got = sa.point_relation(sb)
        assert np.array_equal(got, want), [(n, int(g), int(w)) for n, g, w in zip(names, got, want) if g != w]


# ---- 3. random lattice columns -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("pad", [0, PAD], ids=["as-is", "padded"])
@pytest.mark.parametrize("ka,kb", P.FAMILIES, ids=FAMILY_IDS)
def test_random_columns(gpk, ka, kb, pad):
    A, B, want = P.random_columns(ka, kb)
    assert len(A) == 96 and P.honest(ka, kb, want)
    sa, sb = series(ka, [P.padded(ka, r, pad) for r in A]), series(kb, [P.padded(kb, r, pad) for r in B])
    assert lanes_of(sa, sb) == (16 if pad and (ka, kb) != (PT, PT) else 4)
    got = sa.point_relation(sb)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    assert np.array_equal(sb.point_relation(sa), P.swapped(want) if P.DIM[kb] == 0 else want)


# ---- 4. kernels the project already trusts -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("ka,kb", P.FAMILIES, ids=FAMILY_IDS)
def test_agrees_with_dwithin_distance_and_the_older_predicates(gpk, ka, kb):
    A, B, _ = P.random_columns(ka, kb)
    sa, sb = series(ka, A), series(kb, B)
    mask = sa.point_relation(sb)
    hit = (mask & 3) != 0
    # the point kernels of distance / dwithin keep geo's convention that a point is 0.0 away from an EMPTY member of a multi-geometry
    # (exact_ref.EMPTY_DISTANCE); the relation ignores empty members.  With a POINT column the statement holds on the other rows.
    same = np.array([ka != PT or no_empty_member(kb, r) for r in B])
    assert same.sum() >= 48 and (ka != PT or kb in (PT, MPT, LS, PG) or not same.all())
    assert np.array_equal(hit[same], sa.dwithin(sb, 0.0)[same])
    assert np.array_equal(hit[same], (sa.distance(sb) == 0.0)[same])
    assert sa.dwithin(sb, 0.0)[~same].all()  # (the convention itself)
    if ka == PT and P.DIM[kb] == 2:  # gpk_predicate_rowwise
        within = sa.point_predicate(sb, "within")
        assert np.array_equal(within, sa.within(sb)) and np.array_equal(within, sb.contains(sa))
        assert np.array_equal(sb.point_predicate(sa, "contains"), sb.contains(sa))
        assert np.array_equal(hit, sa.intersects(sb)) and np.array_equal(hit, sb.intersects(sa))
    if ka == PT and P.DIM[kb] == 1:  # gpk_line_relation of [p, p]
        ll = series(LS, [[p, p] for p in A]).line_relation(sb)
        mapped = ((ll & L.INTERIORS) != 0) * 1 | ((ll & L.INT_BND) != 0) * 2 | ((ll & L.A_OUTSIDE) != 0) * 4 | ((ll & L.B_OUTSIDE) != 0) * 8
        assert np.array_equal(mapped.astype(np.uint8), mask)


@pytest.mark.parametrize("ka,kb", [(PT, PG), (PT, MPG), (MPT, PG), (PT, LS), (MPT, MLS), (MPT, MPT), (PT, PT)], ids=lambda k: P.NAMES.get(k, k))
def test_intersects_join_agrees_with_the_older_joins(gpk, ka, kb):
    """the `intersects` pairs are those of gpk_dwithin_join at distance 0 and, for POINT x polygon, of gpk_spatial_join(intersects).

    Two conventions of the older calls bound the statement, and the test says where.  (1) With a POINT column gpk_dwithin_join puts a
    point at distance 0.0 from an EMPTY member of a multi-geometry (geo's convention, exact_ref.EMPTY_DISTANCE): right rows with an
    empty member are compared apart — there the older join reports every candidate.  (2) gpk_spatial_join evaluates
    `poly.contains(point)` whatever the predicate (include/geopolars_hip.h), so it leaves out a point ON a ring: on this fixture the
    new join has 1191 pairs, gpk_spatial_join(intersects) the 424 of them with the point in the interior, and the 767 it leaves out
    are exactly the pairs whose exact mask says "on the boundary" (10)."""
    A, av, B, bv, table, _ = P.join_fixture(ka, kb)
    sa, sb = series(ka, A, av), series(kb, B, bv)
    pairs, counts, masks = point_relation_pairs(sa, sb, "intersects")
    d_pairs, d_counts, _ = dwithin_pairs(sa, sb, 0.0)
    assert len(pairs) > 50
    if ka == PT:
        plain = np.array([no_empty_member(kb, r) if r is not None else True for r in B])
        assert np.array_equal(pairs[plain[pairs[:, 1]]], d_pairs[plain[d_pairs[:, 1]]])
        assert set(map(tuple, pairs.tolist())) <= set(map(tuple, d_pairs.tolist()))
    else:
        assert np.array_equal(pairs, d_pairs) and np.array_equal(counts, d_counts)
    if ka == PT and kb == PG:
        j_pairs, _ = join_pairs(sa, sb, "intersects")
        inside = masks == 9
        assert np.array_equal(pairs[inside], j_pairs) and inside.sum() > 50
        assert (masks[~inside] == 10).all() and np.array_equal(pairs[~inside], P.expected_pairs(table, "touches", 2)[0])


# ---- 5. unusable rows and refused calls ------------------------------------------------------------------------------------------------------


def test_unusable_rows_give_mask_zero_and_never_join(gpk):
    nan, inf = float("nan"), float("inf")
    sq = P.SQ4[0]
    good_pt, good_pg = (1, 1), [sq]
    bad_pts = [None, (nan, 1), (1, inf), (-inf, 0), good_pt, good_pt]  # POINT EMPTY, NaN, infinite; a null row; a usable one
    valid = [True, True, True, True, False, True]
    want = np.array([0, 0, 0, 0, 0, 9], dtype=np.uint8)
    assert np.array_equal(P.masks(PT, bad_pts, PG, [good_pg] * 6, av=valid), want)
    sb_, sg = series(PT, bad_pts, valid), series(PG, [good_pg] * 6)
    assert np.array_equal(sb_.point_relation(sg), want) and np.array_equal(sg.point_relation(sb_), want)
    bad_mpt = [[], [(1, 1), (nan, 1)], [(1, 1), (1, inf)], [(1, 1)], [(1, 1), (9, 9)], [(1, 1)]]
    mwant = np.array([0, 0, 0, 9, 13, 0], dtype=np.uint8)
    mvalid = [True, True, True, True, True, False]
    assert np.array_equal(series(MPT, bad_mpt, mvalid).point_relation(sg), mwant)
    # B unusable: an unclosed ring, three coordinates, collinear, a NaN, an infinite coordinate, an empty row, a null row
    bad_pg = [[sq[:-1]], [sq[:2] + sq[:1]], [[(0, 0), (2, 2), (4, 4), (0, 0)]], [[(0, 0), (4, 0), (4, nan), (0, 0)]], [[(0, 0), (inf, 0), (4, 4), (0, 0)]], [], [sq], [sq]]
    pvalid = [True] * 6 + [False, True]
    pwant = np.array([0, 0, 0, 0, 0, 0, 0, 9], dtype=np.uint8)
    assert np.array_equal(P.masks(PT, [good_pt] * 8, PG, bad_pg, bv=pvalid), pwant)
    assert np.array_equal(series(PT, [good_pt] * 8).point_relation(series(PG, bad_pg, pvalid)), pwant)
    bad_ls = [[], [(0, 0), (nan, 1)], [(0, 0), (1, inf)], [(0, 0), (2, 2)]]
    assert np.array_equal(series(PT, [good_pt] * 4).point_relation(series(LS, bad_ls)), np.array([0, 0, 0, 9], dtype=np.uint8))
    assert np.array_equal(series(MPT, [[good_pt]] * 4).point_relation(series(MPT, [[], [(nan, nan)], [(1, 1), (inf, 0)], [(1, 1)]])), np.array([0, 0, 0, 1], dtype=np.uint8))
    rows = np.array([5, 6, 0xFFFFFFFF, 4, 5, 0], dtype=np.uint32)  # entries out of range: mask 0
    assert np.array_equal(sb_.point_relation(sg, other_rows=rows), np.array([0, 0, 0, 0, 0, 9], dtype=np.uint8))
    assert np.array_equal(series(PT, [good_pt] * 6).point_relation(sg, other_rows=rows), np.array([9, 0, 0, 9, 9, 9], dtype=np.uint8))
    for name in POINT_MASK_PREDICATES:
        assert not sb_.point_predicate(sg, name)[:5].any(), name
    for pred in P.PRED_IDS:
        for l, r in ((sb_, sg), (sg, sb_)):
            pairs, _, _ = point_relation_pairs(l, r, pred)
            assert set(pairs[:, 0 if l is sb_ else 1].tolist()) <= {5}, pred


def test_refused_calls(gpk):
    lib = _abi.lib()
    line = [(0, 0), (4, 4)]
    sl, sm = series(LS, [line] * 3), series(MLS, [[line]] * 3)
    sp = series(PG, [P.SQ4] * 3)
    pts, pts2, mpt = series(PT, [(1.0, 1.0)] * 3), series(PT, [(1.0, 1.0)] * 2), series(MPT, [[(1.0, 1.0)]] * 3)
    out = np.zeros(3, dtype=np.uint8)
    call = lambda a, b, rows=None: lib.gpk_point_relation(a.device().handle, b.device().handle, rows, out.ctypes.data, _abi.MEM_HOST, None)  # noqa: E731
    assert call(pts, sl) == _abi.GPK_OK and (out == 9).all()
    assert call(mpt, pts) == _abi.GPK_OK and (out == 1).all()
    assert call(pts, pts2) == _abi.GPK_ERR_INVALID_ARGUMENT  # row counts differ
    assert lib.gpk_point_relation(pts.device().handle, sl.device().handle, None, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    for a, b in ((sp, pts), (sl, pts), (sm, mpt), (sp, sp), (sl, sp)):  # the punctual column comes first in the C call
        assert call(a, b) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    assert call(sl, pts2) == _abi.GPK_ERR_MISMATCHED_GEOMETRY  # the families before the counts
    n = C.c_int64(-1)
    join = lambda a, b, pred, idx=None: lib.gpk_point_relation_join(a.device().handle, b.device().handle, idx, pred, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None)  # noqa: E731
    for a, b, own in ((sp, sl, "gpk_line_polygon_join"), (sl, sp, "gpk_line_polygon_join"), (sl, sm, "gpk_line_relation_join"), (sp, sp, "gpk_polygon_relation_join")):
        assert join(a, b, 0) == _abi.GPK_ERR_MISMATCHED_GEOMETRY and own in _abi.last_error()
    for pred in (-1, 9, 99):
        assert join(pts, sl, pred) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert join(sp, sl, 99) == _abi.GPK_ERR_INVALID_ARGUMENT  # the predicate id first
    idx = SpatialIndex(series(LS, [line] * 2), for_points=False)  # an index over another column
    assert join(pts, sl, 0, idx.handle) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert join(sp, sl, 0, idx.handle) == _abi.GPK_ERR_MISMATCHED_GEOMETRY  # the families before the index
    idx.free()
    assert join(pts, sl, 0) == _abi.GPK_OK and n.value == 9
    assert join(sl, pts, 2) == _abi.GPK_OK and n.value == 9  # the line contains the point: the point is within the line
    assert join(sl, pts, 1) == _abi.GPK_OK and n.value == 0  # no line lies within a point
    # a predicate that can never hold for the pair of families: a valid call with zero pairs and zero counts
    counts = np.full(3, 7, dtype=np.uint32)
    for a, b, pred in ((pts, sl, 7), (pts, sp, 7), (sl, mpt, 7), (pts, mpt, 5), (mpt, mpt, 5)):
        n.value = -1
        rc = lib.gpk_point_relation_join(a.device().handle, b.device().handle, None, pred, 0, counts.ctypes.data, None, None, 0, C.byref(n), _abi.MEM_HOST, None)
        assert rc == _abi.GPK_OK and n.value == 0 and not counts.any()
        counts[:] = 7
    small = np.zeros((8, 2), dtype=np.uint32)
    rc = lib.gpk_point_relation_join(pts.device().handle, sl.device().handle, None, 0, 0, None, small.ctypes.data, None, 8, C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_CAPACITY and n.value == 9
    rc = lib.gpk_point_relation_join(pts.device().handle, sl.device().handle, None, 0, 0, None, None, None, 8, C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_INVALID_ARGUMENT  # a capacity without a pair buffer
    with pytest.raises(NotImplementedError, match="Point x"):
        pts.touches(sp)


# ---- 6. the join ---------------------------------------------------------------------------------------------------------------------------


def _check_join(sl, sr, table, dim_b, transpose=False, may_be_empty=()):
    lib = _abi.lib()
    idx = SpatialIndex(sr, for_points=False)
    for pred, pid in P.PRED_IDS.items():
        p0, c0, m0 = P.expected_pairs(table, pred, dim_b, transpose)
        assert len(p0) > 0 or pred in may_be_empty, pred
        for ix in (None, idx):
            pairs, counts, masks = point_relation_pairs(sl, sr, pred, r_index=ix)
            assert np.array_equal(pairs, p0), (pred, len(pairs), len(p0))
            assert np.array_equal(counts, c0) and np.array_equal(masks, m0), pred
        n = C.c_int64(-1)  # count-only: the early-stop form of the refine
        assert lib.gpk_point_relation_join(sl.device().handle, sr.device().handle, idx.handle, pid, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_OK
        assert n.value == len(p0), pred
        got = np.zeros((max(len(p0), 1), 2), dtype=np.uint32)  # pairs without masks: early stop, emitted
        assert lib.gpk_point_relation_join(sl.device().handle, sr.device().handle, None, pid, 0, None, got.ctypes.data, None, len(got), C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_OK
        assert np.array_equal(got[: len(p0)], p0), pred
    # device buffers, left_row_base and the capacity error on the largest pair set
    p0, c0, m0 = P.expected_pairs(table, "intersects", dim_b, transpose)
    assert len(p0) > 50
    counts = torch.full((len(c0),), -1, dtype=torch.int32, device="cuda:0")
    assert point_relation_pairs_device(sl.device(), sr.device(), None, "intersects", counts, None) == len(p0)
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy().astype(np.uint32), c0)
    pairs = torch.zeros((len(p0) + 3, 2), dtype=torch.int32, device="cuda:0")
    masks = torch.zeros(len(p0) + 3, dtype=torch.uint8, device="cuda:0")
    assert point_relation_pairs_device(sl.device(), sr.device(), idx, "intersects", counts, pairs, masks, left_row_base=1000) == len(p0)
    torch.cuda.synchronize()
    assert np.array_equal(pairs.cpu().numpy().astype(np.uint32)[: len(p0)], p0 + np.array([1000, 0], dtype=np.uint32))
    assert np.array_equal(masks.cpu().numpy()[: len(p0)], m0)
    small = np.zeros((len(p0) - 1, 2), dtype=np.uint32)
    n = C.c_int64(-1)
    rc = lib.gpk_point_relation_join(sl.device().handle, sr.device().handle, None, 0, 0, None, small.ctypes.data, None, len(small), C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_CAPACITY and n.value == len(p0)
    idx.free()


NEVER = {0: ("crosses",), 1: ("overlaps",), 2: ("overlaps",)}


@pytest.mark.parametrize("ka,kb", [(PT, PG), (MPT, MPG), (PT, LS), (MPT, MLS)], ids=["pt-pg", "mpt-mpg", "pt-ls", "mpt-mls"])
def test_join_against_the_brute_force_table(gpk, ka, kb):
    A, av, B, bv, table, _ = P.join_fixture(ka, kb)
    empty = NEVER[P.DIM[kb]] + (("crosses", "contains", "covers", "equals") if ka == PT or P.DIM[kb] == 2 else ())
    _check_join(series(ka, A, av), series(kb, B, bv), table, P.DIM[kb], may_be_empty=empty)


@pytest.mark.parametrize("ka,kb", [(PT, PG), (MPT, MLS)], ids=["pg-pt", "mls-mpt"])
def test_join_with_the_punctual_side_on_the_right(gpk, ka, kb):
    """the lines or polygons on the left: the transposed predicate is evaluated, the masks keep A = the punctual side"""
    A, av, B, bv, table, _ = P.join_fixture(ka, kb)
    empty = NEVER[P.DIM[kb]] + (("crosses", "within", "covered_by", "equals") if ka == PT or P.DIM[kb] == 2 else ())
    _check_join(series(kb, B, bv), series(ka, A, av), table, P.DIM[kb], transpose=True, may_be_empty=empty)


@pytest.mark.parametrize("ka,kb", [(PT, PT), (MPT, MPT), (PT, MPT)], ids=["pt-pt", "mpt-mpt", "pt-mpt"])
def test_join_of_two_punctual_columns(gpk, ka, kb):
    A, av, B, bv, table, _ = P.join_fixture(ka, kb)
    empty = NEVER[0] + (("overlaps", "covers", "contains") if ka == PT else ()) + (("touches",))
    _check_join(series(ka, A, av), series(kb, B, bv), table, 0, may_be_empty=empty)


@pytest.mark.parametrize("ka", [PT, MPT], ids=["pt", "mpt"])
def test_self_join_finds_the_duplicates(gpk, ka):
    A, av, _, _, _, table = P.join_fixture(ka, PG)
    s = series(ka, A, av)
    _check_join(s, s, table, 0, may_be_empty=("crosses", "touches") + (("overlaps",) if ka == PT else ()))
    usable = np.nonzero(table.diagonal())[0]
    for pred, on_diagonal in (("intersects", True), ("equals", True), ("within", True), ("contains", True), ("covered_by", True), ("covers", True),
                              ("touches", False), ("crosses", False), ("overlaps", False)):
        pairs = point_relation_pairs(s, s, pred)[0]
        diag = pairs[pairs[:, 0] == pairs[:, 1], 0]
        assert np.array_equal(diag, usable if on_diagonal else usable[:0]), pred
    e = point_relation_pairs(s, s, "equals")[0]
    assert len(e) >= len(usable) + 20 and np.array_equal(e[np.lexsort((e[:, 0], e[:, 1]))][:, ::-1], e)  # duplicates: symmetric


# ---- 7. pairs for the work-group schedule ------------------------------------------------------------------------------------------------------


def large_cost() -> int:
    """PT_LARGE_COST, read from the header text"""
    csrc = os.path.join(ROOT, "geopolars_amd", "csrc")
    value = re.search(r"constexpr int64_t PT_LARGE_COST = ([^;]+);", open(os.path.join(csrc, "gpk_pointrel.h")).read()).group(1).strip()
    if value == "PD_LARGE_COST":
        value = re.search(r"constexpr int64_t PD_LARGE_COST = ([^;]+);", open(os.path.join(csrc, "gpk_frac.h")).read()).group(1).strip()
    assert re.fullmatch(r"[0-9 <*+()]+", value), value
    return int(eval(value))  # noqa: S307 (digits and operators only)


def _cloud(n, seed, lo=-4, hi=330):
    rng = np.random.default_rng(seed)
    return [(int(x), int(y)) for x, y in rng.integers(lo, hi, size=(n, 2))]


def test_large_pairs(gpk):
    """a multipoint of 600 points against a 300-coordinate polygon with a hole and a 400-coordinate zigzag: ten listed pairs in one call,
    against the reference and against the same points cut into rows of 40 (the bits 1, 2, 4 are the OR over the pieces)"""
    cost = large_cost()
    donut, zig = P.big_donut(), P.zigzag()
    assert len(donut[0]) + len(donut[1]) >= 295 and len(zig) == 400 and 600 * 295 > cost
    for kb, row, on in ((PG, donut, donut[0][:60] + donut[1]), (LS, zig, zig[:50] + [(1, 0), (3, 2), (5, 2)])):
        # three point sets in turn: anywhere and on coordinates of B; in a window that lies inside the polygon; anywhere
        sets = [_cloud(600 - len(on), 10 * kb) + on, _cloud(600, 77, 1, 99), _cloud(600, 78)]
        A = [sets[i % 3] for i in range(10)]
        sa, sb = series(MPT, A), series(kb, [row])
        rows = np.zeros(10, dtype=np.uint32)
        got = sa.point_relation(sb, other_rows=rows)
        want = np.array([P.mask(MPT, s, kb, row) for s in sets], dtype=np.uint8)[np.arange(10) % 3]
        assert np.array_equal(got, want) and len(set(want.tolist())) > 1, (got, want)
        pieces = [a[k : k + 40] for a in A for k in range(0, 600, 40)]
        small = series(MPT, pieces).point_relation(sb, other_rows=np.zeros(len(pieces), dtype=np.uint32)).reshape(10, 15)
        assert np.array_equal(np.bitwise_or.reduce(small & 7, axis=1), got & 7)
        for name in ("intersects", "within", "touches", "crosses"):  # the join's refine lists the same pairs: early stop and full masks
            p0 = np.array([(i, 0) for i in range(10) if P.PREDICATES[name](int(want[i]), P.DIM[kb])], dtype=np.uint32).reshape(-1, 2)
            pairs, _, masks = point_relation_pairs(sa, sb, name)
            assert np.array_equal(pairs, p0) and np.array_equal(masks, want[p0[:, 0]]), name
            n = C.c_int64(-1)
            rc = _abi.lib().gpk_point_relation_join(sa.device().handle, sb.device().handle, None, P.PRED_IDS[name], 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None)
            assert rc == _abi.GPK_OK and n.value == len(p0), name


def test_large_pairs_of_two_finite_sets(gpk):
    """bit 8 of a listed pair is the same walk with the sides exchanged: a multipoint of 600 points against its subsets, itself, an
    overlapping set and a disjoint one in the same box, and against 300 degenerate members of a MULTILINESTRING"""
    a = sorted(set(_cloud(700, 5)))[:600]
    other = [p for p in sorted(set(_cloud(900, 6))) if p not in set(a)][:300]
    assert len(a) == 600 and len(other) == 300
    B = [a[::2], a[::-1], a[:299] + other[:1], other, a[:300] + a[:300]]
    sa = series(MPT, [a] * len(B))
    want = P.masks(MPT, [a] * len(B), MPT, B)
    assert want.tolist() == [5, 1, 13, 12, 5]
    assert np.array_equal(sa.point_relation(series(MPT, B)), want)
    assert np.array_equal(series(MPT, B).point_relation(sa), P.swapped(want))
    lines = [[[p, p] for p in b[:300]] for b in B]
    lwant = P.masks(MPT, [a] * len(B), MLS, lines)
    assert lwant.tolist() == [5, 5, 13, 12, 5] and np.array_equal(sa.point_relation(series(MLS, lines)), lwant)
    for name in ("contains", "equals", "overlaps", "intersects"):
        pairs = point_relation_pairs(sa, series(MPT, B), name)[0]
        assert np.array_equal(pairs[pairs[:, 0] == 0, 1], np.nonzero(predicate_of(want, name, MPT))[0]), name


def test_pairs_at_the_threshold(gpk):
    """n_A * n_B == PT_LARGE_COST stays with the lane groups, PT_LARGE_COST + 1 is listed: both answers are the reference's"""
    cost = large_cost()
    side = int(round(cost**0.5))
    assert side * side == cost
    line = [(2 * i, i % 2) for i in range(side)]
    at = [(2 * i, 1) for i in range(side)]  # every second point on a vertex
    long_line = [(i, (i % 2) * 2) for i in range(cost + 1)]
    A = [at, [(3, 2)], [(3, 1)], [(0, 0)]]
    B = [line, long_line, long_line, long_line]
    assert [len(a) * len(b) for a, b in zip(A, B)] == [cost, cost + 1, cost + 1, cost + 1]
    want = P.masks(MPT, A, LS, B)
    assert want.tolist() == [15, 9, 12, 10]  # (the last of the 256 points is the line's end)
    assert np.array_equal(series(MPT, A).point_relation(series(LS, B)), want)
    assert np.array_equal(series(PT, [a[0] for a in A[1:]]).point_relation(series(LS, B[1:])), want[1:])  # a POINT column lists nothing


def list_loop_base():
    """(A rows, B rows, base pairs as (row of A, row of B)) for test_list_kernel_past_its_first_pass: MULTIPOINT rows of 300, 280 and
    257 points — no multiple of the 256 threads — against MULTILINESTRING rows: a zigzag of 400 coordinates (one chunk), one of 1100
    (more than PT_CHUNK = 1024: staged in two chunks), and finite sets written as degenerate members [p, p] — a subset, a disjoint set,
    an overlapping set of 150 points (300 coordinates) and all 300 points twice (1200 coordinates: a finite B in two chunks)"""
    a = sorted(set(_cloud(400, 5)))[:300]
    other = [p for p in sorted(set(_cloud(500, 6))) if p not in set(a)][:150]
    assert len(a) == 300 and len(other) == 150
    A = [a, _cloud(280, 21), a[:200] + _cloud(57, 22)]
    as_members = lambda pts: [[p, p] for p in pts]  # noqa: E731
    B = [[P.zigzag(400)], [P.zigzag(1100)], as_members(a[::2]), as_members(other), as_members(a[:149] + other[:1]), as_members(a + a)]
    pairs = [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (1, 0), (1, 1), (2, 1), (2, 5), (1, 3), (2, 2)]
    return A, B, pairs


def test_list_kernel_past_its_first_pass(gpk):
    """point_relation_large_kernel runs on a fixed grid of PT_LIST_BLOCKS = 1024 work-groups and loops `e += gridDim.x` over the listed
    units, with its PtLds (the staged chunk of B, its ends, the word the threads OR their bits into) carried from one unit to the
    next; no other test lists more than ten units, so the loop's second trip never ran.  Here PT_LIST_BLOCKS + 293 units are listed,
    ordered by second_pass.rotating_tiling over twelve base pairs.  The list is filled by atomic appends of the first kernel, so its
    order is not the unit order and the tiling cannot promise that a work-group's second unit differs from its first: with twelve
    mixed base pairs it is only very likely for nearly all of the 293.  Expected masks come from pointrel_ref on the twelve base
    pairs alone.  That the units are listed rests on the reasoning below: the list's length stays on the device, no counter shows it.

    Why pt::prepare settles none of them before listing (gpk_pointrel.h): both rows have finite coordinates; B is no polygon (no ring
    rule); the boxes overlap (all of it lies in the cloud's square); and done(pre.mask, st) is false — pre.mask is 0 for a finite B
    and B_OUTSIDE for the zigzags, and the stop is that of the full mask for the row-wise call and for a join that returns masks, and
    {3, ALL} / {4, ALL} for the count-only `intersects` and `within`, which B_OUTSIDE = 8 does not meet.  n_A * n_B is above
    PT_LARGE_COST for every pair (asserted), and the column is a MULTIPOINT column, so every unit is listed.  A finite B leaves the
    first launch PENDING and makes two classify_workgroup calls in one trip."""
    from tests import second_pass as SP

    blocks = SP.fixed_grid("PT_LIST_BLOCKS")
    assert blocks == 1024 and "constexpr int PT_CHUNK = 1024;" in open(os.path.join(ROOT, "geopolars_amd", "csrc", "gpk_pointrel.hip")).read()
    cost = large_cost()
    A, B, pairs = list_loop_base()
    n_coords = lambda row: sum(len(m) for m in row)  # noqa: E731
    assert all(len(A[i]) * n_coords(B[j]) > cost for i, j in pairs) and all(len(a) % 256 for a in A)
    assert sorted(n_coords(b) for b in B) == [300, 300, 300, 400, 1100, 1200] and len(pairs) >= 8
    table = np.array([[P.mask(MPT, a, MLS, b) for b in B] for a in A], dtype=np.uint8)
    base = np.array([table[i, j] for i, j in pairs], dtype=np.uint8)
    assert len(set(base.tolist())) >= 4, base.tolist()
    n = SP.second_trip_rows(blocks, 1, 1)
    assert n > blocks and n == 1317
    order = SP.rotating_tiling(len(pairs), n, blocks)
    ia, ib = np.array([pairs[k][0] for k in order]), np.array([pairs[k][1] for k in order], dtype=np.uint32)
    ca, cb = X.column(MPT, A), X.column(MLS, B)
    sa, sb = GeoSeries(ca.take(ia.astype(np.int64))), GeoSeries(cb)
    got = sa.point_relation(sb, other_rows=ib)
    bad = np.nonzero(got != base[order])[0]
    assert len(bad) == 0, [(int(k), int(order[k]), int(got[k]), int(base[order[k]]), bool(k >= blocks)) for k in bad[:8]]
    # the join's refine lists the same kind of units: 3 rows of A tiled to 440 against the 6 rows of B give 2640 candidates, all listed
    reps = 440
    ja = np.arange(3 * reps) % 3
    sja = GeoSeries(ca.take(ja.astype(np.int64)))
    assert 3 * reps * len(B) > 2 * blocks
    for name in ("intersects", "within", "contains", "equals"):  # with masks: the full mask; count-only: the early stop
        hit = np.vectorize(lambda m: P.PREDICATES[name](int(m), 1), otypes=[bool])(table)
        p0 = np.array([(l, r) for l in range(3 * reps) for r in range(len(B)) if hit[ja[l], r]], dtype=np.uint32).reshape(-1, 2)
        pairs_got, _, masks = point_relation_pairs(sja, sb, name)
        assert 0 < len(p0) < 3 * reps * len(B) and np.array_equal(pairs_got, p0) and np.array_equal(masks, table[ja[p0[:, 0]], p0[:, 1]]), name
        k = C.c_int64(-1)
        rc = _abi.lib().gpk_point_relation_join(sja.device().handle, sb.device().handle, None, P.PRED_IDS[name], 0, None, None, None, 0, C.byref(k), _abi.MEM_HOST, None)
        assert rc == _abi.GPK_OK and k.value == len(p0), name


# ---- 8. the table join and the router ------------------------------------------------------------------------------------------------------------


def test_table_join_and_sjoin(gpk):
    a, b, want, _ = P.case_columns(P.TIES, PT, PG)
    sa, sb = series(PT, a), series(PG, [b[0], b[0]])  # the same polygon twice on the right
    lt = pa.table({"stop": pa.array(np.arange(len(a))), "geometry": sa.device().to_arrow("wkb")})
    rt = pa.table({"name": pa.array(["a", "b"]), "geometry": sb.device().to_arrow("wkb")})
    col = P.masks(PT, a, PG, [b[0]] * len(a))
    touching = [i for i, m in enumerate(col) if P.PREDICATES["touches"](int(m), 2)]
    assert touching and len(touching) < len(a)
    for join in (lambda **kw: spatial_join_point_relation(lt, rt, SpatialJoinRelationArgs(**kw)), lambda **kw: sjoin(lt, rt, **kw)):
        out = join(predicate="touches", relation_col="relation")
        assert out.column_names == ["stop_left", "geometry_left", "name_right", "geometry_right", "relation"]
        assert out.column("stop_left").to_pylist() == [i for i in touching for _ in range(2)]
        assert out.column("relation").to_pylist() == [int(col[i]) for i in touching for _ in range(2)]
        left = join(predicate="touches", join_type="left", relation_col="relation", l_suffix="_l", r_suffix="_r")
        assert left.column_names == ["stop_l", "geometry_l", "name_r", "geometry_r", "relation"]
        assert left.num_rows == 2 * len(touching) + len(a) - len(touching)
        assert left.column("relation").null_count == len(a) - len(touching)
    # the polygons on the left: "polygon contains point" is the transposed name, the mask keeps A = the point
    out = sjoin(rt, lt, predicate="contains", relation_col="relation")
    inside = [i for i, m in enumerate(col) if P.PREDICATES["within"](int(m), 2)]
    assert inside and out.column("stop_right").to_pylist() == inside * 2 and out.column("relation").to_pylist() == [int(col[i]) for i in inside] * 2
    # the router reaches the other three families with their own masks
    la, lb, lwant, _ = L.case_columns(L.TIES, LS, LS)
    pairs, _, masks = sjoin_pairs(series(LS, la), series(LS, lb), "touches")
    diag = pairs[:, 0] == pairs[:, 1]
    assert np.array_equal(pairs[diag, 0], np.nonzero([L.PREDICATES["touches"](int(m)) for m in lwant])[0]) and np.array_equal(masks[diag], lwant[pairs[diag, 0]])
    assert len(sjoin_pairs(sb, sb, "equals")[0]) == 4 and len(sjoin_pairs(series(LS, [[(1, 1), (3, 3)]]), sb, "within")[0]) == 2
    assert np.array_equal(series(LS, la).predicate(series(LS, lb), "touches"), series(LS, la).line_predicate(series(LS, lb), "touches"))
    assert series(LS, [[(1, 1), (3, 3)]] * 2).predicate(sb, "within").all() and sb.predicate(sb, "equals").all()


# ---- 9. the older calls stay ---------------------------------------------------------------------------------------------------------------------


def test_the_older_calls_stay(gpk):
    """gpk_predicate_rowwise and gpk_spatial_join on the fixtures against the reference's answers, and the refusals of the named methods"""
    for kb in (PG, MPG):
        A, B, want = P.random_columns(PT, kb)
        sa, sb = series(PT, A), series(kb, B)
        inside, meets = (want & 7) == 1, (want & 3) != 0
        assert np.array_equal(sa.within(sb), inside) and np.array_equal(sb.contains(sa), inside)
        assert np.array_equal(sa.intersects(sb), meets) and np.array_equal(sb.intersects(sa), meets)
    A, av, B, bv, table, _ = P.join_fixture(PT, PG)
    sa, sb = series(PT, A, av), series(PG, B, bv)
    p0, c0, _ = P.expected_pairs(table, "within", 2)  # gpk_spatial_join: `poly.contains(point)` whatever the predicate
    for name in ("intersects", "within"):
        pairs, counts = join_pairs(sa, sb, name)
        assert len(p0) > 50 and np.array_equal(pairs, p0) and np.array_equal(counts, c0), name
    for name in ("touches", "crosses", "covered_by", "covers", "disjoint", "overlaps", "geom_equals"):
        with pytest.raises(NotImplementedError, match="Point x"):
            getattr(sa, name)(sb)
