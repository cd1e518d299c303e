"""GPU: the line x polygon relation mask and its join (gpk_line_polygon_relation / gpk_line_polygon_join, csrc/gpk_linearea.hip) against
the exact rational reference (tests/relation_ref.py; tests/test_relation_ref.py pins it).  Masks and pair sets are compared exactly.

  1. known answers in the four family combinations, identity rows and poly_rows; 2. random lattice columns; 3. rings that touch each
  other at a point, with the line through the contact; 4. both lane-group sizes of the row-wise kernel and of the join's refine (rings
  padded with collinear vertices: the answers stay, the rows grow past the threshold); 5. placements; 6. unusable rows and refused
  calls; 7. agreement with the distance machinery (dwithin at 0); 8. the join: both side orders, every predicate, masks, capacity,
  count-only, left_row_base, prebuilt and NULL index, device buffers; 9. gpk_spatial_join's lines x polygons arm is still empty."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest
import torch

from geopolars_amd import _abi
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import (
    SpatialIndex,
    SpatialJoinRelationArgs,
    join_pairs,
    relation_pairs,
    relation_pairs_device,
    spatial_join_relation,
)
from tests import exact_ref as X
from tests import relation_ref as R

pytestmark = pytest.mark.gpu

LS, MLS, PG, MPG = R.LS, R.MLS, R.PG, R.MPG
FAMILY_IDS = [f"{R.NAMES[a]}-{R.NAMES[b]}" for a, b in R.FAMILIES]


def series(kind, rows, validity=None):
    return GeoSeries(X.column(kind, rows, validity))


def lanes_of(polys: GeoSeries) -> int:
    """the lane-group size the launch picks (gpk_linearea.h relation_group_size): 16 from a mean of 32 coordinates a polygon row"""
    a = polys.array
    return 16 if a.n_coords / max(a.n_geoms, 1) >= 32.0 else 4


# ---- 1. known answers ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kl,kp", R.FAMILIES, ids=FAMILY_IDS)
def test_known_answers(gpk, kl, kp):
    lines, polys, want = R.known_columns(kl, kp)
    sl, sp = series(kl, lines), series(kp, polys)
    assert np.array_equal(sl.line_polygon_relation(sp), want)
    assert np.array_equal(sp.line_polygon_relation(sl), want)  # either order of the two families
    # poly_rows: one polygon row (and an unusable one) for every line
    one = series(kp, [[], polys[0]])
    assert np.array_equal(sl.line_polygon_relation(one, other_rows=np.ones(len(lines), dtype=np.uint32)), want)
    assert not sl.line_polygon_relation(one, other_rows=np.zeros(len(lines), dtype=np.uint32)).any()
    # the named predicates, from either side
    for name, f in R.PREDICATES.items():
        if name in ("intersects", "within"):
            continue  # (GeoSeries.intersects / within are gpk_predicate_rowwise's and keep the reference's `false` arm)
        exp = np.array([f(int(m)) for m in want])
        assert np.array_equal(getattr(sl, name)(sp), exp), name
        if name != "covered_by":
            assert np.array_equal(getattr(sp, name)(sl), exp), name
    assert np.array_equal(sp.covers(sl), sl.covered_by(sp))
    assert not sp.covered_by(sl).any() and not sl.covers(sp).any()


# ---- 2. random lattice columns, both lane-group sizes ----------------------------------------------------------------------------------


@pytest.mark.parametrize("pad", [0, 1], ids=["as-is", "padded"])
@pytest.mark.parametrize("kl,kp", R.FAMILIES, ids=FAMILY_IDS)
def test_random_columns(gpk, kl, kp, pad):
    lines, polys, want = R.random_columns(kl, kp)
    sl = series(kl, [R.scaled_line(kl, r, pad) for r in lines])
    sp = series(kp, [R.padded(kp, r, pad) for r in polys])
    if pad:
        assert lanes_of(sp) == 16
    got = sl.line_polygon_relation(sp)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (bad[:5], got[bad[:5]], want[bad[:5]])


def test_fixtures_reach_both_lane_group_sizes(gpk):
    polys = R.random_columns(LS, PG)[1]
    assert lanes_of(series(PG, polys)) == 4 and lanes_of(series(PG, [R.padded(PG, r, 1) for r in polys])) == 16


# ---- 3 + 4. rings that touch, every kernel instance ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("pad", [0, 7], ids=["G4", "G16"])
@pytest.mark.parametrize("kl", [LS, MLS], ids=["ls", "mls"])
def test_ring_touch_rule(gpk, kl, pad):
    for kp, (lines, polys, want) in R.tie_columns(kl, pad).items():
        sl, sp = series(kl, [R.scaled_line(kl, r, pad) for r in lines]), series(kp, polys)
        assert lanes_of(sp) == (16 if pad else 4)
        got = sl.line_polygon_relation(sp)
        names = [t[0] for t in R.TIES if t[1] == kp]
        assert np.array_equal(got, want), [(n, int(g), int(w)) for n, g, w in zip(names, got, want) if g != w]


@pytest.mark.parametrize("pad", [0, 7], ids=["G4", "G16"])
def test_ring_touch_rule_in_the_join(gpk, pad):
    """every tie line against every tie polygon of its kind through the join's refine, both lane-group sizes"""
    for kp, (lines, polys, _) in R.tie_columns(LS, pad).items():
        lines = [R.scaled_line(LS, r, pad) for r in lines]
        sl, sp = series(LS, lines), series(kp, polys)
        assert lanes_of(sp) == (16 if pad else 4)
        table = np.stack([R.masks(LS, lines, kp, [p] * len(lines)) for p in polys], axis=1)
        for pred in ("intersects", "touches", "crosses", "covered_by", "within"):
            p0, c0, m0 = R.expected_pairs(table, pred)
            pairs, counts, masks = relation_pairs(sl, sp, pred)
            assert np.array_equal(pairs, p0) and np.array_equal(counts, c0) and np.array_equal(masks, m0), (kp, pred)
            n = C.c_int64(-1)  # count-only: the early-exit form of the refine
            rc = _abi.lib().gpk_line_polygon_join(sl.device().handle, sp.device().handle, None, R.PRED_IDS[pred], 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None)
            assert rc == _abi.GPK_OK and n.value == len(p0), (kp, pred)


# ---- 5. placement ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("offset,scale", R.PLACEMENTS, ids=["utm", "web-mercator", "tiny", "huge"])
def test_placement_does_not_change_the_mask(gpk, offset, scale):
    for kp, (lines, polys, want) in R.tie_columns(LS, 0).items():
        sl = series(LS, [R.placed(LS, r, offset, scale) for r in lines])
        sp = series(kp, [R.placed(kp, r, offset, scale) for r in polys])
        assert np.array_equal(sl.line_polygon_relation(sp), want)
    lines, polys, want = R.random_columns(MLS, MPG)
    sl = series(MLS, [R.placed(MLS, r, offset, scale) for r in lines])
    sp = series(MPG, [R.placed(MPG, r, offset, scale) for r in polys])
    assert np.array_equal(sl.line_polygon_relation(sp), want)


# ---- 6. unusable rows and refused calls ------------------------------------------------------------------------------------------------------


def test_unusable_rows_give_mask_zero(gpk):
    nan = float("nan")
    inside = [(1, 1), (3, 2)]
    open_ring = [(0, 0), (12, 0), (12, 12), (0, 12)]
    flat_ring = [(0, 0), (5, 0), (9, 0), (0, 0)]
    lines = [inside, inside, [], [(1, 1), (nan, 2)], inside, inside, inside, inside, [(1, 1)], inside]
    polys = [R.DONUT, R.DONUT, R.DONUT, R.DONUT, [], [open_ring], [R.sq(0, 0, 12, 12), [(4, 4), (8, 4), (4, 4)]], [flat_ring], R.DONUT, [R.sq(0, 0, 12, 12), []]]
    lv = [True, False, True, True, True, True, True, True, True, True]
    want = np.array([1, 0, 0, 0, 0, 0, 0, 0, 1, 1], dtype=np.uint8)
    assert np.array_equal(R.masks(LS, lines, PG, polys, lv=lv), want)
    assert np.array_equal(series(LS, lines, lv).line_polygon_relation(series(PG, polys)), want)
    pv = [True, True, True, True, True, True, True, True, False, True]
    want_pv = want.copy()
    want_pv[8] = 0
    assert np.array_equal(series(LS, lines, lv).line_polygon_relation(series(PG, polys, pv)), want_pv)
    # multi-geometries: empty members are ignored, a row of empty members only is unusable, one invalid ring spoils the row
    ml = [[[], inside], [[], []], [inside]]
    mp = [[[], R.DONUT], [[]], [R.DONUT, [open_ring]]]
    assert np.array_equal(series(MLS, ml).line_polygon_relation(series(MPG, mp)), np.array([1, 0, 0], dtype=np.uint8))
    # an out-of-range poly_rows entry
    rows = np.array([0, 10, 0xFFFFFFFF, 0, 0, 0, 0, 0, 0, 0], dtype=np.uint32)
    got = series(LS, lines, lv).line_polygon_relation(series(PG, polys), other_rows=rows)
    assert np.array_equal(got, np.array([1, 0, 0, 0, 1, 1, 1, 1, 1, 1], dtype=np.uint8))
    # every derived predicate is False on an unusable row
    bad = series(LS, [[], inside]), series(PG, [R.DONUT, []])
    for name in ("crosses", "touches", "covered_by", "disjoint"):
        assert not getattr(bad[0], name)(bad[1]).any(), name


def test_refused_calls(gpk):
    lib = _abi.lib()
    sl, sp = series(LS, [[(1, 1), (3, 2)]] * 3), series(PG, [R.DONUT] * 2)
    pts = GeoSeries(X.column(_abi.GEOM_POINT, [(1.0, 1.0)] * 3))
    out = np.zeros(3, dtype=np.uint8)
    call = lambda a, b, rows=None: lib.gpk_line_polygon_relation(a.device().handle, b.device().handle, rows, out.ctypes.data, _abi.MEM_HOST, None)  # noqa: E731
    assert call(sl, sp) == _abi.GPK_ERR_INVALID_ARGUMENT  # row counts differ
    for a, b in ((sp, sl), (sl, sl), (sp, sp), (pts, sp), (sl, pts)):
        assert call(a, b) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    n = C.c_int64(-1)
    join = lambda a, b, pred, idx=None: lib.gpk_line_polygon_join(a.device().handle, b.device().handle, idx, pred, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None)  # noqa: E731
    for a, b in ((sl, sl), (sp, sp), (pts, sp), (sl, pts)):
        assert join(a, b, 0) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    for pred in (-1, 5, 99):
        assert join(sl, sp, pred) == _abi.GPK_ERR_INVALID_ARGUMENT
    idx = SpatialIndex(sl, for_points=False)  # an index over another column
    assert join(sl, sp, 0, idx.handle) == _abi.GPK_ERR_INVALID_ARGUMENT
    idx.free()
    with pytest.raises(NotImplementedError, match="Point"):
        pts.crosses(sp)
    with pytest.raises(NotImplementedError):
        sl.touches(sl)


# ---- 7. an independent device path ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kl,kp", R.FAMILIES, ids=FAMILY_IDS)
def test_agrees_with_dwithin_at_zero(gpk, kl, kp):
    lines, polys, want = R.random_columns(kl, kp)
    sl, sp = series(kl, lines), series(kp, polys)
    mask = sl.line_polygon_relation(sp)
    assert np.array_equal((mask & 3) != 0, sl.dwithin(sp, 0.0))
    covered, within, touches = sl.covered_by(sp), R.PREDICATES["within"], sl.touches(sp)
    assert all((not c) or within(int(m)) or t for c, m, t in zip(covered, mask, touches))


# ---- 8. the join ---------------------------------------------------------------------------------------------------------------------------


def _check_join(sl, sr, table, transpose):
    lib = _abi.lib()
    idx = SpatialIndex(sr, for_points=False)
    for pred in ("intersects", "within", "covered_by", "crosses", "touches"):
        p0, c0, m0 = R.expected_pairs(table, pred, transpose)
        name = {"within": "contains", "covered_by": "covers"}.get(pred, pred) if transpose else pred
        for ix in (None, idx):
            pairs, counts, masks = relation_pairs(sl, sr, name, r_index=ix)
            assert np.array_equal(pairs, p0), (pred, len(pairs), len(p0))
            assert np.array_equal(counts, c0) and np.array_equal(masks, m0), pred
        n = C.c_int64(-1)  # count-only
        assert lib.gpk_line_polygon_join(sl.device().handle, sr.device().handle, idx.handle, R.PRED_IDS[pred], 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_OK
        assert n.value == len(p0), pred
    # device buffers, left_row_base and the capacity error on the largest pair set
    p0, c0, m0 = R.expected_pairs(table, "intersects", transpose)
    assert len(p0) > 300 and max(c0.max(), np.bincount(p0[:, 1]).max()) > 250  # the polygon that covers the domain
    counts = torch.full((len(c0),), -1, dtype=torch.int32, device="cuda:0")
    assert relation_pairs_device(sl.device(), sr.device(), None, "intersects", counts, None) == len(p0)
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy().astype(np.uint32), c0)
    pairs = torch.zeros((len(p0) + 3, 2), dtype=torch.int32, device="cuda:0")
    masks = torch.zeros(len(p0) + 3, dtype=torch.uint8, device="cuda:0")
    assert relation_pairs_device(sl.device(), sr.device(), idx, "intersects", counts, pairs, masks, left_row_base=1000) == len(p0)
    torch.cuda.synchronize()
    assert np.array_equal(pairs.cpu().numpy().astype(np.uint32)[: len(p0)], p0 + np.array([1000, 0], dtype=np.uint32))
    assert np.array_equal(masks.cpu().numpy()[: len(p0)], m0)
    small = np.zeros((len(p0) - 1, 2), dtype=np.uint32)
    n = C.c_int64(-1)
    rc = lib.gpk_line_polygon_join(sl.device().handle, sr.device().handle, None, 0, 0, None, small.ctypes.data, None, len(small), C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_CAPACITY and n.value == len(p0)
    idx.free()


@pytest.mark.parametrize("kl,kp", [(LS, PG), (MLS, MPG)], ids=["ls-pg", "mls-mpg"])
@pytest.mark.parametrize("line_left", [True, False], ids=["lines-left", "polygons-left"])
def test_join_against_the_brute_force_table(gpk, kl, kp, line_left):
    lines, lv, polys, pv, table = R.join_fixture(kl, kp)
    sl, sp = series(kl, lines, lv), series(kp, polys, pv)
    if line_left:
        _check_join(sl, sp, table, False)
    else:
        _check_join(sp, sl, table, True)


def test_table_join(gpk):
    lines, polys, want = R.known_columns(LS, PG)
    sl, sp = series(LS, lines), series(PG, polys[:2])
    lt = pa.table({"road": pa.array(np.arange(len(lines))), "geometry": sl.device().to_arrow("wkb")})
    rt = pa.table({"district": pa.array(["a", "b"]), "geometry": sp.device().to_arrow("wkb")})
    out = spatial_join_relation(lt, rt, SpatialJoinRelationArgs(predicate="crosses", relation_col="relation"))
    crossing = [i for i, m in enumerate(want) if R.PREDICATES["crosses"](int(m))]
    assert out.column_names == ["road_left", "geometry_left", "district_right", "geometry_right", "relation"]
    assert out.column("road_left").to_pylist() == [i for i in crossing for _ in range(2)]
    assert set(out.column("relation").to_pylist()) == {7}
    left = spatial_join_relation(lt, rt, SpatialJoinRelationArgs(predicate="within", join_type="left", relation_col="relation"))
    inside = [i for i, m in enumerate(want) if R.PREDICATES["within"](int(m))]
    assert left.num_rows == 2 * len(inside) + len(lines) - len(inside)
    assert left.column("relation").null_count == len(lines) - len(inside)
    other = spatial_join_relation(rt, lt, SpatialJoinRelationArgs(predicate="contains"))
    assert sorted(other.column("road_right").to_pylist()) == sorted(i for i in inside for _ in range(2))


# ---- 9. the reference's dispatch arm stays ---------------------------------------------------------------------------------------------------


def test_spatial_join_still_returns_nothing_for_lines_and_polygons(gpk):
    lines, polys, _ = R.known_columns(LS, PG)
    sl, sp = series(LS, lines), series(PG, polys)
    for a, b in ((sl, sp), (sp, sl)):
        pairs, counts = join_pairs(a, b, "intersects")
        assert len(pairs) == 0 and not counts.any()
    assert not sl.intersects(sp).any() and not sl.within(sp).any()
