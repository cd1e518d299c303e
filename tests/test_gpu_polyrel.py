"""GPU: the polygon x polygon relation mask and its join (gpk_polygon_relation / gpk_polygon_relation_join, csrc/gpk_polyrel.hip)
against the exact rational reference (tests/polyrel_ref.py; tests/test_polyrel_ref.py pins it).  Masks and pair sets are compared exactly.

  1. known answers and ties in the four family combinations, as-is and padded with collinear vertices (both lane-group sizes);
  2. placements; 3. random lattice columns, argument swap; 4. agreement with intersects / contains, dwithin at 0 and gpk_spatial_join;
  5. unusable rows and refused calls; 6. the join: seven predicates, count-only, pairs, masks, prebuilt and NULL index, left_row_base,
  capacity (also with a payload buffer, for all five payload joins), device buffers, self-join; 7. the table join; 8. gpk_spatial_join's polygon arms are unchanged."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest
import torch

from geopolars_amd import _abi
from geopolars_amd.geoseries import GeoSeries, polygon_mask_predicate
from geopolars_amd.spatial_index import (
    SpatialIndex,
    SpatialJoinRelationArgs,
    dwithin_pairs,
    join_pairs,
    polygon_relation_pairs,
    polygon_relation_pairs_device,
    spatial_join_polygon_relation,
)
from tests import exact_predicates as E
from tests import exact_ref as X
from tests import polyrel_ref as P
from tests import relation_ref as R

pytestmark = pytest.mark.gpu

PG, MPG = P.PG, P.MPG
FAMILY_IDS = [f"{P.NAMES[a]}-{P.NAMES[b]}" for a, b in P.FAMILIES]
PAD = 7  # collinear vertices put into every ring edge: a 5-coordinate square becomes a 33-coordinate one


def series(kind, rows, validity=None):
    return GeoSeries(X.column(kind, rows, validity))


def lanes_of(a: GeoSeries, b: GeoSeries) -> int:
    """the lane-group size the launch picks (gpk_polyrel.h relation_group_size): 16 when either column has a mean of 32 coordinates a row"""
    mean = lambda s: s.array.n_coords / max(s.array.n_geoms, 1)  # noqa: E731
    return 16 if max(mean(a), mean(b)) >= 32.0 else 4


# ---- 1. known answers and ties ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("pad", [0, PAD], ids=["G4", "G16"])
@pytest.mark.parametrize("ka,kb", P.FAMILIES, ids=FAMILY_IDS)
def test_known_answers_and_ties(gpk, ka, kb, pad):
    for cases in (P.KNOWN, P.TIES):
        a, b, want, names = P.case_columns(cases, ka, kb, pad)
        sa, sb = series(ka, a), series(kb, b)
        assert lanes_of(sa, sb) == (16 if pad else 4)
        got = sa.polygon_relation(sb)
        assert np.array_equal(got, want), [(n, int(g), int(w)) for n, g, w in zip(names, got, want) if g != w]
        assert np.array_equal(sb.polygon_relation(sa), P.swapped(want))
        # b_rows: every row of A against one row of B, and against an unusable one
        one = series(kb, [[], b[0]])
        col = P.masks(ka, a, kb, [b[0]] * len(a))
        assert np.array_equal(sa.polygon_relation(one, other_rows=np.ones(len(a), dtype=np.uint32)), col)
        assert not sa.polygon_relation(one, other_rows=np.zeros(len(a), dtype=np.uint32)).any()
        # the named predicates
        for name, method in (("touches", "touches"), ("overlaps", "overlaps"), ("equals", "geom_equals"), ("contains_properly", "contains_properly"),
                             ("covers", "covers"), ("covered_by", "covered_by"), ("disjoint", "disjoint"), ("crosses", "crosses")):
            exp = np.array([P.PREDICATES[name](int(m)) for m in want])
            assert np.array_equal(getattr(sa, method)(sb), exp), name


def test_fixtures_reach_both_lane_group_sizes(gpk):
    for cases in (P.KNOWN, P.TIES):
        for pad, lanes in ((0, 4), (PAD, 16)):
            a, b, _, _ = P.case_columns(cases, MPG, MPG, pad)
            assert lanes_of(series(MPG, a), series(MPG, b)) == lanes
    A, B, _ = P.random_columns(PG, PG)
    assert lanes_of(series(PG, A), series(PG, B)) == 4
    assert lanes_of(series(PG, [R.padded(PG, r, PAD) for r in A]), series(PG, [R.padded(PG, r, PAD) for r in B])) == 16


def test_ties_through_the_join_refine(gpk):
    """every tie A against every tie B through the join's refine, with masks (full walk) and count-only (early exit), both group sizes"""
    for pad in (0, PAD):
        a, b, _, _ = P.case_columns(P.TIES, MPG, MPG, pad)
        a0, b0, _, _ = P.case_columns(P.TIES, MPG, MPG, 0)
        sa, sb = series(MPG, a), series(MPG, b)
        table = TIE_TABLE.get("t")
        if table is None:
            table = TIE_TABLE["t"] = P.mask_table(MPG, a0, np.ones(len(a0), bool), MPG, b0, np.ones(len(b0), bool))
        for pred, pid in P.PRED_IDS.items():
            p0, c0, m0 = P.expected_pairs(table, pred)
            pairs, counts, masks = polygon_relation_pairs(sa, sb, pred)
            assert np.array_equal(pairs, p0) and np.array_equal(counts, c0) and np.array_equal(masks, m0), (pad, pred)
            n = C.c_int64(-1)
            rc = _abi.lib().gpk_polygon_relation_join(sa.device().handle, sb.device().handle, None, pid, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None)
            assert rc == _abi.GPK_OK and n.value == len(p0), (pad, pred)


TIE_TABLE = {}

# ---- 2. placement ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("offset,scale", R.PLACEMENTS, ids=["utm", "web-mercator", "tiny", "huge"])
def test_placement_does_not_change_the_mask(gpk, offset, scale):
    a, b, want, names = P.case_columns(P.TIES, MPG, MPG)
    sa = series(MPG, [R.placed(MPG, r, offset, scale) for r in a])
    sb = series(MPG, [R.placed(MPG, r, offset, scale) for r in b])
    got = sa.polygon_relation(sb)
    assert np.array_equal(got, want), [(n, int(g), int(w)) for n, g, w in zip(names, got, want) if g != w]


# ---- 3. random lattice columns -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("pad", [0, PAD], ids=["as-is", "padded"])
@pytest.mark.parametrize("ka,kb", P.FAMILIES, ids=FAMILY_IDS)
def test_random_columns(gpk, ka, kb, pad):
    A, B, want = P.random_columns(ka, kb)
    sa, sb = series(ka, [R.padded(ka, r, pad) for r in A]), series(kb, [R.padded(kb, r, pad) for r in B])
    got = sa.polygon_relation(sb)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    assert np.array_equal(sb.polygon_relation(sa), P.swapped(want))


# ---- 4. kernels the project already trusts -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("ka,kb", P.FAMILIES, ids=FAMILY_IDS)
def test_agrees_with_intersects_and_contains(gpk, ka, kb):
    A, B, _ = P.random_columns(ka, kb)
    sa, sb = series(ka, A), series(kb, B)
    m = sa.polygon_relation(sb)
    assert np.array_equal((m & 3) != 0, sa.intersects(sb))
    assert np.array_equal(((m & 1) != 0) & ((m & 8) == 0), sa.contains(sb))
    assert np.array_equal(((m & 1) != 0) & ((m & 4) == 0), sa.within(sb))
    assert np.array_equal((m & 3) != 0, sa.dwithin(sb, 0.0))


def test_intersects_join_agrees_with_dwithin_at_zero_and_spatial_join(gpk):
    left, lv, right, rv, table, _ = P.join_fixture(PG, PG)
    sl, sr = series(PG, left, lv), series(PG, right, rv)
    pairs, counts, _ = polygon_relation_pairs(sl, sr, "intersects")
    d_pairs, d_counts, _ = dwithin_pairs(sl, sr, 0.0)
    j_pairs, j_counts = join_pairs(sl, sr, "intersects")
    assert np.array_equal(pairs, d_pairs) and np.array_equal(counts, d_counts)
    assert np.array_equal(pairs, j_pairs) and np.array_equal(counts, j_counts)
    c_pairs, _ = join_pairs(sl, sr, "contains")
    assert np.array_equal(polygon_relation_pairs(sl, sr, "contains")[0], c_pairs)


# ---- 5. unusable rows and refused calls ------------------------------------------------------------------------------------------------------


def test_unusable_rows_give_mask_zero_and_never_join(gpk):
    nan = float("nan")
    sq = P.S10
    open_ring = [(0, 0), (12, 0), (12, 12), (0, 12)]
    bad = [[], [[(0, 0), (nan, 1), (3, 3), (0, 0)]], [open_ring], [[(0, 0), (5, 0), (0, 0)]], [sq, [(4, 4), (8, 4), (4, 4)]], [sq], [sq], [sq, []]]
    valid = [True, True, True, True, True, False, True, True]
    want = np.array([0, 0, 0, 0, 0, 0, 3, 3], dtype=np.uint8)
    good = [[sq]] * len(bad)
    assert np.array_equal(P.masks(PG, bad, PG, good, av=valid), want)
    sb, sg = series(PG, bad, valid), series(PG, good)
    assert np.array_equal(sb.polygon_relation(sg), want) and np.array_equal(sg.polygon_relation(sb), want)
    mp = [[[], [sq]], [[]], [[sq], [open_ring]], [[sq], []]]
    assert np.array_equal(series(MPG, mp).polygon_relation(series(PG, good[:4])), np.array([3, 0, 0, 3], dtype=np.uint8))
    assert np.array_equal(series(PG, good[:4]).polygon_relation(series(MPG, mp)), np.array([3, 0, 0, 3], dtype=np.uint8))
    rows = np.array([6, 8, 0xFFFFFFFF, 7, 6, 6, 0, 5], dtype=np.uint32)  # an out-of-range entry: mask 0
    assert np.array_equal(sg.polygon_relation(sb, other_rows=rows), np.array([3, 0, 0, 3, 3, 3, 0, 0], dtype=np.uint8))
    for name in ("touches", "overlaps", "geom_equals", "contains_properly", "covers", "covered_by", "disjoint", "crosses"):
        assert not getattr(sb, name)(sg)[:6].any(), name
    for pred in P.PRED_IDS:
        for l, r in ((sb, sg), (sg, sb)):
            pairs, counts, _ = polygon_relation_pairs(l, r, pred)
            rows_in = set(pairs[:, 0 if l is sb else 1].tolist())
            assert rows_in <= {6, 7}, pred


def test_refused_calls(gpk):
    lib = _abi.lib()
    sq = [P.S10]
    sp, sp2, sm = series(PG, [sq] * 3), series(PG, [sq] * 2), series(MPG, [[sq]] * 3)
    sl = GeoSeries(X.column(_abi.GEOM_LINESTRING, [[(1, 1), (3, 2)]] * 3))
    pts = GeoSeries(X.column(_abi.GEOM_POINT, [(1.0, 1.0)] * 3))
    out = np.zeros(3, dtype=np.uint8)
    call = lambda a, b, rows=None: lib.gpk_polygon_relation(a.device().handle, b.device().handle, rows, out.ctypes.data, _abi.MEM_HOST, None)  # noqa: E731
    assert call(sp, sm) == _abi.GPK_OK and (out == 3).all()
    assert call(sp, sp2) == _abi.GPK_ERR_INVALID_ARGUMENT  # row counts differ
    for a, b in ((sp, sl), (sl, sp), (pts, sp), (sm, pts), (sl, sl)):
        assert call(a, b) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    n = C.c_int64(-1)
    join = lambda a, b, pred, idx=None: lib.gpk_polygon_relation_join(a.device().handle, b.device().handle, idx, pred, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None)  # noqa: E731
    for a, b in ((sp, sl), (sl, sm), (pts, sp), (sp, pts)):
        assert join(a, b, 0) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    for pred in (-1, 7, 99):
        assert join(sp, sm, pred) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert join(sp, sl, 99) == _abi.GPK_ERR_INVALID_ARGUMENT  # the error order of gpk_line_polygon_join: the predicate id first
    idx = SpatialIndex(sp2, for_points=False)  # an index over another column
    assert join(sp, sp, 0, idx.handle) == _abi.GPK_ERR_INVALID_ARGUMENT
    idx.free()
    assert join(sp, sm, 5) == _abi.GPK_OK and n.value == 9
    small = np.zeros((8, 2), dtype=np.uint32)
    rc = lib.gpk_polygon_relation_join(sp.device().handle, sm.device().handle, None, 5, 0, None, small.ctypes.data, None, 8, C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_CAPACITY and n.value == 9
    rc = lib.gpk_polygon_relation_join(sp.device().handle, sm.device().handle, None, 5, 0, None, None, None, 8, C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_INVALID_ARGUMENT  # a capacity without a pair buffer
    with pytest.raises(NotImplementedError, match="Point"):
        pts.overlaps(sp)
    with pytest.raises(NotImplementedError):
        sl.touches(sl)


# ---- 6. the join ---------------------------------------------------------------------------------------------------------------------------


def _check_join(sl, sr, table):
    lib = _abi.lib()
    idx = SpatialIndex(sr, for_points=False)
    for pred, pid in P.PRED_IDS.items():
        p0, c0, m0 = P.expected_pairs(table, pred)
        assert len(p0) > 0, pred
        for ix in (None, idx):
            pairs, counts, masks = polygon_relation_pairs(sl, sr, pred, r_index=ix)
            assert np.array_equal(pairs, p0), (pred, len(pairs), len(p0))
            assert np.array_equal(counts, c0) and np.array_equal(masks, m0), pred
        n = C.c_int64(-1)  # count-only: the early-exit form of the refine
        assert lib.gpk_polygon_relation_join(sl.device().handle, sr.device().handle, idx.handle, pid, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_OK
        assert n.value == len(p0), pred
        got = np.zeros((len(p0), 2), dtype=np.uint32)  # pairs without masks: early exit, emitted
        assert lib.gpk_polygon_relation_join(sl.device().handle, sr.device().handle, None, pid, 0, None, got.ctypes.data, None, len(got), C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_OK
        assert np.array_equal(got, p0), pred
    for alias, pred in (("covers", "contains"), ("covered_by", "within")):
        assert np.array_equal(polygon_relation_pairs(sl, sr, alias, r_index=idx)[0], P.expected_pairs(table, pred)[0])
    # device buffers, left_row_base and the capacity error on the largest pair set
    p0, c0, m0 = P.expected_pairs(table, "intersects")
    assert len(p0) > 300 and max(c0.max(), np.bincount(p0[:, 1]).max()) > 250  # the polygon that covers the domain
    counts = torch.full((len(c0),), -1, dtype=torch.int32, device="cuda:0")
    assert polygon_relation_pairs_device(sl.device(), sr.device(), None, "intersects", counts, None) == len(p0)
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy().astype(np.uint32), c0)
    pairs = torch.zeros((len(p0) + 3, 2), dtype=torch.int32, device="cuda:0")
    masks = torch.zeros(len(p0) + 3, dtype=torch.uint8, device="cuda:0")
    assert polygon_relation_pairs_device(sl.device(), sr.device(), idx, "intersects", counts, pairs, masks, left_row_base=1000) == len(p0)
    torch.cuda.synchronize()
    assert np.array_equal(pairs.cpu().numpy().astype(np.uint32)[: len(p0)], p0 + np.array([1000, 0], dtype=np.uint32))
    assert np.array_equal(masks.cpu().numpy()[: len(p0)], m0)
    small = np.zeros((len(p0) - 1, 2), dtype=np.uint32)
    n = C.c_int64(-1)
    rc = lib.gpk_polygon_relation_join(sl.device().handle, sr.device().handle, None, 0, 0, None, small.ctypes.data, None, len(small), C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_CAPACITY and n.value == len(p0)
    idx.free()


@pytest.mark.parametrize("ka,kb", [(PG, PG), (MPG, MPG)], ids=["pg-pg", "mpg-mpg"])
def test_join_against_the_brute_force_table(gpk, ka, kb):
    left, lv, right, rv, table, _ = P.join_fixture(ka, kb)
    _check_join(series(ka, left, lv), series(kb, right, rv), table)


def _payload_join_case(family):
    """(ABI function, left, right, the family's argument, reference pairs, counts and per-pair payload) on the family's join fixture"""
    lib = _abi.lib()
    if family == "polygon_relation":
        left, lv, right, rv, table, _ = P.join_fixture(PG, PG)
        return (lib.gpk_polygon_relation_join, series(PG, left, lv), series(PG, right, rv), P.PRED_IDS["intersects"]) + P.expected_pairs(table, "intersects")
    if family == "line_relation":
        from tests import linerel_ref as L

        left, lv, right, rv, table, _ = L.join_fixture(L.LS, L.LS)
        return (lib.gpk_line_relation_join, series(L.LS, left, lv), series(L.LS, right, rv), L.PRED_IDS["intersects"]) + L.expected_pairs(table, "intersects")
    if family == "line_polygon":
        lines, lnv, polys, pv, table = R.join_fixture(R.LS, R.PG)
        return (lib.gpk_line_polygon_join, series(R.LS, lines, lnv), series(R.PG, polys, pv), R.PRED_IDS["intersects"]) + R.expected_pairs(table, "intersects")
    if family == "intersection_measure":  # the reference of the doubles: the row-wise call, which the join repeats bit for bit
        from tests import overlay_ref as O
        from tests import test_gpu_overlay as OV

        golden = np.load(O.GOLDEN)
        left, right = GeoSeries(O.unpack(golden, "join_left_", PG)), GeoSeries(O.unpack(golden, "join_right_", PG))
        p0, c0, _ = OV.expected(golden["join_area"], len(left), OV.THETA, OV.JOIN_TOL_AREA)
        return lib.gpk_intersection_measure_join, left, right, OV.THETA, p0, c0, OV.rowwise_of_pairs(left, right, PG, p0)
    from tests import dwithin_ref as W  # two non-point columns: the refine that keeps a list behind the distances
    from tests import test_gpu_dwithin as DW

    left, right = W.pair_fixture(*W.PAIR_INSTANCES[0])
    sl, sr = DW.series(left), DW.series(right)
    D = DW.distance_matrix(left, right, sl, sr)
    t = DW.quantile_thresholds(D)[2]
    return (lib.gpk_dwithin_join, sl, sr, t) + DW.expected(D, t)


@pytest.mark.parametrize("family", ["polygon_relation", "line_relation", "line_polygon", "intersection_measure", "dwithin"])
def test_payload_buffer_with_too_small_a_capacity(gpk, family):
    """every join that returns a value per pair, handed a pair buffer AND a payload buffer one element short: the capacity error, the
    exact total and the counts, from host and from device buffers; with the exact capacity the pairs and the payload, bit for bit"""
    fn, sl, sr, arg, p0, c0, v0 = _payload_join_case(family)
    total = len(p0)
    assert total > 1 and v0.dtype in (np.uint8, np.float64)
    lh, rh = sl.device().handle, sr.device().handle
    n = C.c_int64(-1)
    counts = np.full(len(c0), 0xFFFFFFFF, dtype=np.uint32)
    pairs, values = np.zeros((total - 1, 2), dtype=np.uint32), np.zeros(total - 1, dtype=v0.dtype)
    rc = fn(lh, rh, None, arg, 0, counts.ctypes.data, pairs.ctypes.data, values.ctypes.data, total - 1, C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_CAPACITY and n.value == total
    assert np.array_equal(counts, c0)
    d_counts = torch.full((len(c0),), -1, dtype=torch.int32, device="cuda:0")
    d_pairs = torch.zeros((total - 1, 2), dtype=torch.int32, device="cuda:0")
    d_values = torch.zeros(total - 1, dtype=torch.uint8 if v0.dtype == np.uint8 else torch.float64, device="cuda:0")
    n = C.c_int64(-1)
    rc = fn(lh, rh, None, arg, 0, d_counts.data_ptr(), d_pairs.data_ptr(), d_values.data_ptr(), total - 1, C.byref(n), _abi.MEM_DEVICE, None)
    torch.cuda.synchronize()
    assert rc == _abi.GPK_ERR_CAPACITY and n.value == total
    pairs, values = np.zeros((total, 2), dtype=np.uint32), np.zeros(total, dtype=v0.dtype)
    rc = fn(lh, rh, None, arg, 0, counts.ctypes.data, pairs.ctypes.data, values.ctypes.data, total, C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_OK and n.value == total
    assert np.array_equal(pairs, p0) and np.array_equal(counts, c0)
    assert values.dtype == v0.dtype and values.tobytes() == np.ascontiguousarray(v0).tobytes()


@pytest.mark.parametrize("ka", [PG, MPG], ids=["pg", "mpg"])
def test_self_join(gpk, ka):
    left, lv, _, _, _, table = P.join_fixture(ka, ka)
    s = series(ka, left, lv)
    _check_join(s, s, table)
    usable = np.nonzero(table.diagonal())[0]
    for pred, on_diagonal in (("intersects", True), ("equals", True), ("touches", False), ("overlaps", False)):
        pairs = polygon_relation_pairs(s, s, pred)[0]
        diag = pairs[pairs[:, 0] == pairs[:, 1], 0]
        assert np.array_equal(diag, usable if on_diagonal else usable[:0]), pred
    t = polygon_relation_pairs(s, s, "touches")[0]
    assert len(t) and np.array_equal(t[np.lexsort((t[:, 0], t[:, 1]))][:, ::-1], t)  # adjacency is symmetric


# ---- 7. the table join -----------------------------------------------------------------------------------------------------------------------


def test_table_join(gpk):
    a, b, want, _ = P.case_columns(P.TIES, PG, PG)
    sa, sb = series(PG, a), series(PG, b[:2])  # two equal squares on the right
    lt = pa.table({"parcel": pa.array(np.arange(len(a))), "geometry": sa.device().to_arrow("wkb")})
    rt = pa.table({"zone": pa.array(["a", "b"]), "geometry": sb.device().to_arrow("wkb")})
    col = P.masks(PG, a, PG, [b[0]] * len(a))
    out = spatial_join_polygon_relation(lt, rt, SpatialJoinRelationArgs(predicate="touches", relation_col="relation"))
    touching = [i for i, m in enumerate(col) if P.PREDICATES["touches"](int(m))]
    assert touching and out.column_names == ["parcel_left", "geometry_left", "zone_right", "geometry_right", "relation"]
    assert out.column("parcel_left").to_pylist() == [i for i in touching for _ in range(2)]
    assert set(out.column("relation").to_pylist()) == {14}
    left = spatial_join_polygon_relation(lt, rt, SpatialJoinRelationArgs(predicate="equals", join_type="left", relation_col="relation"))
    same = [i for i, m in enumerate(col) if P.PREDICATES["equals"](int(m))]
    assert same and left.num_rows == 2 * len(same) + len(a) - len(same)
    assert left.column("relation").null_count == len(a) - len(same)
    assert set(left.column("relation").drop_null().to_pylist()) == {3}
    other = spatial_join_polygon_relation(rt, lt, SpatialJoinRelationArgs(predicate="overlaps"))
    lapping = [i for i, m in enumerate(col) if P.PREDICATES["overlaps"](int(P.swapped(m)))]
    assert lapping and sorted(other.column("parcel_right").to_pylist()) == sorted(i for i in lapping for _ in range(2))


# ---- 8. the older joins stay ---------------------------------------------------------------------------------------------------------------------


def test_spatial_join_for_polygons_is_unchanged(gpk):
    """gpk_spatial_join's polygon arms against the exact integer predicates of their own golden tests"""
    left, lv, right, rv, table, _ = P.join_fixture(PG, PG)
    sl, sr = series(PG, left, lv), series(PG, right, rv)
    ok_l, ok_r = table.any(axis=1), table.any(axis=0)  # the usable rows
    bl, br = P._boxes(PG, left, ok_l), P._boxes(PG, right, ok_r)
    near = [(i, j) for i in np.nonzero(ok_l)[0] for j in np.nonzero(ok_r & (br[:, 0] <= bl[i, 2]) & (br[:, 2] >= bl[i, 0]) & (br[:, 1] <= bl[i, 3]) & (br[:, 3] >= bl[i, 1]))[0]]
    for pred, f in (("intersects", E.intersects), ("contains", E.contains)):
        want = np.array([(i, j) for i, j in near if f([left[i]], [right[j]])], dtype=np.uint32).reshape(-1, 2)
        pairs, counts = join_pairs(sl, sr, pred)
        assert len(want) > 300 and np.array_equal(pairs, want), pred
        assert np.array_equal(counts, np.bincount(want[:, 0], minlength=len(left)).astype(np.uint32)), pred
