"""GPU: the line x line relation mask and its join (gpk_line_relation / gpk_line_relation_join, csrc/gpk_lineline.hip) against the exact
rational reference (tests/linerel_ref.py; tests/test_linerel_ref.py pins it).  Masks and pair sets are compared exactly.

  1. known answers and ties in the four family combinations, as-is and padded with collinear vertices (both lane-group sizes);
  2. placements; 3. random lattice columns; 4. agreement with dwithin at 0, distance 0 and the dwithin join; 5. unusable rows and
  refused calls; 6. the join: nine predicates, count-only, pairs, masks, prebuilt and NULL index, left_row_base, capacity, device
  buffers, self-join; 7. two rows of hundreds of coordinates; 8. the table join; 9. the older joins stay."""
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
    dwithin_pairs,
    join_pairs,
    line_relation_pairs,
    line_relation_pairs_device,
    relation_pairs,
    spatial_join_line_relation,
)
from tests import exact_predicates as E
from tests import exact_ref as X
from tests import linerel_ref as L
from tests import polyrel_ref as P
from tests import relation_ref as R

pytestmark = pytest.mark.gpu

LS, MLS = L.LS, L.MLS
FAMILY_IDS = [f"{L.NAMES[a]}-{L.NAMES[b]}" for a, b in L.FAMILIES]
PAD = 40  # collinear vertices put into every segment: a 2-coordinate line becomes a 42-coordinate one
NAMED = ("intersects", "disjoint", "touches", "crosses", "overlaps", "within", "contains", "covered_by", "covers", "equals")


def series(kind, rows, validity=None):
    return GeoSeries(X.column(kind, rows, validity))


def lanes_of(a: GeoSeries, b: GeoSeries) -> int:
    """the lane-group size the launch picks (gpk_lineline.h relation_group_size): 16 when either column has a mean of 32 coordinates a row"""
    mean = lambda s: s.array.n_coords / max(s.array.n_geoms, 1)  # noqa: E731
    return 16 if max(mean(a), mean(b)) >= 32.0 else 4


# ---- 1. known answers and ties ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("pad", [0, PAD], ids=["G4", "G16"])
@pytest.mark.parametrize("ka,kb", L.FAMILIES, ids=FAMILY_IDS)
def test_known_answers_and_ties(gpk, ka, kb, pad):
    for cases in (L.KNOWN, L.TIES):
        a, b, want, names = L.case_columns(cases, ka, kb, pad)
        sa, sb = series(ka, a), series(kb, b)
        assert lanes_of(sa, sb) == (16 if pad else 4)
        got = sa.line_relation(sb)
        assert np.array_equal(got, want), [(n, int(g), int(w)) for n, g, w in zip(names, got, want) if g != w]
        assert np.array_equal(sb.line_relation(sa), L.swapped(want))
        # b_rows: every row of A against one row of B, against an unusable one and against an entry out of range
        one = series(kb, [[], b[0]])
        col = L.masks(ka, a, kb, [b[0]] * len(a))
        assert np.array_equal(sa.line_relation(one, other_rows=np.ones(len(a), dtype=np.uint32)), col)
        assert not sa.line_relation(one, other_rows=np.zeros(len(a), dtype=np.uint32)).any()
        assert not sa.line_relation(one, other_rows=np.full(len(a), 2, dtype=np.uint32)).any()
        for name in NAMED:
            exp = np.array([L.PREDICATES[name](int(m)) for m in want])
            assert np.array_equal(sa.line_predicate(sb, name), exp), name


TIE_TABLE = {}


def test_ties_through_the_join_refine(gpk):
    """every tie A against every tie B through the join's refine, with masks (full mask) and count-only (early exit), both group sizes"""
    a0, b0, _, _ = L.case_columns(L.TIES, MLS, MLS, 0)
    table = TIE_TABLE.setdefault("t", L.mask_table(MLS, a0, np.ones(len(a0), bool), MLS, b0, np.ones(len(b0), bool)))
    for pad in (0, PAD):
        a, b, _, _ = L.case_columns(L.TIES, MLS, MLS, pad)
        sa, sb = series(MLS, a), series(MLS, b)
        for pred, pid in L.PRED_IDS.items():
            p0, c0, m0 = L.expected_pairs(table, pred)
            pairs, counts, masks = line_relation_pairs(sa, sb, pred)
            assert np.array_equal(pairs, p0) and np.array_equal(counts, c0) and np.array_equal(masks, m0), (pad, pred)
            n = C.c_int64(-1)
            rc = _abi.lib().gpk_line_relation_join(sa.device().handle, sb.device().handle, None, pid, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None)
            assert rc == _abi.GPK_OK and n.value == len(p0), (pad, pred)


# ---- 2. placement ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("offset,scale", L.PLACEMENTS, ids=["utm", "web-mercator", "tiny", "huge"])
def test_placement_does_not_change_the_mask(gpk, offset, scale):
    a, b, want, names = L.case_columns(L.TIES, MLS, MLS)
    sa = series(MLS, [L.placed(MLS, r, offset, scale) for r in a])
    sb = series(MLS, [L.placed(MLS, r, offset, scale) for r in b])
    got = sa.line_relation(sb)
    assert np.array_equal(got, want), [(n, int(g), int(w)) for n, g, w in zip(names, got, want) if g != w]


# ---- 3. random lattice columns -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("pad", [0, PAD], ids=["as-is", "padded"])
@pytest.mark.parametrize("ka,kb", L.FAMILIES, ids=FAMILY_IDS)
def test_random_columns(gpk, ka, kb, pad):
    A, B, want = L.random_columns(ka, kb)
    assert len(A) == 96
    sa, sb = series(ka, [L.padded(ka, r, pad) for r in A]), series(kb, [L.padded(kb, r, pad) for r in B])
    assert lanes_of(sa, sb) == (16 if pad else 4)
    got = sa.line_relation(sb)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    assert np.array_equal(sb.line_relation(sa), L.swapped(want))


# ---- 4. kernels the project already trusts -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("ka,kb", L.FAMILIES, ids=FAMILY_IDS)
def test_agrees_with_dwithin_and_distance(gpk, ka, kb):
    A, B, _ = L.random_columns(ka, kb)
    sa, sb = series(ka, A), series(kb, B)
    hit = (sa.line_relation(sb) & 31) != 0
    assert np.array_equal(hit, sa.dwithin(sb, 0.0))
    assert np.array_equal(hit, sa.distance(sb) == 0.0)
    if ka == LS:
        assert sa.line_predicate(sa, "equals").all()


def test_intersects_join_agrees_with_dwithin_at_zero(gpk):
    left, lv, right, rv, _, _ = L.join_fixture(LS, LS)
    sl, sr = series(LS, left, lv), series(LS, right, rv)
    pairs, counts, _ = line_relation_pairs(sl, sr, "intersects")
    d_pairs, d_counts, _ = dwithin_pairs(sl, sr, 0.0)
    assert len(pairs) > 300 and np.array_equal(pairs, d_pairs) and np.array_equal(counts, d_counts)
    assert line_relation_pairs(sl, sl, "equals")[0].shape[0] >= 298 and sl.line_predicate(sl, "equals").sum() == 298


# ---- 5. unusable rows and refused calls ------------------------------------------------------------------------------------------------------


def test_unusable_rows_give_mask_zero_and_never_join(gpk):
    nan, inf = float("nan"), float("inf")
    line = [(0, 0), (4, 4)]
    bad = [[], [(0, 0), (nan, 1)], [(0, 0), (1, inf)], [(-inf, 0), (1, 1)], line, line]
    valid = [True, True, True, True, False, True]
    want = np.array([0, 0, 0, 0, 0, 19], dtype=np.uint8)
    good = [line] * len(bad)
    assert np.array_equal(L.masks(LS, bad, LS, good, av=valid), want)
    sb, sg = series(LS, bad, valid), series(LS, good)
    assert np.array_equal(sb.line_relation(sg), want) and np.array_equal(sg.line_relation(sb), want)
    mp = [[[], line], [[]], [[], []], [line, [(1, nan)]], [line, []], []]
    mwant = np.array([19, 0, 0, 0, 19, 0], dtype=np.uint8)
    assert np.array_equal(series(MLS, mp).line_relation(sg), mwant) and np.array_equal(sg.line_relation(series(MLS, mp)), mwant)
    rows = np.array([5, 6, 0xFFFFFFFF, 4, 5, 0], dtype=np.uint32)  # entries out of range: mask 0
    assert np.array_equal(sg.line_relation(sb, other_rows=rows), np.array([19, 0, 0, 0, 19, 0], dtype=np.uint8))
    for name in NAMED:
        assert not sb.line_predicate(sg, name)[:5].any(), name
    for pred in L.PRED_IDS:
        for l, r in ((sb, sg), (sg, sb)):
            pairs, _, _ = line_relation_pairs(l, r, pred)
            assert set(pairs[:, 0 if l is sb else 1].tolist()) <= {5}, pred


def test_refused_calls(gpk):
    lib = _abi.lib()
    line = [(0, 0), (4, 4)]
    sl, sl2, sm = series(LS, [line] * 3), series(LS, [line] * 2), series(MLS, [[line]] * 3)
    sp = GeoSeries(X.column(_abi.GEOM_POLYGON, [[P.S10]] * 3))
    pts = GeoSeries(X.column(_abi.GEOM_POINT, [(1.0, 1.0)] * 3))
    mpt = GeoSeries(X.column(_abi.GEOM_MULTIPOINT, [[(1.0, 1.0)]] * 3))
    out = np.zeros(3, dtype=np.uint8)
    call = lambda a, b, rows=None: lib.gpk_line_relation(a.device().handle, b.device().handle, rows, out.ctypes.data, _abi.MEM_HOST, None)  # noqa: E731
    assert call(sl, sm) == _abi.GPK_OK and (out == 19).all()
    assert call(sl, sl2) == _abi.GPK_ERR_INVALID_ARGUMENT  # row counts differ
    assert lib.gpk_line_relation(sl.device().handle, sm.device().handle, None, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    for a, b in ((sp, sl), (sl, sp), (pts, sl), (sm, pts), (sl, mpt), (sp, sp)):
        assert call(a, b) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    assert call(sp, sl2) == _abi.GPK_ERR_MISMATCHED_GEOMETRY  # the families before the counts
    n = C.c_int64(-1)
    join = lambda a, b, pred, idx=None: lib.gpk_line_relation_join(a.device().handle, b.device().handle, idx, pred, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None)  # noqa: E731
    for a, b in ((sp, sl), (sl, sp), (pts, sl), (sl, pts), (sp, sp)):
        assert join(a, b, 0) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    for pred in (-1, 9, 99):
        assert join(sl, sm, pred) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert join(sp, sl, 99) == _abi.GPK_ERR_INVALID_ARGUMENT  # the predicate id first
    idx = SpatialIndex(sl2, for_points=False)  # an index over another column
    assert join(sl, sl, 0, idx.handle) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert join(sp, sl, 0, idx.handle) == _abi.GPK_ERR_MISMATCHED_GEOMETRY  # the families before the index
    idx.free()
    assert join(sl, sm, 8) == _abi.GPK_OK and n.value == 9
    small = np.zeros((8, 2), dtype=np.uint32)
    rc = lib.gpk_line_relation_join(sl.device().handle, sm.device().handle, None, 8, 0, None, small.ctypes.data, None, 8, C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_CAPACITY and n.value == 9
    rc = lib.gpk_line_relation_join(sl.device().handle, sm.device().handle, None, 8, 0, None, None, None, 8, C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_INVALID_ARGUMENT  # a capacity without a pair buffer
    with pytest.raises(NotImplementedError, match="LineString x LineString"):
        sl.touches(sl)


# ---- 6. the join ---------------------------------------------------------------------------------------------------------------------------


def _check_join(sl, sr, table):
    lib = _abi.lib()
    idx = SpatialIndex(sr, for_points=False)
    for pred, pid in L.PRED_IDS.items():
        p0, c0, m0 = L.expected_pairs(table, pred)
        assert len(p0) > 0, pred
        for ix in (None, idx):
            pairs, counts, masks = line_relation_pairs(sl, sr, pred, r_index=ix)
            assert np.array_equal(pairs, p0), (pred, len(pairs), len(p0))
            assert np.array_equal(counts, c0) and np.array_equal(masks, m0), pred
        n = C.c_int64(-1)  # count-only: the early-exit form of the refine
        assert lib.gpk_line_relation_join(sl.device().handle, sr.device().handle, idx.handle, pid, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_OK
        assert n.value == len(p0), pred
        got = np.zeros((len(p0), 2), dtype=np.uint32)  # pairs without masks: early exit, emitted
        assert lib.gpk_line_relation_join(sl.device().handle, sr.device().handle, None, pid, 0, None, got.ctypes.data, None, len(got), C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_OK
        assert np.array_equal(got, p0), pred
    # device buffers, left_row_base and the capacity error on the largest pair set
    p0, c0, m0 = L.expected_pairs(table, "intersects")
    assert len(p0) > 300
    counts = torch.full((len(c0),), -1, dtype=torch.int32, device="cuda:0")
    assert line_relation_pairs_device(sl.device(), sr.device(), None, "intersects", counts, None) == len(p0)
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy().astype(np.uint32), c0)
    pairs = torch.zeros((len(p0) + 3, 2), dtype=torch.int32, device="cuda:0")
    masks = torch.zeros(len(p0) + 3, dtype=torch.uint8, device="cuda:0")
    assert line_relation_pairs_device(sl.device(), sr.device(), idx, "intersects", counts, pairs, masks, left_row_base=1000) == len(p0)
    torch.cuda.synchronize()
    assert np.array_equal(pairs.cpu().numpy().astype(np.uint32)[: len(p0)], p0 + np.array([1000, 0], dtype=np.uint32))
    assert np.array_equal(masks.cpu().numpy()[: len(p0)], m0)
    small = np.zeros((len(p0) - 1, 2), dtype=np.uint32)
    n = C.c_int64(-1)
    rc = lib.gpk_line_relation_join(sl.device().handle, sr.device().handle, None, 0, 0, None, small.ctypes.data, None, len(small), C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_CAPACITY and n.value == len(p0)
    idx.free()


@pytest.mark.parametrize("ka,kb", [(LS, LS), (MLS, MLS)], ids=["ls-ls", "mls-mls"])
def test_join_against_the_brute_force_table(gpk, ka, kb):
    left, lv, right, rv, table, _ = L.join_fixture(ka, kb)
    _check_join(series(ka, left, lv), series(kb, right, rv), table)


@pytest.mark.parametrize("ka", [LS, MLS], ids=["ls", "mls"])
def test_self_join(gpk, ka):
    left, lv, _, _, _, table = L.join_fixture(ka, ka)
    s = series(ka, left, lv)
    _check_join(s, s, table)
    usable = np.nonzero(table.diagonal())[0]
    for pred, on_diagonal in (("intersects", True), ("equals", True), ("within", True), ("covers", True), ("touches", False), ("crosses", False), ("overlaps", False)):
        pairs = line_relation_pairs(s, s, pred)[0]
        diag = pairs[pairs[:, 0] == pairs[:, 1], 0]
        assert np.array_equal(diag, usable if on_diagonal else usable[:0]), pred
    t = line_relation_pairs(s, s, "touches")[0]
    assert len(t) and np.array_equal(t[np.lexsort((t[:, 0], t[:, 1]))][:, ::-1], t)  # connectivity is symmetric


# ---- 7. rows of hundreds of coordinates ----------------------------------------------------------------------------------------------------


def test_two_long_rows(gpk):
    a, b = L.zigzag_pair()
    want = L.mask(LS, a, LS, b)
    sa, sb = series(LS, [a]), series(LS, [b])
    assert lanes_of(sa, sb) == 16
    assert sa.line_relation(sb)[0] == want and sb.line_relation(sa)[0] == int(L.swapped(want))
    assert sa.line_relation(sa)[0] == 19  # the covering walk over 599 segments


# ---- 8. the table join -----------------------------------------------------------------------------------------------------------------------


def test_table_join(gpk):
    a, b, want, _ = L.case_columns(L.TIES, LS, LS)
    sa, sb = series(LS, a), series(LS, [b[0], b[0]])  # the same line twice on the right
    lt = pa.table({"road": pa.array(np.arange(len(a))), "geometry": sa.device().to_arrow("wkb")})
    rt = pa.table({"name": pa.array(["a", "b"]), "geometry": sb.device().to_arrow("wkb")})
    col = L.masks(LS, a, LS, [b[0]] * len(a))
    out = spatial_join_line_relation(lt, rt, SpatialJoinRelationArgs(predicate="crosses", relation_col="relation"))
    crossing = [i for i, m in enumerate(col) if L.PREDICATES["crosses"](int(m))]
    assert crossing and out.column_names == ["road_left", "geometry_left", "name_right", "geometry_right", "relation"]
    assert out.column("road_left").to_pylist() == [i for i in crossing for _ in range(2)]
    assert out.column("relation").to_pylist() == [int(col[i]) for i in crossing for _ in range(2)]
    left = spatial_join_line_relation(lt, rt, SpatialJoinRelationArgs(predicate="touches", join_type="left", relation_col="relation", l_suffix="_l", r_suffix="_r"))
    touching = [i for i, m in enumerate(col) if L.PREDICATES["touches"](int(m))]
    assert left.column_names == ["road_l", "geometry_l", "name_r", "geometry_r", "relation"]
    assert left.num_rows == 2 * len(touching) + len(a) - len(touching)
    assert left.column("relation").null_count == len(a) - len(touching)


# ---- 9. the older joins stay ---------------------------------------------------------------------------------------------------------------------


def test_older_joins_are_unchanged(gpk):
    """gpk_spatial_join, gpk_line_polygon_join and gpk_dwithin_join against their own references"""
    left, lv, right, rv, table, _ = P.join_fixture(P.PG, P.PG)
    sl, sr = series(P.PG, left, lv), series(P.PG, right, rv)
    ok_l, ok_r = table.any(axis=1), table.any(axis=0)
    bl, br = P._boxes(P.PG, left, ok_l), P._boxes(P.PG, right, ok_r)
    near = [(i, j) for i in np.nonzero(ok_l)[0] for j in np.nonzero(ok_r & (br[:, 0] <= bl[i, 2]) & (br[:, 2] >= bl[i, 0]) & (br[:, 1] <= bl[i, 3]) & (br[:, 3] >= bl[i, 1]))[0]]
    want = np.array([(i, j) for i, j in near if E.intersects([left[i]], [right[j]])], dtype=np.uint32).reshape(-1, 2)
    assert len(want) > 300 and np.array_equal(join_pairs(sl, sr, "intersects")[0], want)
    lines, lnv, polys, pv, lp_table = R.join_fixture(R.LS, R.PG)
    p0, _, m0 = R.expected_pairs(lp_table, "crosses")
    got = relation_pairs(series(R.LS, lines, lnv), series(R.PG, polys, pv), "crosses")
    assert len(p0) and np.array_equal(got[0], p0) and np.array_equal(got[2], m0)
    ll, llv, lr, lrv, ll_table, _ = L.join_fixture(LS, LS)
    assert np.array_equal(dwithin_pairs(series(LS, ll, llv), series(LS, lr, lrv), 0.0)[0], L.expected_pairs(ll_table, "intersects")[0])
