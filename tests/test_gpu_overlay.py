"""GPU: intersection area and length and their join (gpk_intersection_measure / gpk_intersection_measure_join, csrc/gpk_overlay.hip)
against the exact rational reference (tests/overlay_ref.py; tests/test_overlay_ref.py pins it).

Tolerance (include/geopolars_hip.h): area |got - exact| <= 1e-9 * (d_A^2 + d_B^2), length |got - exact| <= 1e-9 * length(L).

  1. the whole fixture, every family pair, both lane-group sizes, at the lattice placement and a georeferenced one; host and device
     outputs, with and without b_rows, an out-of-range entry; 2. symmetry and area(a, a) = gpk_area(a); 3. unusable rows, apart boxes;
  4. 2^20 rectangle pairs (grid wrap); 5. the join; 6. the Python wrappers."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest
import torch

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import (
    SpatialIndex,
    SpatialJoinIntersectionArgs,
    intersection_measure_pairs,
    intersection_measure_pairs_device,
    polygon_relation_pairs,
    spatial_join_intersection,
)
from tests import exact_ref as X
from tests import overlay_ref as O

pytestmark = pytest.mark.gpu

PG, MPG, LS, MLS = O.PG, O.MPG, O.LS, O.MLS
FAMILIES = O.families()
FAMILY_IDS = [f"{w}-{O.NAMES[a]}-{O.NAMES[b]}" for w, a, b in FAMILIES]
TOL = O.REL_TOL
NAN = float("nan")


@pytest.fixture(scope="module")
def golden():
    return np.load(O.GOLDEN)


def series(kind, rows, validity=None):
    return GeoSeries(X.column(kind, rows, validity))


def lanes_of(a: GeoSeries, b: GeoSeries) -> int:
    """the lane-group size the launch picks: from the polygon column's mean coordinate count for lines, from the larger mean for two
    polygon columns; 16 from 32 coordinates a row"""
    mean = lambda s: s.array.n_coords / max(s.array.n_geoms, 1)  # noqa: E731
    m = mean(b) if a.array.geom_type in (LS, MLS) else max(mean(a), mean(b))
    return 16 if m >= 32.0 else 4


def _append(off, v):
    return np.concatenate([off, np.asarray(v, dtype=np.int32)])


def with_rows(col: GeoArrowArray, rings) -> GeoArrowArray:
    """the column with one more single-sequence row per entry of `rings`"""
    for ring in rings:
        xy = np.concatenate([col.xy, np.asarray(ring, dtype=np.float64).reshape(-1, 2)])
        n, k = len(xy), col.geom_type
        if k == LS:
            col = GeoArrowArray(k, xy, geom_offsets=_append(col.geom_offsets, [n]))
            continue
        ro = _append(col.ring_offsets, [n])
        if k in (MLS, PG):
            col = GeoArrowArray(k, xy, geom_offsets=_append(col.geom_offsets, [len(ro) - 1]), ring_offsets=ro)
        else:
            po = _append(col.part_offsets, [len(ro) - 1])
            col = GeoArrowArray(k, xy, geom_offsets=_append(col.geom_offsets, [len(po) - 1]), part_offsets=po, ring_offsets=ro)
    return col


def dense_square(x0, y0, side, step=0.125):
    """a square with a vertex every `step` along its edges (exact in doubles)"""
    t = np.arange(0.0, side, step)
    z, s = np.zeros_like(t), np.full_like(t, side)
    xy = np.concatenate([np.stack([t, z], 1), np.stack([s, t], 1), np.stack([side - t, s], 1), np.stack([z, side - t], 1), [[0.0, 0.0]]])
    return xy + [x0, y0]


N_BALLAST = 4
BALLAST_AREA, BALLAST_LENGTH = 1024.0, 64.0  # the 64-square against the square (16, 16) - (48, 48); the line y = 32 across it


def fixture_columns(golden, what, ka, kb, lanes, offset):
    """(a, b, exact, scale) of a family pair; for 16 lanes a few dense squares are appended, which lift the polygon columns' mean
    coordinate count past 32 (answers in closed form)"""
    key = O.fixture_key(what, ka, kb)
    a, b = O.unpack(golden, key + "a_", ka), O.unpack(golden, key + "b_", kb)
    exact, scale = golden[key + "exact"], golden[key + "scale"]
    if lanes == 16:
        dense = [dense_square(0.0, 0.0, 64.0)] * N_BALLAST
        if what == "area":
            a, b = with_rows(a, dense), with_rows(b, [O.sq(16, 16, 48, 48)] * N_BALLAST)
            exact, scale = np.concatenate([exact, [BALLAST_AREA] * N_BALLAST]), np.concatenate([scale, [2 * 64.0**2 + 2 * 32.0**2] * N_BALLAST])
        else:
            a, b = with_rows(a, [[(-8, 32), (72, 32)]] * N_BALLAST), with_rows(b, dense)
            exact, scale = np.concatenate([exact, [BALLAST_LENGTH] * N_BALLAST]), np.concatenate([scale, [80.0] * N_BALLAST])
    move = lambda c: GeoArrowArray(c.geom_type, c.xy + np.asarray(offset), geom_offsets=c.geom_offsets, part_offsets=c.part_offsets, ring_offsets=c.ring_offsets)  # noqa: E731
    return GeoSeries(move(a)), GeoSeries(move(b)), exact, scale


def measure(a: GeoSeries, b: GeoSeries, rows=None, device=False):
    """gpk_intersection_measure through the C ABI, host or device buffers"""
    n = len(a)
    lib = _abi.lib()
    if not device:
        out = np.full(n, -7.0)
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint32)
        _abi.check(lib.gpk_intersection_measure(a.device().handle, b.device().handle, None if r is None else r.ctypes.data, out.ctypes.data, _abi.MEM_HOST, None))
        return out
    out = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    r = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.uint32).view(np.int32)).cuda()
    _abi.check(lib.gpk_intersection_measure(a.device().handle, b.device().handle, None if r is None else r.data_ptr(), out.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same(got, want, atol):
    """NaN where NaN is wanted, within `atol` elsewhere"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.array_equal(np.isnan(got), np.isnan(want)) and bool((np.abs(got - want)[~np.isnan(want)] <= atol).all())


# the hand rows below span at most 30 units a side: d^2 <= 1800 a row; their lines are at most 40 long
AREA_ATOL, LENGTH_ATOL = TOL * 2 * 1800.0, TOL * 40.0


def assert_close(got, exact, scale, what):
    assert np.isfinite(got).all() and (got >= 0).all(), what
    err = np.abs(got - exact)
    print(what, f"worst |err| / scale = {np.max(err / np.maximum(scale, 1.0)):.2e}")
    bad = np.nonzero(~(err <= TOL * scale))[0]
    assert len(bad) == 0, (what, [(int(i), got[i], exact[i], scale[i]) for i in bad[:5]])


# ---- 1. the fixture --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("placement", ["lattice", "georeferenced"])
@pytest.mark.parametrize("lanes", [4, 16], ids=["G4", "G16"])
@pytest.mark.parametrize("what,ka,kb", FAMILIES, ids=FAMILY_IDS)
def test_fixture_rowwise(gpk, golden, what, ka, kb, lanes, placement):
    offset = (0.0, 0.0) if placement == "lattice" else O.TRANSLATION
    a, b, exact, scale = fixture_columns(golden, what, ka, kb, lanes, offset)
    assert lanes_of(a, b) == lanes
    n = len(a)
    host = measure(a, b)
    assert_close(host, exact, scale, (what, ka, kb, lanes, placement))
    assert np.array_equal(measure(a, b, device=True), host)
    # b_rows: the identity written out, with one entry out of range
    rows = np.arange(n, dtype=np.uint32)
    rows[3] = n + 5
    for device in (False, True):
        got = measure(a, b, rows, device)
        assert np.isnan(got[3]) and np.array_equal(np.delete(got, 3), np.delete(host, 3))
    wrapper = a.intersection_area(b) if what == "area" else a.intersection_length(b)
    assert np.array_equal(wrapper, host)


def test_row_map_pairs_rows_freely(gpk):
    a = series(PG, [[O.S10]] * 4)
    b = series(MPG, [[[O.sq(0, 0, 1, 1)]], [[O.sq(5, 5, 20, 7)]], [[O.sq(-3, -3, 3, 3)], [O.sq(8, 8, 12, 12)]], [[O.sq(20, 20, 30, 30)]]])
    assert same(measure(a, b, [3, 2, 1, 0]), [0.0, 13.0, 10.0, 1.0], AREA_ATOL)
    assert same(measure(a, b, [2, 2, 7, 1], device=True), [13.0, 13.0, NAN, 10.0], AREA_ATOL)
    lines = series(LS, [[(-5, 6), (25, 6)]] * 4)
    assert same(lines.intersection_length(b, other_rows=[0, 1, 2, 3]), [0.0, 15.0, 0.0, 0.0], LENGTH_ATOL)


def test_stride_rows_are_in_both_group_sizes(golden):
    a = O.unpack(golden, "area_pg_pg_a_", PG)
    edges = {int(a.ring_offsets[k + 1] - a.ring_offsets[k]) - 1 for k in range(len(a.ring_offsets) - 1)}
    assert {5, 33, 39} <= edges  # rings of 5 and 33 edges, and the hole of 40 coordinates


# ---- 2. symmetry and the area of a row against itself ------------------------------------------------------------------------------------


@pytest.mark.parametrize("ka,kb", O.AREA_FAMILIES, ids=FAMILY_IDS[:4])
def test_area_symmetry_and_self(gpk, golden, ka, kb):
    a, b, exact, scale = fixture_columns(golden, "area", ka, kb, 4, (0.0, 0.0))
    ab, ba = measure(a, b), measure(b, a)
    assert (np.abs(ab - ba) <= 2 * TOL * scale).all()
    for s in (a, b):
        box = s.bounds()
        d2 = (box[:, 2] - box[:, 0]) ** 2 + (box[:, 3] - box[:, 1]) ** 2
        assert (np.abs(measure(s, s) - s.area()) <= TOL * 2 * d2).all()


# ---- 3. unusable rows and apart boxes ------------------------------------------------------------------------------------------------------


def test_unusable_rows_give_nan_and_apart_boxes_zero(gpk):
    unclosed = [[(0, 0), (4, 0), (4, 4), (0, 4)]]
    rows = [[O.S10], [O.S10], [], unclosed, [O.S10], [O.S10]]
    valid = [True, False, True, True, True, True]
    good = series(PG, [[O.S10]] * 6)
    bad = series(PG, rows, valid)
    want = np.array([100.0, NAN, NAN, NAN, 100.0, 100.0])
    for got in (measure(bad, good), measure(good, bad), measure(bad, good, device=True)):
        assert same(got, want, AREA_ATOL)
    mbad = series(MPG, [[[O.S10]], [[]], [], [[], unclosed], [[], [O.S10]], [[O.S10], [[(20, 20), (24, 20), (24, 24)]]]], valid)
    assert same(measure(mbad, good), [100.0, NAN, NAN, NAN, 100.0, NAN], AREA_ATOL)
    assert same(measure(good, mbad), [100.0, NAN, NAN, NAN, 100.0, NAN], AREA_ATOL)
    lines = series(LS, [[(2, 2), (5, 2)], [(2, 2), (5, 2)], [], [(2, 2), (5, 2)], [(2, 2), (np.nan, 2)], [(2, 2), (np.inf, 2)]], valid)
    assert same(measure(lines, good), [3.0, NAN, NAN, 3.0, NAN, NAN], LENGTH_ATOL)
    assert same(measure(series(LS, [[(2, 2), (5, 2)]] * 6), bad), [3.0, NAN, NAN, NAN, 3.0, 3.0], LENGTH_ATOL)
    mlines = series(MLS, [[[], [(2, 2), (5, 2)]], [[]], [], [[(1, 1)]], [[(2, 2), (5, 2)], [(1, np.nan)]], [[(1, 1), (1, 1)]]])
    assert same(measure(mlines, good), [3.0, NAN, NAN, 0.0, NAN, 0.0], LENGTH_ATOL)
    # strictly apart boxes: exactly +0.0, whatever lies between
    far = series(PG, [[O.sq(10.000001, 0, 20, 10)], [O.sq(0, -20, 10, -1e-9)], [O.sq(40, 40, 50, 50)], [O.sq(-9, -9, -1, -1)], [O.sq(0, 11, 10, 12)], [O.sq(11, 11, 12, 12)]])
    got = measure(good, far)
    assert (got == 0.0).all() and not np.signbit(got).any()
    got = measure(series(LS, [[(30, 30), (40, 45)]] * 6), good)
    assert (got == 0.0).all() and not np.signbit(got).any()


def test_refused_calls(gpk):
    polys, lines, pts = series(PG, [[O.S10]]), series(LS, [[(0, 0), (1, 1)]]), GeoSeries(GeoArrowArray.from_points([[0.0, 0.0]]))
    lib = _abi.lib()
    out = np.zeros(1)
    for a, b in ((polys, lines), (lines, lines), (pts, polys), (polys, pts)):
        rc = lib.gpk_intersection_measure(a.device().handle, b.device().handle, None, out.ctypes.data, _abi.MEM_HOST, None)
        assert rc == _abi.GPK_ERR_MISMATCHED_GEOMETRY
        n = C.c_int64(-1)
        rc = lib.gpk_intersection_measure_join(a.device().handle, b.device().handle, None, 0.0, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None)
        assert rc == _abi.GPK_ERR_MISMATCHED_GEOMETRY and n.value == 0
    rc = lib.gpk_intersection_measure(polys.device().handle, lines.device().handle, None, out.ctypes.data, _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_MISMATCHED_GEOMETRY and "swap the arguments" in _abi.last_error()
    two = series(PG, [[O.S10]] * 2)
    assert lib.gpk_intersection_measure(polys.device().handle, two.device().handle, None, out.ctypes.data, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT


# ---- 4. grid wrap --------------------------------------------------------------------------------------------------------------------------


def test_a_million_rectangle_pairs(gpk):
    """2^20 pairs of axis-aligned integer rectangles: more groups than the grid holds, so every group takes several pairs"""
    n = 1 << 20
    rng = np.random.default_rng(20)

    def rects(lo, w):
        x0, y0 = lo[:, 0], lo[:, 1]
        x1, y1 = x0 + w[:, 0], y0 + w[:, 1]
        xy = np.stack([x0, y0, x1, y0, x1, y1, x0, y1, x0, y0], axis=1).reshape(-1, 2).astype(np.float64)
        off = np.arange(n + 1, dtype=np.int32)
        return GeoSeries(GeoArrowArray(PG, xy, geom_offsets=off, ring_offsets=off * 5)), (x0, y0, x1, y1)

    a, (ax0, ay0, ax1, ay1) = rects(rng.integers(0, 1000, (n, 2)), rng.integers(1, 40, (n, 2)))
    shift = rng.integers(-30, 31, (n, 2))
    b, (bx0, by0, bx1, by1) = rects(np.stack([ax0, ay0], 1) + shift, rng.integers(1, 40, (n, 2)))
    want = np.maximum(0, np.minimum(ax1, bx1) - np.maximum(ax0, bx0)) * np.maximum(0, np.minimum(ay1, by1) - np.maximum(ay0, by0))
    scale = (ax1 - ax0) ** 2 + (ay1 - ay0) ** 2 + (bx1 - bx0) ** 2 + (by1 - by0) ** 2
    got = measure(a, b, device=True)
    assert (want > 0).sum() > n // 4 and (want == 0).sum() > n // 8
    assert (np.abs(got - want) <= TOL * scale).all()
    assert (got[want == 0] <= TOL * scale[want == 0]).all()


# ---- 5. the join -------------------------------------------------------------------------------------------------------------------------

THETA = 0.5


@pytest.fixture(scope="module")
def join_cols(golden):
    left, right, lines = (GeoSeries(O.unpack(golden, f"join_{k}_", kind)) for k, kind in (("left", PG), ("right", PG), ("lines", LS)))
    return left, right, lines


def expected(table, n_left, theta, tol):
    """(pairs, counts, exact) of the pairs whose exact measure exceeds theta — after asserting that none lies within `tol` of it"""
    assert not (np.abs(table[:, 2] - theta) <= tol).any()
    hit = table[table[:, 2] > theta]
    order = np.lexsort((hit[:, 1], hit[:, 0]))
    pairs = hit[order][:, :2].astype(np.uint32)
    return pairs, np.bincount(pairs[:, 0], minlength=n_left).astype(np.uint32), hit[order][:, 2]


def rowwise_of_pairs(left: GeoSeries, right: GeoSeries, kind, pairs):
    """the row-wise measure of every pair: the pairs' left rows as a column of their own, against right[r]"""
    rows = [O.row_parts(left.array, int(l))[0] for l in pairs[:, 0]]
    col = series(kind, [r[0] for r in rows] if kind == LS else rows)
    assert lanes_of(col, right) == lanes_of(left, right)
    return measure(col, right, pairs[:, 1])


# an upper bound of the tolerance of any fixture pair (rows at most 50 lattice units across, lines at most 5 x 36 long): no exact
# measure may lie this close to the threshold
JOIN_TOL_AREA, JOIN_TOL_LENGTH = TOL * 4 * 50.0**2, TOL * 180.0


def pair_tolerance(l: GeoSeries, r: GeoSeries, kind, pairs):
    """the contract's tolerance of every pair: 1e-9 * (d_l^2 + d_r^2), or 1e-9 * length(l)"""
    if kind == LS:
        return TOL * l.euclidean_length()[pairs[:, 0]]
    d2 = lambda b: (b[:, 2] - b[:, 0]) ** 2 + (b[:, 3] - b[:, 1]) ** 2  # noqa: E731
    return TOL * (d2(l.bounds())[pairs[:, 0]] + d2(r.bounds())[pairs[:, 1]])


@pytest.mark.parametrize("what", ["area", "length", "self"])
def test_join_against_the_reference(gpk, golden, join_cols, what):
    left, right, lines = join_cols
    l, r, kind, table, tol = {"area": (left, right, PG, golden["join_area"], JOIN_TOL_AREA), "length": (lines, right, LS, golden["join_length"], JOIN_TOL_LENGTH),
                              "self": (left, left, PG, golden["join_self"], JOIN_TOL_AREA)}[what]
    assert THETA > tol
    pairs0, counts0, exact0 = expected(table, len(l), THETA, tol)
    assert len(pairs0) > 100
    pairs, counts, m = intersection_measure_pairs(l, r, THETA)
    assert np.array_equal(pairs, pairs0) and np.array_equal(counts, counts0)
    assert np.array_equal(m, rowwise_of_pairs(l, r, kind, pairs0))  # bit for bit
    each = pair_tolerance(l, r, kind, pairs0)
    assert (each <= tol).all() and (np.abs(m - exact0) <= each).all()
    if what == "self":
        diag = pairs[:, 0] == pairs[:, 1]
        assert diag.sum() == len(l) and (np.abs(m[diag] - l.area()) <= each[diag]).all()
    # a prebuilt index, and left_row_base
    idx = SpatialIndex(r, for_points=False)
    p2, c2, m2 = intersection_measure_pairs(l, r, THETA, idx, left_row_base=1000)
    assert np.array_equal(p2, pairs0 + np.array([1000, 0], dtype=np.uint32)) and np.array_equal(c2, counts0) and np.array_equal(m2, m)
    lib = _abi.lib()
    # count-only
    n = C.c_int64(-1)
    cnt = np.full(len(l), 9, dtype=np.uint32)
    rc = lib.gpk_intersection_measure_join(l.device().handle, r.device().handle, None, THETA, 0, cnt.ctypes.data, None, None, 0, C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_OK and n.value == len(pairs0) and np.array_equal(cnt, counts0)
    # too small a capacity: the total is reported, the first pairs and measures are there
    cap = 50
    pbuf, mbuf = np.zeros((cap, 2), dtype=np.uint32), np.zeros(cap)
    rc = lib.gpk_intersection_measure_join(l.device().handle, r.device().handle, idx.handle, THETA, 0, None, pbuf.ctypes.data, mbuf.ctypes.data, cap, C.byref(n),
                                           _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_CAPACITY and n.value == len(pairs0)
    # device buffers
    dc = torch.zeros(len(l), dtype=torch.int32, device="cuda")
    dp = torch.zeros((len(pairs0) + 8, 2), dtype=torch.int32, device="cuda")
    dm = torch.zeros(len(pairs0) + 8, dtype=torch.float64, device="cuda")
    h = intersection_measure_pairs_device(l.device(), r.device(), idx, THETA, dc, dp, dm)
    torch.cuda.synchronize()
    assert h == len(pairs0) and np.array_equal(dp.cpu().numpy().view(np.uint32)[:h], pairs0) and np.array_equal(dm.cpu().numpy()[:h], m)
    assert np.array_equal(dc.cpu().numpy().view(np.uint32), counts0)
    assert intersection_measure_pairs_device(l.device(), r.device(), None, THETA, None, None) == len(pairs0)


def test_join_edges(gpk, join_cols):
    left, right, _ = join_cols
    empty = series(PG, [])
    pairs, counts, m = intersection_measure_pairs(left, empty, 0.0)
    assert len(pairs) == 0 and len(m) == 0 and not counts.any() and len(counts) == len(left)
    pairs, counts, m = intersection_measure_pairs(empty, right, 0.0)
    assert len(pairs) == 0 and len(counts) == 0
    other = SpatialIndex(left, for_points=False)  # an index over another array
    with pytest.raises(_abi.GeopolarsHipError) as e:
        intersection_measure_pairs(left, series(PG, [[O.S10]]), 0.0, other)
    assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT and "different array" in str(e.value)


def test_join_at_zero_on_a_fixture_without_touching_pairs(gpk):
    """left: squares of side 10 every 20 units; right: the same moved by (5, 5).  Every pair is box-disjoint or overlaps in a 5 x 5
    square — asserted from the reference — so min_measure = 0 has a determined pair set; it is a subset of the intersects join."""
    k = 12
    lrows = [[O.sq(20 * i, 20 * j, 20 * i + 10, 20 * j + 10)] for i in range(k) for j in range(k)]
    rrows = [[O.sq(20 * i + 5, 20 * j + 5, 20 * i + 15, 20 * j + 15)] for i in range(k) for j in range(k)]
    tol = TOL * 4 * 10.0**2
    for i in (0, 17, k * k - 1):  # (the layout repeats: three left rows against every right row)
        for j, rr in enumerate(rrows):
            (ax0, ay0), (ax1, ay1) = lrows[i][0][0], lrows[i][0][2]
            (bx0, by0), (bx1, by1) = rr[0][0], rr[0][2]
            apart = ax1 < bx0 or bx1 < ax0 or ay1 < by0 or by1 < ay0
            assert apart or O.exact_area(PG, lrows[i], PG, rr) == 25 > tol
            assert apart == (i != j)
    left, right = series(PG, lrows), series(PG, rrows)
    pairs, counts, m = intersection_measure_pairs(left, right, 0.0)
    assert np.array_equal(pairs, np.stack([np.arange(k * k)] * 2, axis=1)) and (counts == 1).all() and (np.abs(m - 25.0) <= tol).all()
    ipairs, _, _ = polygon_relation_pairs(left, right, "intersects")
    assert {tuple(p) for p in pairs} <= {tuple(p) for p in ipairs}


# ---- 6. the table join ---------------------------------------------------------------------------------------------------------------------


def test_table_join_with_the_measure_column(gpk):
    zones = series(PG, [[O.sq(0, 0, 10, 10)], [O.sq(10, 0, 20, 10)], [O.sq(50, 50, 60, 60)]])
    parcels = series(PG, [[O.sq(5, 2, 15, 6)], [O.sq(30, 30, 31, 31)], [O.sq(12, 1, 14, 3)]])
    roads = series(LS, [[(-5, 5), (25, 5)], [(12, -3), (12, 4)]])
    zt = pa.table({"zone": pa.array(["a", "b", "c"]), "geometry": zones.device().to_arrow("wkb")})
    pt = pa.table({"parcel": pa.array([7, 8, 9]), "geometry": parcels.device().to_arrow("wkb")})
    rt = pa.table({"road": pa.array(["r0", "r1"]), "geometry": roads.device().to_arrow("wkb")})
    out = spatial_join_intersection(pt, zt, SpatialJoinIntersectionArgs(min_measure=1.0))
    assert out.column_names == ["parcel_left", "geometry_left", "zone_right", "geometry_right", "measure"]
    assert out.column("parcel_left").to_pylist() == [7, 7, 9] and out.column("zone_right").to_pylist() == ["a", "b", "b"]
    assert out.column("measure").type == pa.float64() and same(out.column("measure").to_pylist(), [20.0, 20.0, 4.0], AREA_ATOL)
    out = spatial_join_intersection(pt, zt, SpatialJoinIntersectionArgs(min_measure=1.0, join_type="left", measure_col="shared"))
    shared = out.column("shared").to_pylist()
    assert out.column("parcel_left").to_pylist() == [7, 7, 8, 9] and shared[2] is None and same(shared[:2] + shared[3:], [20.0, 20.0, 4.0], AREA_ATOL)
    out = spatial_join_intersection(rt, zt, SpatialJoinIntersectionArgs(min_measure=0.5))
    assert out.column("road_left").to_pylist() == ["r0", "r0", "r1"] and out.column("zone_right").to_pylist() == ["a", "b", "b"]
    assert same(out.column("measure").to_pylist(), [10.0, 10.0, 4.0], LENGTH_ATOL)
