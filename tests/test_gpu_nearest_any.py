"""GPU: the any-family nearest join (gpk_nearest_join_any / nearest_pairs_any / spatial_join_nearest for a non-POINT left column).

  1. against the library's own distance, bit for bit, all 36 ordered pairs of families and every refine instance: the matrix D[l, r] of
     gpk_distance_rowwise's per-row kernels (tests/test_gpu_dwithin.distance_matrix), the expected result its argmin sets by double
     equality within max_distance (tests/nearest_any_ref.expected_from_matrix), for max_distance in {inf, a median nearest distance, 0};
  2. against the exact reference on the rows tests/test_nearest_any_host.py proves decided;
  3. a POINT left column: the bytes of gpk_nearest_join;
  4. true ties on integer lattices, max_distance closed, grid cases, the never-matched rules, arguments and capacity, the refine
     kernels past their first pass (the pattern of tests/test_gpu_second_pass.py), determinism, the table join."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest
import torch

from geopolars_amd import _abi
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import (
    SpatialIndex,
    SpatialJoinNearestArgs,
    join_indices,
    nearest_pairs,
    nearest_pairs_any,
    nearest_pairs_any_device,
    spatial_join_nearest,
    take_column,
)
from tests import dwithin_ref as W
from tests import exact_ref as X
from tests import nearest_any_ref as N
from tests import second_pass as SP
from tests.test_gpu_dwithin import distance_matrix, series
from tests.test_gpu_second_pass import _dwithin_fixture, _join_case, cus  # noqa: F401  (cus: the module-scoped CU count fixture)

pytestmark = pytest.mark.gpu

PT, MP, LS, MLS, PG, MPG = W.PT, W.MP, W.LS, W.MLS, W.PG, W.MPG
INF = float("inf")


def _sq(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]


def squares(boxes, valid=None):
    return (PG, [[_sq(*map(float, b))] for b in boxes], valid)


def median_nearest(D):
    with np.errstate(invalid="ignore"):
        best = np.nanmin(np.where(np.isnan(D), np.inf, D), axis=1)
    best = best[np.isfinite(best)]
    assert len(best) > 2
    return float(np.quantile(best, 0.5, method="lower"))


def same(got, want, what=None):
    (gp, gc, gd), (wp, wc, wd) = got, want
    assert np.array_equal(gc, wc), (what, np.nonzero(gc != wc)[0][:8])
    assert np.array_equal(gp, wp), (what, len(gp), len(wp))
    assert SP.same_bits(gd, wd), what


def check_against_matrix(left, right, bounds=None, D=None, sl=None, sr=None):
    """nearest_pairs_any == the argmin sets of the library's own distance matrix, with and without a prebuilt index; returns D"""
    sl, sr = sl or series(left), sr or series(right)
    D = distance_matrix(left, right, sl, sr) if D is None else D
    idx = SpatialIndex(sr, for_points=False)
    for md in bounds if bounds is not None else (INF, median_nearest(D), 0.0):
        want = N.expected_from_matrix(D, md)
        same(nearest_pairs_any(sl, sr, max_distance=md), want, md)
        same(nearest_pairs_any(sl, sr, r_index=idx, max_distance=md), want, (md, "index"))
    idx.free()
    return D


# ---- 1 + 2: every ordered pair of families, every refine instance ------------------------------------------------------------------


def check_exact(key, seed, left, sl, sr):
    rows = N.exact_nearest(N.fixture_table(key, seed), len(left[1]))
    pairs, counts, dist = nearest_pairs_any(sl, sr)
    off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    assert set(np.nonzero(counts)[0].tolist()) == set(rows)  # every usable left row has a pair (the right sides have usable rows)
    for l, (at, best2, decided, lmax) in rows.items():
        got_r, got_d = pairs[off[l]:off[l + 1], 1].tolist(), dist[off[l]:off[l + 1]]
        exact = X.dec_sqrt(best2)
        # the distance contract: 1e-9 of the pair's size (its distance plus its longest segment)
        assert all(X.abs_err(float(d), exact) <= 1e-9 * (float(exact) + lmax) for d in got_d), (key, l, got_d, exact)
        if decided:
            assert got_r == at, (key, l, got_r, at)


@pytest.mark.parametrize("key", W.POINT_FIXTURES, ids=lambda k: f"{k[0]}-G{k[1]}-{'pl' if k[2] else 'pr'}")
def test_point_side_against_own_distance_and_exact_reference(gpk, key):
    left, right = W.point_fixture(*key)
    sl, sr = series(left), series(right)
    assert X.group_size_of((sr if key[2] else sl).array) == key[1]
    check_against_matrix(left, right, sl=sl, sr=sr)
    check_exact(key, None, left, sl, sr)


@pytest.mark.parametrize("key", W.PAIR_INSTANCES, ids=lambda k: f"{k[0]}x{k[1]}-{k[2]}")
def test_non_point_pairs_against_own_distance_and_exact_reference(gpk, key):
    from tests.test_gpu_distance_pairs import pair_group_size

    left, right = W.pair_fixture(*key)
    sl, sr = series(left), series(right)
    assert pair_group_size(sl.array, sr.array) == (8 if key[2] == "g8" else 32)
    check_against_matrix(left, right, sl=sl, sr=sr)
    check_exact(key, 0, left, sl, sr)


# ---- 3: a POINT left column gives gpk_nearest_join's bytes -------------------------------------------------------------------------


@pytest.mark.parametrize("key", [k for k in W.POINT_FIXTURES if k[2]], ids=lambda k: f"{k[0]}-G{k[1]}")
def test_point_left_equals_the_point_entry_point(gpk, key):
    left, right = W.point_fixture(*key)
    sl, sr = series(left), series(right)
    idx = SpatialIndex(sr, for_points=False)
    base = nearest_pairs(sl, sr)
    assert len(base[0]) > 0
    md = float(np.quantile(base[2], 0.5, method="lower"))
    for bound in (None, md, 0.0):
        for ix in (None, idx):
            want, got = nearest_pairs(sl, sr, r_index=ix, max_distance=bound), nearest_pairs_any(sl, sr, r_index=ix, max_distance=bound)
            same(got, want, (bound, ix is not None))
    idx.free()


# ---- 4: true ties --------------------------------------------------------------------------------------------------------------------


def test_true_ties_on_an_integer_lattice(gpk):
    # right: unit squares on a lattice of pitch 4; left squares midway between two and between four of them, a square inside one, one
    # overlapping two, and one next to a single square
    right = squares([(4 * i, 4 * j, 4 * i + 1, 4 * j + 1) for j in range(4) for i in range(4)])
    left = squares([(2, 0, 3, 1), (2, 2, 3, 3), (4.25, 4.25, 4.75, 4.75), (0.5, 0, 4.5, 1), (-3, 0, -2, 1), (10, 6, 11, 7)])
    sl, sr = series(left), series(right)
    pairs, counts, dist = nearest_pairs_any(sl, sr)
    by_row = [pairs[pairs[:, 0] == l, 1].tolist() for l in range(6)]
    assert by_row[0] == [0, 1] and by_row[1] == [0, 1, 4, 5] and by_row[2] == [5] and by_row[3] == [0, 1] and by_row[4] == [0] and by_row[5] == [6, 7, 10, 11]
    assert counts.tolist() == [2, 4, 1, 2, 1, 4]
    want = [1.0, 1.0] + [2.0 ** 0.5] * 4 + [0.0] + [0.0, 0.0] + [2.0] + [2.0 ** 0.5] * 4
    assert dist.tolist() == want
    check_against_matrix(left, right, D=None, sl=sl, sr=sr)
    # a line touching two polygons returns both at 0; segments on the lattice
    lines = (LS, [[(1.0, 0.5), (4.0, 0.5)], [(2.0, 2.0), (3.0, 2.0)], [(4.5, -3.0), (8.5, -3.0)]], None)
    p, c, d = nearest_pairs_any(series(lines), sr)
    assert p.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [2, 1], [2, 2]] and d.tolist() == [0.0, 0.0, 2.0 ** 0.5, 2.0 ** 0.5, 3.0, 3.0]
    check_against_matrix(lines, right)
    check_against_matrix(right, lines)


def test_max_distance_is_closed(gpk):
    right = squares([(3, 0, 4, 1), (10, 0, 11, 1)])
    pts = (PT, [(6.0, 0.5)], None)
    for left in (squares([(0, 0, 1, 1)]), (LS, [[(0.0, 0.0), (1.0, 0.5)]], None), (MP, [[(1.0, 0.5), (-5.0, 0.0)]], None)):
        sl = series(left)
        for sr, at, d in ((series(right), 0, 2.0), (series(pts), 0, 5.0)):
            below = float(np.nextafter(d, 0.0))
            p, c, dist = nearest_pairs_any(sl, sr, max_distance=d)
            assert p.tolist() == [[0, at]] and dist.tolist() == [d] and c.tolist() == [1]
            p, c, dist = nearest_pairs_any(sl, sr, max_distance=below)
            assert len(p) == 0 and c.tolist() == [0] and len(dist) == 0
            p, c, dist = nearest_pairs_any(sl, sr, max_distance=float(np.nextafter(d, INF)))
            assert p.tolist() == [[0, at]]


# ---- grid cases ------------------------------------------------------------------------------------------------------------------------


def test_grid_cases(gpk):
    rng = np.random.default_rng(5)
    # right side on one vertical line: the x axis of the directory has zero extent
    on_line = (LS, [[(3.0, float(y)), (3.0, float(y) + 0.5)] for y in rng.uniform(0, 50, 30)], None)
    left = squares([(x, y, x + 1, y + 2) for x, y in rng.uniform(-40, 40, (40, 2))])
    check_against_matrix(left, on_line)
    one_point = (PT, [(3.0, 8.0)] * 9, None)  # both axes: every right row is the same point, nine ties per left row
    D = check_against_matrix(left, one_point)
    assert (np.nonzero(~np.isnan(D))[0].size) == 40 * 9
    small = squares([(x, y, x + 0.5, y + 0.5) for x, y in rng.uniform(0, 100, (60, 2))])
    # left rows far outside the extent on each side and corner, and one covering all of it
    far = [(-1e6, 50), (1e6, 50), (50, -1e6), (50, 1e6), (-300, -300), (400, 400), (-250, 350), (320, -120), (-1, 50), (101, 50)]
    outside = squares([(x, y, x + 3, y + 3) for x, y in far] + [(-10, -10, 120, 120), (0, 0, 100.5, 100.5)])
    check_against_matrix(outside, small)
    check_against_matrix((LS, [[(x, y), (x + 3.0, y + 1.0)] for x, y in far], None), small)
    # one right row spanning every cell beside small ones (an L-shaped line along two sides of the extent: its box is the extent)
    spanning = (LS, [[(float(x), float(y)), (float(x) + 0.5, float(y))] for x, y in rng.uniform(0, 100, (50, 2))], None)
    spanning[1][7] = [(0.0, 100.0), (0.0, 0.0), (100.0, 0.0)]
    inside = squares([(x, y, x + 1, y + 1) for x, y in rng.uniform(5, 95, (40, 2))])
    check_against_matrix(inside, spanning)
    # a single right row
    check_against_matrix(squares([(x, y, x + 1, y + 1) for x, y in rng.uniform(-50, 50, (6, 2))]), squares([(0, 0, 2, 2)]))


# ---- never matched ---------------------------------------------------------------------------------------------------------------------


def test_null_empty_and_nan_rows(gpk):
    nan = float("nan")
    left = (MP, [[(0.0, 0.0)], [], [(5.0, 5.0), (6.0, 6.0)], [(1.0, 1.0)], [(9.0, 9.0)]], [True, True, True, False, True])
    right = (PT, [(0.0, 1.0), (nan, 2.0), (5.0, 4.0), (3.0, nan), (5.0, 4.0), (100.0, 100.0)], [True, True, True, True, True, False])
    D = check_against_matrix(left, right, bounds=(INF, 1.0, 0.0))
    p, c, d = nearest_pairs_any(series(left), series(right))
    assert p.tolist() == [[0, 0], [2, 2], [2, 4], [4, 2], [4, 4]] and c.tolist() == [1, 0, 2, 0, 2]
    D = check_against_matrix(right, left, bounds=(INF, 1.0, 0.0))
    p, c, d = nearest_pairs_any(series(right), series(left))
    assert c.tolist() == [1, 0, 1, 0, 1, 0] and p[:, 1].tolist() == [0, 2, 2]
    # polygons with a null and an empty row on both sides
    lp = (PG, [[_sq(0.0, 0.0, 1.0, 1.0)], [], [_sq(5.0, 5.0, 6.0, 6.0)]], [True, True, False])
    rl = (MLS, [[[(3.0, 0.0), (3.0, 1.0)]], [], [[(0.5, 0.5), (0.6, 0.6)]], [[(2.0, 0.0), (2.0, 1.0)]]], [True, True, False, True])
    check_against_matrix(lp, rl, bounds=(INF, 0.5))
    p, c, d = nearest_pairs_any(series(lp), series(rl))
    assert p.tolist() == [[0, 3]] and d.tolist() == [1.0] and c.tolist() == [1, 0, 0]
    # an all-empty right side, and empty columns on either side
    empty_right = (LS, [[], []], None)
    p, c, d = nearest_pairs_any(series(lp), series(empty_right))
    assert len(p) == 0 and len(d) == 0 and c.tolist() == [0, 0, 0]
    none = (LS, [], None)
    p, c, d = nearest_pairs_any(series(lp), series(none))
    assert len(p) == 0 and c.tolist() == [0, 0, 0]
    p, c, d = nearest_pairs_any(series(none), series(lp))
    assert len(p) == 0 and len(c) == 0 and len(d) == 0


# ---- arguments, capacity, device buffers ----------------------------------------------------------------------------------------------


def test_arguments_capacity_and_device_buffers(gpk):
    lib = _abi.lib()
    left, right = W.pair_fixture(LS, PG, "g8")
    sl, sr = series(left), series(right)
    D = distance_matrix(left, right, sl, sr)
    md = median_nearest(D)
    p0, c0, d0 = N.expected_from_matrix(D, md)
    assert len(p0) > 2 and (c0 == 0).any()
    call = lambda *a: lib.gpk_nearest_join_any(sl.device().handle, sr.device().handle, *a)  # noqa: E731
    n = C.c_int64(-1)
    counts = np.full(len(c0), 77, np.uint32)
    assert call(None, md, 0, counts.ctypes.data, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_OK  # count-only
    assert n.value == len(p0) and np.array_equal(counts, c0)
    small = np.zeros((len(p0) - 1, 2), np.uint32)
    n.value = -1
    assert call(None, md, 0, None, small.ctypes.data, None, len(small), C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_CAPACITY
    assert n.value == len(p0)
    for bad in (-1.0, float("nan"), -INF):
        n.value = -1
        assert call(None, bad, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT and n.value == 0
    assert call(None, md, 0, None, None, None, 4, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT  # capacity without pairs
    wrong = SpatialIndex(sl, for_points=False)  # an index of another column
    assert call(wrong.handle, md, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    wrong.free()
    # device buffers == host buffers, with left_row_base
    idx = SpatialIndex(sr, for_points=False)
    dc = torch.full((len(c0),), -1, dtype=torch.int32, device="cuda:0")
    assert nearest_pairs_any_device(sl.device(), sr.device(), None, dc, None, max_distance=md) == len(p0)
    torch.cuda.synchronize()
    assert np.array_equal(dc.cpu().numpy().astype(np.uint32), c0)
    dp = torch.zeros((len(p0) + 3, 2), dtype=torch.int32, device="cuda:0")
    dd = torch.full((len(p0) + 3,), -1.0, dtype=torch.float64, device="cuda:0")
    assert nearest_pairs_any_device(sl.device(), sr.device(), idx, dc, dp, dd, max_distance=md, left_row_base=1000) == len(p0)
    torch.cuda.synchronize()
    assert np.array_equal(dp.cpu().numpy().astype(np.uint32)[: len(p0)], p0 + np.array([1000, 0], dtype=np.uint32))
    assert SP.same_bits(dd.cpu().numpy()[: len(p0)], d0) and (dd.cpu().numpy()[len(p0):] == -1.0).all()
    hp, hc, hd = nearest_pairs_any(sl, sr, r_index=idx, max_distance=md, left_row_base=1000)
    assert np.array_equal(hp, p0 + np.array([1000, 0], dtype=np.uint32)) and np.array_equal(hc, c0) and SP.same_bits(hd, d0)
    idx.free()


def test_two_calls_give_identical_bytes(gpk):
    for key in ((MLS, MPG, "g8"), (PG, LS, "g32"), (MPG, MLS, "large")):
        left, right = W.pair_fixture(*key)
        sl, sr = series(left), series(right)
        a, b = nearest_pairs_any(sl, sr), nearest_pairs_any(sl, sr)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a[0]) > 0


# ---- past the first pass: more candidates than the refine grids take in one trip ------------------------------------------------------


def _tiled_case(cus, key, G, cap_mult=32, per_block=None, seed=300):
    """a dwithin_ref fixture with its left column tiled past the cap (device_info() sizes it): the expected pairs, counts and distances
    are those of the base columns' distance matrix, gathered with the tiling's order"""
    if not isinstance(key[0], str) and key[2] == "g8":
        # a nearest join returns about one pair per left row: three of the small fixtures (three seeds) joined into one, so that a refine
        # group meets more different pairs in a row than one fixture's seven
        parts = [W.pair_fixture(*key, seed=s) for s in (0, 1, 2)]
        left = (key[0], [r for p in parts for r in p[0][1]], [v for p in parts for v in p[0][2]])
        right = (key[1], [r for p in parts for r in p[1][1]], [v for p in parts for v in p[1][2]])
    else:
        left, right, _ = _dwithin_fixture(key)
    a, b = W.columns(left, right)
    sr = GeoSeries(b)
    D = distance_matrix(left, right, GeoSeries(a), sr)
    p0, c0, d0 = N.expected_from_matrix(D, INF)
    assert len(p0) >= 6
    same(nearest_pairs_any(GeoSeries(a), sr), (p0, c0, d0), key)
    order, pairs, counts, src = _join_case(cus, G, p0, len(a), seed, cap_mult, per_block)
    tiled = GeoSeries(a.take(order))
    got_p, got_c, got_d = nearest_pairs_any(tiled, sr)
    assert np.array_equal(got_c, counts) and np.array_equal(got_p, pairs) and SP.same_bits(got_d, d0[src])
    return tiled.array, b, len(pairs)


@pytest.mark.parametrize("size,G", [("g8", 8), ("g32", 32)])
def test_pair_refine_past_its_first_pass(gpk, cus, size, G):
    from tests.test_gpu_distance_pairs import pair_group_size

    a, b, n_pairs = _tiled_case(cus, (LS, PG, size), G)
    assert n_pairs > cus * 32 * (256 // G) and pair_group_size(a, b) == G


@pytest.mark.parametrize("family,G", [("linestring", 1), ("polygon", 8), ("multipolygon", 32)])
def test_point_refine_past_its_first_pass(gpk, cus, family, G):
    """(the POINT column on the left: the lane-group size comes from the right column, which the tiling leaves alone)"""
    key = (family, G, True)
    assert key in W.POINT_FIXTURES
    a, b, n_pairs = _tiled_case(cus, key, G, seed=310)
    assert n_pairs > cus * 32 * (256 // G) and X.group_size_of(b) == G


def test_large_list_past_its_first_pass(gpk, cus):
    """every pair of the fixture costs more than PD_LARGE_COST: seeds and candidates are all listed for the cus * 4 work-groups"""
    from tests.test_gpu_distance_pairs import row_coords

    left, right, _ = _dwithin_fixture((MLS, MPG, "large"))
    assert min(row_coords(MLS, x) for x in left[1]) * min(row_coords(MPG, y) for y in right[1]) > W.LARGE_COST
    a, b, n_pairs = _tiled_case(cus, (MLS, MPG, "large"), 32, cap_mult=4, per_block=1, seed=320)
    assert n_pairs > cus * 4 * 1


# ---- table level -----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", [PG, LS], ids=["polygons", "lines"])
@pytest.mark.parametrize("how", ["inner", "left"])
def test_spatial_join_nearest_over_tables(gpk, how, kind):
    left, right = W.pair_fixture(kind, MLS, "g8")
    la, ra = W.columns(left, right)
    lt = pa.table({"id": pa.array(np.arange(len(la))), "geometry": la.to_arrow_wkb()})
    rt = pa.table({"name": pa.array([f"r{i}" for i in range(len(ra))]), "geometry": ra.to_arrow_wkb()})
    lgeo, rgeo = GeoSeries.from_arrow(lt.column("geometry")), GeoSeries.from_arrow(rt.column("geometry"))
    base = nearest_pairs_any(lgeo, rgeo)
    md = float(np.quantile(base[2], 0.5, method="lower"))
    pairs, counts, dist = nearest_pairs_any(lgeo, rgeo, max_distance=md)
    assert 0 < len(pairs) < len(base[0]) and 0 < np.count_nonzero(counts == 0) < len(la)
    li, ri = join_indices(counts, pairs, how)
    t = spatial_join_nearest(lt, rt, SpatialJoinNearestArgs(join_type=how, max_distance=md, distance_col="dist"))
    assert t.column_names == ["id_left", "geometry_left", "name_right", "geometry_right", "dist"] and t.num_rows == len(li)
    assert t.column("id_left").combine_chunks().equals(take_column(lt.column("id"), li))
    assert t.column("name_right").combine_chunks().equals(take_column(rt.column("name"), ri))
    d = t.column("dist").combine_chunks()
    assert d.null_count == np.count_nonzero(ri < 0) and (how == "inner") == (d.null_count == 0)
    assert SP.same_bits(np.asarray(d.drop_null()), dist)
    t = spatial_join_nearest(lt, rt, SpatialJoinNearestArgs(join_type=how))
    assert t.column_names == ["id_left", "geometry_left", "name_right", "geometry_right"]
    assert t.num_rows == int(base[1].sum()) + (np.count_nonzero(base[1] == 0) if how == "left" else 0)
