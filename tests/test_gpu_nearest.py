"""GPU: nearest-neighbour join (gpk_nearest_join / spatial_index.nearest_pairs / spatial_join_nearest).

Hand-written known answers (ties, boundaries, mirror images, nulls, max_distance), parity with a brute-force CPU oracle for every
right-side family, self-consistency with the row-wise distance, the search's edge cases and the table-level join."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest
import torch

from geopolars_amd import _abi, synth
from geopolars_amd.geoarrow import DeviceGeoArray, GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import (
    SpatialIndex,
    SpatialJoinNearestArgs,
    join_indices,
    nearest_pairs,
    nearest_pairs_device,
    spatial_join_nearest,
    take_column,
)

pytestmark = pytest.mark.gpu


def _lines(lines, validity=None):
    a = GeoArrowArray.from_linestrings(lines) if lines else GeoArrowArray(_abi.GEOM_LINESTRING, np.zeros((0, 2)), geom_offsets=np.zeros(1, np.int32))
    if validity is not None:
        a.validity = np.packbits(np.asarray(validity, dtype=bool), bitorder="little")
    return a


def _pts(xy, validity=None):
    a = GeoArrowArray.from_points(np.asarray(xy, dtype=np.float64))
    if validity is not None:
        a.validity = np.packbits(np.asarray(validity, dtype=bool), bitorder="little")
    return a


def _near(left, right, **kw):
    return nearest_pairs(GeoSeries(left), GeoSeries(right), **kw)


# ---- known answers ---------------------------------------------------------------------------------------------------------------


def test_point_equidistant_from_two_linestrings_gets_both(gpk):
    pairs, counts, dist = _near(_pts([[0.0, 0.0]]), _lines([[(-1.0, 1.0), (1.0, 1.0)], [(5.0, 5.0), (6.0, 5.0)], [(-1.0, -1.0), (1.0, -1.0)]]))
    assert pairs.tolist() == [[0, 0], [0, 2]] and counts.tolist() == [2]
    assert dist.tolist() == [1.0, 1.0]


def test_point_inside_two_overlapping_polygons_gets_both_at_zero(gpk):
    sq = lambda x0, y0, s: [[(x0, y0), (x0 + s, y0), (x0 + s, y0 + s), (x0, y0 + s)]]
    polys = GeoArrowArray.from_polygons([sq(0, 0, 4), sq(10, 10, 1), sq(1, 1, 4)])
    pairs, counts, dist = _near(_pts([[2.0, 2.0], [10.5, 10.5]]), polys)
    assert pairs.tolist() == [[0, 0], [0, 2], [1, 1]] and counts.tolist() == [2, 1]
    assert dist.tolist() == [0.0, 0.0, 0.0]


def test_point_on_a_polygon_boundary_is_at_zero(gpk):
    polys = GeoArrowArray.from_polygons([[[(3.0, 0.0), (4.0, 0.0), (4.0, 1.0), (3.0, 1.0)]], [[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]]])
    pairs, counts, dist = _near(_pts([[0.0, 0.5], [1.0, 1.0]]), polys)
    assert pairs.tolist() == [[0, 1], [1, 1]] and dist.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("q", [(0.0, 0.0), (2.5, -1.25)])
def test_mirror_images_are_exact_ties(gpk, q):
    """one segment / point / triangle and its three reflections about the query point (dyadic offsets: every difference is exact,
    the arithmetic of the four copies differs only in signs): all four are returned, at one distance"""
    qx, qy = q
    refl = [(1, 1), (-1, 1), (1, -1), (-1, -1)]
    seg = [(1.25, 2.0), (3.0, 0.5)]
    lines = [[(qx + sx * x, qy + sy * y) for x, y in seg] for sx, sy in refl]
    pairs, counts, dist = _near(_pts([q]), _lines(lines))
    assert counts.tolist() == [4] and pairs[:, 1].tolist() == [0, 1, 2, 3] and len(set(dist.tolist())) == 1
    pts_r = _pts([(qx + sx * 0.75, qy + sy * 1.5) for sx, sy in refl])
    pairs, counts, dist = _near(_pts([q]), pts_r)
    assert counts.tolist() == [4] and len(set(dist.tolist())) == 1
    tri = [(1.0, 1.0), (3.0, 1.5), (2.0, 2.75)]
    polys = GeoArrowArray.from_polygons([[[(qx + sx * x, qy + sy * y) for x, y in tri]] for sx, sy in refl])
    pairs, counts, dist = _near(_pts([q]), polys)
    assert counts.tolist() == [4] and len(set(dist.tolist())) == 1 and dist[0] > 0


def test_null_empty_and_nan_left_rows_never_match(gpk):
    left = _pts([[0.0, 0.0], [0.5, 0.5], [np.nan, np.nan], [np.nan, 1.0], [1.0, 1.0]], validity=[1, 0, 1, 1, 1])
    pairs, counts, dist = _near(left, _lines([[(0.0, 0.0), (2.0, 2.0)]]))
    assert counts.tolist() == [1, 0, 0, 0, 1]
    assert pairs.tolist() == [[0, 0], [4, 0]]


def test_null_and_empty_right_rows_are_never_candidates(gpk):
    lines = [[(0.0, 0.0), (1.0, 0.0)], [], [(50.0, 50.0), (51.0, 50.0)], [(0.0, 0.1), (1.0, 0.1)]]
    right = _lines(lines, validity=[0, 1, 1, 0])
    pairs, counts, dist = _near(_pts([[0.5, 0.0], [0.0, 0.0]]), right)
    assert pairs.tolist() == [[0, 2], [1, 2]] and counts.tolist() == [1, 1]


def test_all_empty_right_side_gives_no_pairs(gpk):
    for right in (_lines([[], []]), _lines([[(0.0, 0.0), (1.0, 1.0)]], validity=[0]), _lines([])):
        pairs, counts, dist = _near(_pts([[0.0, 0.0], [3.0, 4.0]]), right)
        assert len(pairs) == 0 and counts.tolist() == [0, 0] and len(dist) == 0


def test_max_distance_is_a_closed_bound(gpk):
    left, right = _pts([[0.0, 0.0], [10.0, 0.0]]), _lines([[(0.3, 0.4), (0.3, 5.0)], [(10.0, 7.0), (11.0, 7.0)]])
    _, _, dist = _near(left, right)
    d0 = dist[0]
    pairs, counts, _ = _near(left, right, max_distance=d0)
    assert pairs.tolist() == [[0, 0]] and counts.tolist() == [1, 0]
    pairs, counts, _ = _near(left, right, max_distance=np.nextafter(d0, 0.0))
    assert len(pairs) == 0 and counts.tolist() == [0, 0]
    pairs, counts, _ = _near(left, right, max_distance=float("inf"))
    assert counts.tolist() == [1, 1]


def test_bad_arguments_are_refused_by_the_library(gpk):
    lib = _abi.lib()
    left, right = GeoSeries(_pts([[0.0, 0.0]])), GeoSeries(_lines([[(0.0, 0.0), (1.0, 1.0)]]))
    n = C.c_int64(0)
    for md in (-1.0, float("nan")):
        assert lib.gpk_nearest_join(left.device().handle, right.device().handle, None, md, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    rc = lib.gpk_nearest_join(right.device().handle, left.device().handle, None, float("inf"), 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    other = SpatialIndex(GeoSeries(_lines([[(0.0, 0.0), (1.0, 1.0)], [(2.0, 2.0), (3.0, 3.0)]])), for_points=False)
    rc = lib.gpk_nearest_join(left.device().handle, right.device().handle, other.handle, float("inf"), 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_INVALID_ARGUMENT


# ---- parity with a brute-force oracle ------------------------------------------------------------------------------------------


def _multipoints(n, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(1, 6, n)
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum(k)
    centers = np.repeat(rng.uniform(0, synth.DOMAIN, (n, 2)), k, axis=0)
    return GeoArrowArray(_abi.GEOM_MULTIPOINT, centers + rng.normal(0, 5.0, (int(off[-1]), 2)), geom_offsets=off)


def _multilines(n, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(1, 4, n)
    go = np.zeros(n + 1, np.int32)
    go[1:] = np.cumsum(k)
    ls = synth.random_linestrings(int(go[-1]), seed=seed, max_log2=5.0)
    return GeoArrowArray(_abi.GEOM_MULTILINESTRING, ls.xy, geom_offsets=go, ring_offsets=ls.geom_offsets)


RIGHTS = {
    "point": lambda: synth.uniform_points(1000, seed=11),
    "multipoint": lambda: _multipoints(1000, 12),
    "linestring": lambda: synth.random_linestrings(1000, seed=13),
    "multilinestring": lambda: _multilines(1000, 14),
    "polygon": lambda: synth.clustered_polygons(1000, seed=15),
    "multipolygon": lambda: synth.powerlaw_multipolygons(1000, seed=16, cap=2000),
}


def _row_sizes(a: GeoArrowArray) -> np.ndarray:
    """coordinates per row (0 = empty)"""
    if a.geom_type == _abi.GEOM_POINT:
        return (~np.isnan(a.xy).any(axis=1)).astype(np.int64)
    off = a.geom_offsets.astype(np.int64)
    for inner in (a.part_offsets, a.ring_offsets):
        if inner is not None:
            off = inner.astype(np.int64)[off]
    return np.diff(off)


def _oracle_matrix(oracle, left: GeoArrowArray, right: GeoArrowArray) -> np.ndarray:
    """distance of every (l, r) by the CPU oracle; inf where r is null or empty (never a candidate)"""
    nl, nr = len(left), len(right)
    rep = GeoArrowArray.from_points(np.repeat(left.xy, nr, axis=0))
    d = oracle.distance_rowwise(rep, right, b_rows=np.tile(np.arange(nr, dtype=np.uint32), nl)).reshape(nl, nr)
    d[:, ~(right.is_valid() & (_row_sizes(right) > 0))] = np.inf
    return d


def _check_against_oracle(D, pairs, counts, dist, rel=1e-9):
    nl = D.shape[0]
    assert np.array_equal(np.bincount(pairs[:, 0].astype(np.int64), minlength=nl), counts.astype(np.int64))
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    assert np.array_equal(order, np.arange(len(pairs))), "pairs are sorted by (l, r)"
    best = D.min(axis=1)
    srt = np.sort(D, axis=1)
    second = srt[:, 1] if D.shape[1] > 1 else np.full(nl, np.inf)
    starts = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    for l in range(nl):
        got_r = pairs[starts[l] : starts[l + 1], 1].astype(np.int64)
        if not np.isfinite(best[l]):
            assert len(got_r) == 0
            continue
        assert len(got_r) >= 1, l
        gmin = dist[starts[l]]
        assert np.all(dist[starts[l] : starts[l + 1]] == gmin)
        assert (gmin == 0.0) == (best[l] == 0.0), (l, gmin, best[l])
        assert abs(gmin - best[l]) <= rel * max(abs(best[l]), 1e-300), (l, gmin, best[l])
        assert np.all(np.abs(D[l, got_r] - best[l]) <= rel * max(abs(best[l]), 1e-300)), l
        if second[l] > best[l] * (1.0 + 1e-6) and second[l] - best[l] > 1e-300:
            assert got_r.tolist() == [int(np.argmin(D[l]))], l


@pytest.mark.parametrize("family", list(RIGHTS))
def test_parity_with_brute_force_oracle(gpk, oracle, family):
    right = RIGHTS[family]()
    left = synth.uniform_points(2000, seed=21)
    pairs, counts, dist = _near(left, right)
    _check_against_oracle(_oracle_matrix(oracle, left, right), pairs, counts, dist)


@pytest.mark.parametrize("family", list(RIGHTS))
def test_distances_equal_rowwise_distance_bit_for_bit(gpk, family):
    right = GeoSeries(RIGHTS[family]())
    left = synth.uniform_points(2000, seed=22)
    pairs, counts, dist = nearest_pairs(GeoSeries(left), right)
    assert len(pairs) >= len(left)
    taken = GeoSeries(GeoArrowArray.from_points(left.xy[pairs[:, 0]]))
    rw = taken.distance(right, other_rows=pairs[:, 1])
    assert np.array_equal(rw.view(np.uint64), dist.view(np.uint64))


# ---- the search's edge cases ------------------------------------------------------------------------------------------------------


def test_points_far_outside_the_extent(gpk, oracle):
    right = synth.star_polygons(50, 16)
    far = 1e6 * synth.DOMAIN
    rng = np.random.default_rng(5)
    ang = rng.uniform(0, 2 * np.pi, 64)
    xy = np.stack([synth.DOMAIN / 2 + far * np.cos(ang), synth.DOMAIN / 2 + far * np.sin(ang)], axis=1)
    xy = np.concatenate([xy, [[-far, 500.0], [far, -far], [500.0, far]]])
    left = _pts(xy)
    pairs, counts, dist = _near(left, right)
    _check_against_oracle(_oracle_matrix(oracle, left, right), pairs, counts, dist)


def test_right_side_clustered_in_one_corner_of_a_large_extent(gpk, oracle):
    ls = synth.random_linestrings(300, seed=31, domain=10.0, max_log2=4.0)
    lines = [ls.xy[ls.geom_offsets[i] : ls.geom_offsets[i + 1]].tolist() for i in range(len(ls))] + [[(1e4, 1e4), (1e4 + 1.0, 1e4)]]
    right = _lines(lines)
    left = _pts(np.concatenate([np.random.default_rng(3).uniform(0, 20.0, (500, 2)), np.random.default_rng(4).uniform(0, 1e4, (500, 2))]))
    pairs, counts, dist = _near(left, right)
    _check_against_oracle(_oracle_matrix(oracle, left, right), pairs, counts, dist)


def test_a_long_linestring_spanning_the_grid_is_returned_once(gpk, oracle):
    ls = synth.random_linestrings(400, seed=41, max_log2=4.0)
    lines = [ls.xy[ls.geom_offsets[i] : ls.geom_offsets[i + 1]].tolist() for i in range(len(ls))]
    lines.insert(7, [(0.0, 0.0), (synth.DOMAIN, synth.DOMAIN)])
    right = _lines(lines)
    t = np.random.default_rng(6).uniform(0, synth.DOMAIN, 1000)
    left = _pts(np.stack([t, t + np.random.default_rng(7).normal(0, 0.5, 1000)], axis=1))
    pairs, counts, dist = _near(left, right)
    assert len(np.unique(pairs, axis=0)) == len(pairs)
    assert np.count_nonzero(pairs[:, 1] == 7) > 500
    _check_against_oracle(_oracle_matrix(oracle, left, right), pairs, counts, dist)


def test_single_right_geometry(gpk):
    left = synth.uniform_points(3000, seed=8)
    pairs, counts, dist = _near(left, synth.star_polygons(1, 32))
    assert counts.tolist() == [1] * 3000 and pairs[:, 1].tolist() == [0] * 3000 and pairs[:, 0].tolist() == list(range(3000))


def test_left_row_base_index_and_output_spaces(gpk):
    right = GeoSeries(synth.random_linestrings(2000, seed=51))
    left_h = synth.uniform_points(5000, seed=52)
    left = GeoSeries(left_h)
    p0, c0, d0 = nearest_pairs(left, right)
    idx = SpatialIndex(right, for_points=False)
    p1, c1, d1 = nearest_pairs(left, right, r_index=idx, left_row_base=1000)
    assert np.array_equal(c0, c1) and np.array_equal(d0, d1)
    assert np.array_equal(p1[:, 0], p0[:, 0] + 1000) and np.array_equal(p1[:, 1], p0[:, 1])
    # device buffers (torch tensors), with and without a prebuilt index
    dl = DeviceGeoArray.upload(left_h)
    for ix in (idx, None):
        counts = torch.empty(len(left_h), dtype=torch.int32, device="cuda:0")
        pairs = torch.empty((len(p0) + 10, 2), dtype=torch.int32, device="cuda:0")
        dist = torch.empty(len(p0) + 10, dtype=torch.float64, device="cuda:0")
        h = nearest_pairs_device(dl, right.device(), ix, counts, pairs, dist)
        torch.cuda.synchronize()
        assert h == len(p0)
        assert np.array_equal(counts.cpu().numpy().astype(np.uint32), c0)
        assert np.array_equal(pairs[:h].cpu().numpy().astype(np.uint32), p0)
        assert np.array_equal(dist[:h].cpu().numpy(), d0)
    # count only
    counts = torch.empty(len(left_h), dtype=torch.int32, device="cuda:0")
    assert nearest_pairs_device(dl, right.device(), None, counts, None) == len(p0)
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy().astype(np.uint32), c0)


def test_count_only_and_capacity(gpk):
    lib = _abi.lib()
    left, right = GeoSeries(synth.uniform_points(3000, seed=61)), GeoSeries(synth.clustered_polygons(500, seed=62))
    p0, c0, _ = nearest_pairs(left, right)
    n = C.c_int64(-1)
    counts = np.zeros(len(left), np.uint32)
    assert lib.gpk_nearest_join(left.device().handle, right.device().handle, None, float("inf"), 0, counts.ctypes.data, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_OK
    assert n.value == len(p0) and np.array_equal(counts, c0)
    small = np.zeros((len(p0) - 1, 2), np.uint32)
    n.value = -1
    rc = lib.gpk_nearest_join(left.device().handle, right.device().handle, None, float("inf"), 0, None, small.ctypes.data, None, len(small), C.byref(n), _abi.MEM_HOST, None)
    assert rc == _abi.GPK_ERR_CAPACITY and n.value == len(p0)


# ---- table level -----------------------------------------------------------------------------------------------------------------


def _struct_coords(xy):
    return pa.StructArray.from_arrays([pa.array(xy[:, 0]), pa.array(xy[:, 1])], ["x", "y"])


@pytest.mark.parametrize("how", ["inner", "left"])
def test_spatial_join_nearest_over_tables(gpk, how):
    right = synth.random_linestrings(500, seed=71)
    left = synth.uniform_points(3000, seed=72)
    lt_wkb = pa.table({"id": pa.array(np.arange(len(left))), "geometry": left.to_arrow_wkb()})
    rt_wkb = pa.table({"name": pa.array([f"l{i}" for i in range(len(right))]), "geometry": right.to_arrow_wkb()})
    lt_nat = pa.table({"id": lt_wkb.column("id"), "geometry": _struct_coords(left.xy)})
    line_col = pa.ListArray.from_arrays(pa.array(right.geom_offsets), _struct_coords(right.xy))
    rt_nat = pa.table([rt_wkb.column("name"), line_col],
                      schema=pa.schema([pa.field("name", pa.string()), pa.field("geometry", line_col.type, metadata={"ARROW:extension:name": "geoarrow.linestring"})]))
    md = 3.0  # some points have nothing this close: the left join keeps them with nulls
    pairs, counts, dist = nearest_pairs(GeoSeries(left), GeoSeries(right), max_distance=md)
    assert 0 < np.count_nonzero(counts == 0) < len(left)
    li, ri = join_indices(counts, pairs, how)
    for lt, rt in ((lt_wkb, rt_wkb), (lt_nat, rt_nat)):
        t = spatial_join_nearest(lt, rt, SpatialJoinNearestArgs(join_type=how, max_distance=md, distance_col="dist"))
        assert t.column_names == ["id_left", "geometry_left", "name_right", "geometry_right", "dist"]
        assert t.num_rows == len(li)
        assert t.column("id_left").combine_chunks().equals(take_column(lt_wkb.column("id"), li))
        assert t.column("name_right").combine_chunks().equals(take_column(rt_wkb.column("name"), ri))
        assert t.column("geometry_right").combine_chunks().equals(take_column(rt_wkb.column("geometry"), ri))
        d = t.column("dist").combine_chunks()
        assert d.null_count == np.count_nonzero(ri < 0)
        assert np.array_equal(np.asarray(d.drop_null()), dist)
    _, counts, _ = nearest_pairs(GeoSeries(left), GeoSeries(right))
    t = spatial_join_nearest(lt_wkb, rt_wkb, SpatialJoinNearestArgs(join_type=how))
    assert t.column_names == ["id_left", "geometry_left", "name_right", "geometry_right"] and t.num_rows == int(counts.sum())


# ---- full size ---------------------------------------------------------------------------------------------------------------------


def test_full_size_c3_data(gpk, oracle):
    """10M points x 100k linestrings (the C3 data): every row's minimum against the GPU's own row-wise distance on the returned
    right row (its grouped schedule: within 1e-9), a 100k-row sample against the oracle"""
    lines = synth.random_linestrings(100_000)
    pts_h = synth.uniform_points(10_000_000)
    stream = torch.cuda.current_stream().cuda_stream
    pts = DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, torch.from_numpy(pts_h.xy).to("cuda:0"), stream=stream)
    ls = DeviceGeoArray.upload(lines, stream=stream)
    idx = SpatialIndex.from_device(ls, for_points=False)
    n = len(pts_h)
    counts = torch.empty(n, dtype=torch.int32, device="cuda:0")
    h = nearest_pairs_device(pts, ls, idx, counts, None)
    pairs = torch.empty((h, 2), dtype=torch.int32, device="cuda:0")
    dist = torch.empty(h, dtype=torch.float64, device="cuda:0")
    assert nearest_pairs_device(pts, ls, idx, counts, pairs, dist) == h
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    p = pairs.cpu().numpy().astype(np.int64)
    d = dist.cpu().numpy()
    assert np.all(c >= 1) and h == int(c.sum())
    first = np.concatenate([[0], np.cumsum(c)[:-1]])
    r_first = p[first, 1]
    # (in slices of fewer than 8 rows per linestring: the row-wise call then runs its per-row kernel, whose bits the join shares; with
    # more it orders the rows by target and runs the grouped schedule, which agrees to 1e-9)
    right = GeoSeries(lines, device=ls)
    step = 500_000
    for a in range(0, n, step):
        rw = GeoSeries(GeoArrowArray.from_points(pts_h.xy[a : a + step])).distance(right, other_rows=r_first[a : a + step].astype(np.uint32))
        got = d[first[a : a + step]]
        bad = np.flatnonzero(rw.view(np.uint64) != got.view(np.uint64))
        assert len(bad) == 0, (a, len(bad), rw[bad[:3]], got[bad[:3]])
    # the oracle on a 100k-row sample: the returned distance is the oracle's distance to the returned row
    rng = np.random.default_rng(9)
    sample = np.sort(rng.choice(n, 100_000, replace=False))
    od = oracle.distance_rowwise(GeoArrowArray.from_points(pts_h.xy[sample]), lines, b_rows=r_first[sample].astype(np.uint32))
    assert np.allclose(od, d[first][sample], rtol=1e-9, atol=0.0)
    # every linestring whose bbox is within the returned distance of a sampled point: none of them is nearer (checked on 100 rows)
    b = GeoSeries(lines).bounds()
    sub = sample[:100]
    qx, qy = pts_h.xy[sub, 0][:, None], pts_h.xy[sub, 1][:, None]
    bd = np.hypot(np.maximum(np.maximum(b[None, :, 0] - qx, qx - b[None, :, 2]), 0), np.maximum(np.maximum(b[None, :, 1] - qy, qy - b[None, :, 3]), 0))
    cand_l, cand_r = np.nonzero(bd <= d[first][sub][:, None] * (1 + 1e-9))
    cd = oracle.distance_rowwise(GeoArrowArray.from_points(pts_h.xy[sub][cand_l]), lines, b_rows=cand_r.astype(np.uint32))
    assert np.all(cd >= d[first][sub][cand_l] * (1 - 1e-9))
