"""GPU: gpk_representative_point (csrc/gpk_interior.hip) against the exact reference of tests/interior_ref.py — the checks of the host
driver (tests/test_interior_host.py) through the C ABI and through GeoSeries.representative_point, on both lane-group sizes, the
work-group path and the queued rows, at both placements and in both coordinate layouts; the interior guarantee through the library's own
exact `contains`; and the composition with the point-in-polygon join."""
from fractions import Fraction

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import DeviceGeoArray, GeoArrowArray
from geopolars_amd.geoseries import GeoSeries, representative_point_device
from geopolars_amd.spatial_index import join_pairs
from tests import exact_ref as X
from tests import interior_ref as I

pytestmark = pytest.mark.gpu
PG, MPG = I.PG, I.MPG


@pytest.fixture(scope="module")
def golden():
    return np.load(I.GOLDEN)


def abi_answers(dev: DeviceGeoArray, n: int, space: str):
    """(xy, valid, width) through host buffers or through device buffers"""
    if space == "host":
        xy, valid, width = np.full((n, 2), 7.0), np.full(n, 9, dtype=np.uint8), np.full(n, 7.0)
        _abi.check(_abi.lib().gpk_representative_point(dev.handle, xy.ctypes.data, valid.ctypes.data, width.ctypes.data, _abi.MEM_HOST, None))
        return xy, valid, width
    import torch

    xy = torch.full((n, 2), 7.0, dtype=torch.float64, device="cuda")
    valid = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    width = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    representative_point_device(dev, xy, valid, width)
    torch.cuda.synchronize()
    return xy.cpu().numpy(), valid.cpu().numpy(), width.cpu().numpy()


def separated(col: GeoArrowArray) -> DeviceGeoArray:
    """the column uploaded from separate x / y arrays"""
    import torch

    t = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device="cuda")  # noqa: E731
    x, y = t(col.xy[:, 0], np.float64), t(col.xy[:, 1], np.float64)
    return DeviceGeoArray.from_device_buffers(col.geom_type, (x, y), t(col.geom_offsets, np.int32), t(col.part_offsets, np.int32), t(col.ring_offsets, np.int32),
                                              t(col.validity, np.uint8))


def check_column(kind, rows, valid_in, xy, valid, width, contains=None):
    """the host driver's checks, row by row; returns the worst x error as a fraction of tol"""
    worst = 0.0
    for i, row in enumerate(rows):
        has = bool(valid_in[i]) and len(I.row_coords(kind, row)) > 0 and I.finite_row(kind, row)
        assert bool(valid[i]) == has, i
        if not has:
            assert np.isnan(xy[i]).all() and np.isnan(width[i]), i
            continue
        x, y = float(xy[i, 0]), float(xy[i, 1])
        if kind in (PG, MPG):
            ref = I.polygon_row(kind, row)
            worst = max(worst, I.check_polygon_answer(kind, row, x, y, float(width[i])))
            if ref["choice"] is None:
                assert width[i] == 0.0 and (x, y) == ref["first"], i  # degenerate: bit-exact
            elif contains is not None and ref["max_width"] >= Fraction(I.MIN_REL_WIDTH * I.diagonal(kind, row)):
                assert contains[i], ("interior guarantee", i, x, y)
        else:
            assert np.isnan(width[i]), i
            I.check_vertex_answer(kind, row, x, y)
    return worst


@pytest.mark.parametrize("placement", list(I.PLACEMENTS))
@pytest.mark.parametrize("fam", list(I.FAMILIES))
def test_fixture_rows(gpk, golden, fam, placement):
    """every fixture row through the C ABI (host and device buffers, interleaved and separated coordinates) and through GeoSeries;
    two calls give identical bits"""
    kind = I.FAMILIES[fam]
    col = I.fixture_column(golden, fam, I.PLACEMENTS[placement])
    rows, valid_in = I.column_rows(col), golden[f"{fam}_valid"]
    s = GeoSeries(col)
    n = len(s)
    xy, valid, width = abi_answers(s.device(), n, "host")
    contains = None
    if kind in (PG, MPG):
        contains = s.contains(GeoSeries(GeoArrowArray.from_points(np.where(np.isnan(xy), 0.0, xy))))
    print(f"worst x error: {check_column(kind, rows, valid_in, xy, valid, width, contains):.3g} of tol")
    for other in (abi_answers(s.device(), n, "device"), abi_answers(separated(col), n, "host"), abi_answers(s.device(), n, "host")):
        for a, b in zip((xy, valid, width), other):
            assert np.array_equal(a, b, equal_nan=True)  # (the same bits: another buffer space, the other layout, a second call)
    pts, w = s.representative_point(return_width=True)
    assert np.array_equal(pts.array.xy, xy, equal_nan=True) and np.array_equal(pts.array.is_valid(), valid.astype(bool)) and np.array_equal(w, width, equal_nan=True)
    assert np.array_equal(s.point_on_surface().array.xy, xy, equal_nan=True)
    if kind not in (PG, MPG) and placement == "lattice":  # the fixture's recorded verdicts: exact ties go to the first candidate
        ok = valid.astype(bool)
        assert np.array_equal(xy[ok], golden[f"{fam}_nearest"][ok])


def _padded(rows, filler, count):
    return list(rows) + [filler] * count


@pytest.mark.parametrize("G", [I.G_SMALL, I.G_LARGE])
def test_both_group_sizes_and_the_work_group_paths(gpk, golden, G):
    """the polygon rows in a column whose mean coordinate count picks G = 4 (padded with triangles) and in one that picks G = 16: the
    same bits for every row, whatever the group size — the combs around the slice capacity, the queued comb_17 / comb_33 and the rows
    above 512 coordinates included"""
    col = I.fixture_column(golden, "pg")
    rows = I.column_rows(col)[:-1]  # (without the null row)
    fill = 600 if G == I.G_SMALL else 0
    full = X.column(PG, _padded(rows, [I.TRI], fill))
    assert (I.G_LARGE if full.n_coords / full.n_geoms >= I.G_MEAN else I.G_SMALL) == G
    xy, valid, width = abi_answers(GeoSeries(full).device(), full.n_geoms, "host")
    check_column(PG, I.column_rows(full), np.ones(full.n_geoms, bool), xy, valid, width)
    ref_xy, _, ref_w = abi_answers(GeoSeries(X.column(PG, rows)).device(), len(rows), "host")
    assert np.array_equal(xy[: len(rows)], ref_xy, equal_nan=True) and np.array_equal(width[: len(rows)], ref_w, equal_nan=True)


def test_small_and_work_group_paths_agree(gpk):
    """rows of at most 32 crossings in a column of small rows, which the lane groups finish (G = 4 and G = 16), and the same rows
    padded with vertices on their base beyond 512 coordinates, which the work-group kernel takes: the same point within tol"""
    shapes = [[I.rect(0, 0, 7, 3)], [I.L_SHAPE], [I.U_SHAPE], I.RING_SHAPE, I.holed((2, 3), (12, 13), (16, 17)), [I.comb(3, wide=1)], [I.comb(16, wide=11)],
              [I.TRI]]
    assert all(len(m["crossings"]) <= I.SLICE for row in shapes for m in I.polygon_row(PG, row)["members"])
    big = [[I.pad_base(row[0], I.BLOCK_COORDS + 1 + 37 * i)] + list(row[1:]) for i, row in enumerate(shapes)]
    b = abi_answers(GeoSeries(X.column(PG, big)).device(), len(big), "host")
    check_column(PG, I.column_rows(X.column(PG, big)), np.ones(len(big), bool), *b)
    for fill in ([[I.TRI]] * 40, [[I.comb(17)]] * 6):  # mean coordinate count below / above 32 (the combs of 34 crossings are queued, the shapes are not)
        col = X.column(PG, shapes + fill)
        assert (col.n_coords / col.n_geoms >= I.G_MEAN) == (len(fill) == 6) and max(len(I.row_coords(PG, r)) for r in shapes) <= I.BLOCK_COORDS
        a = abi_answers(GeoSeries(col).device(), col.n_geoms, "host")
        for i, row in enumerate(big):
            tol = I.tolerance(PG, row)
            assert abs(a[0][i, 0] - b[0][i, 0]) <= tol and a[0][i, 1] == b[0][i, 1] and abs(a[2][i] - b[2][i]) <= 2 * tol, i


def test_more_crossings_than_the_lds_list(gpk):
    """a member with more crossings than the work-group's LDS list holds is ranked by walking its edges again"""
    k = I.LDS_CROSSINGS // 2 + 6
    rows = [[I.comb(k, wide=k - 3)], [I.comb(k)], [I.TRI]]
    col = X.column(PG, rows)
    assert len(I.member_sections(rows[0])["crossings"]) == 2 * k > I.LDS_CROSSINGS
    xy, valid, width = abi_answers(GeoSeries(col).device(), 3, "host")
    check_column(PG, I.column_rows(col), np.ones(3, bool), xy, valid, width)
    assert width[0] == 2.0 and (xy[1, 0], width[1]) == (0.5, 1.0)


def test_huge_lineal_and_puntal_rows(gpk):
    """rows above 512 coordinates of the vertex families take the work-group kernel"""
    n = I.BLOCK_COORDS * 3 + 5
    line = [(float(i), float((i * 7) % 13)) for i in range(n)]
    for kind, rows in ((I.LS, [line, line[:5]]), (I.MLS, [[line[:700], [], line[700:]], [line[:3]]]), (I.MPT, [line, line[:2]])):
        col = X.column(kind, rows)
        xy, valid, width = abi_answers(GeoSeries(col).device(), 2, "host")
        check_column(kind, I.column_rows(col), np.ones(2, bool), xy, valid, width)


def test_non_finite_rows(gpk):
    sq = I.rect(0, 0, 4, 4)
    bad = list(sq)
    bad[2] = (float("nan"), 4.0)
    for kind, rows in ((PG, [[sq], [bad], [[(0, 0), (float("inf"), 0), (1, 1), (0, 0)]]]), (I.LS, [[(0, 0), (1, 1), (2, 0)], [(0, 0), (float("nan"), 1), (2, 0)]]),
                       (I.MPT, [[(0, 0)], [(0, 0), (float("-inf"), 1)]])):
        xy, valid, width = abi_answers(GeoSeries(X.column(kind, rows)).device(), len(rows), "host")
        assert valid[0] == 1 and not valid[1:].any() and np.isnan(xy[1:]).all() and np.isnan(width[1:]).all()


def test_representative_points_join_back_to_their_polygons(gpk):
    """a few hundred ring- and L-shaped polygons on a jittered grid: the representative points, computed on the device and joined without
    a host round trip, fall in exactly their own polygons; the centroids of the same polygons do not"""
    import torch

    rng = np.random.default_rng(5)
    polys = []
    for i in range(18):
        for j in range(18):
            ox, oy = 40 * i + int(rng.integers(0, 8)), 40 * j + int(rng.integers(0, 8))
            shape = I.RING_SHAPE if (i + j) % 2 else [I.L_SHAPE]
            k = int(rng.integers(1, 4))
            polys.append([[(ox + k * x, oy + k * y) for x, y in ring] for ring in shape])
    s = GeoSeries(X.column(PG, polys))
    n = len(s)
    xy = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    pts = GeoSeries(None, device=representative_point_device(s.device(), xy))
    pairs, counts = join_pairs(pts, s, "within")
    assert np.array_equal(pairs, np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.uint32)) and (counts == 1).all()
    cpairs, _ = join_pairs(s.centroid(), s, "within")
    assert len(cpairs) < n
