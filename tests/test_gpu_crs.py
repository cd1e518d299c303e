"""gpk_reproject on the GPU against the mp fixture (tests/golden/crs_reference.npz, tests/crs_ref.py): every (source kind, destination
kind) instance to 1e-7 m, wave / block tails, the grid-stride path, nesting carried over, the failure rules and the Python surface."""
import ctypes as C
import os

import numpy as np
import pytest

from geopolars_amd.geoarrow import DeviceGeoArray, GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from tests import crs_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FX = np.load(os.path.join(GOLD, "crs_reference.npz"))
CASES = {c[0]: c for c in R.fixture_cases(FX)}
A = 6378137.0


def points(xy) -> GeoSeries:
    return GeoSeries(GeoArrowArray.from_points(np.asarray(xy, dtype=np.float64)))


@pytest.mark.parametrize("name", list(CASES))
def test_every_instance_matches_the_mp_fixture(gpk, name):
    """all 13 (source kind, destination kind) instances: both Mercators and geographic among each other (world), everything with a
    transverse Mercator on either side incl. zone 33N <-> 34N and 33N <-> 33S across the false northing (tm), zones 1 and 60 across the
    antimeridian (anti).  1e-7 m, ground distance for geographic results"""
    _, s, d, a, b = CASES[name]
    got = points(a).reproject(s, d).array.xy  # errors="raise": no row of the pinned domain fails
    err = R.error_metres(d, got, b)
    print(f"{name}: {len(a)} rows, worst {err.max():.3e} m")
    assert err.max() <= R.TOL_M


@pytest.mark.parametrize("name", ["tm:4326->32633", "tm:32733->32634", "world:3395->4326"])
@pytest.mark.parametrize("n", [1, 63, 255, 257, 1003])
def test_wave_and_block_tails(gpk, name, n):
    _, s, d, a, b = CASES[name]
    got = points(a[:n]).reproject(s, d).array.xy
    assert got.shape == (n, 2) and R.error_metres(d, got, b[:n]).max() <= R.TOL_M
    assert np.array_equal(got, points(a).reproject(s, d).array.xy[:n])  # a coordinate's result does not depend on its neighbours


def test_empty_column_touches_nothing(gpk):
    s = points(np.zeros((0, 2)))
    assert s.reproject(4326, 32633).array.xy.shape == (0, 2)
    sentinel = np.full(4, 7.0)
    nf = C.c_int64(-1)
    gpk.check(gpk.lib().gpk_reproject(s.device().handle, 4326, 3857, sentinel.ctypes.data, C.byref(nf), gpk.MEM_HOST, None))
    assert nf.value == 0 and (sentinel == 7.0).all()
    hollow = GeoSeries(GeoArrowArray.from_polygons([[], []]))
    assert hollow.reproject(3857, 4326).array.n_coords == 0 and len(hollow.reproject(3857, 4326)) == 2


def test_grid_stride_path_is_bit_identical_per_tile(gpk):
    """more coordinates than cu_count * 8 blocks of 256 hold, plus one partial block: every tile of the fixture must come out as the first"""
    import torch

    _, s, d, a, b = CASES["tm:4326->32633"]
    _, cus = gpk.device_info()
    t = len(a)
    k = (cus * 8 * 256) // t + 1
    part = 100
    n = k * t + part
    assert n > cus * 8 * 256 and n % 256 != 0
    xy = torch.from_numpy(np.concatenate([np.tile(a, (k, 1)), a[:part]])).to("cuda:0")
    out = torch.full((n, 2), -1.0, dtype=torch.float64, device="cuda:0")
    dev = DeviceGeoArray.from_device_buffers(gpk.GEOM_POINT, xy)
    nf = C.c_int64(-1)
    gpk.check(gpk.lib().gpk_reproject(dev.handle, s, d, out.data_ptr(), C.byref(nf), gpk.MEM_DEVICE, None))
    got = out.cpu().numpy()
    assert nf.value == 0
    assert R.error_metres(d, got[:t], b).max() <= R.TOL_M
    assert (got[: k * t].reshape(k, t, 2) == got[:t]).all() and np.array_equal(got[k * t :], got[:part])


def _nested_columns():
    ring = lambda x, y: [(x, y), (x + 0.5, y), (x + 0.5, y + 0.25), (x, y + 0.25)]  # noqa: E731
    pts = GeoArrowArray.from_points([(13.0, 52.0), (14.0, 53.0), (15.0, -33.0), (16.5, 0.0)], validity=np.packbits([1, 0, 1, 1], bitorder="little"))
    lines = GeoArrowArray.from_linestrings([[(13.0, 52.0), (13.5, 52.5), (14.0, 52.0)], [], [(15.0, -1.0), (15.0, 1.0)]])
    lines.validity = np.packbits([1, 1, 0], bitorder="little")
    polys = GeoArrowArray.from_polygons([[ring(12.0, 40.0), ring(12.1, 40.05)], [ring(17.0, -20.0)], [], [ring(15.0, 60.0)]])
    polys.validity = np.packbits([1, 0, 1, 1], bitorder="little")
    mps = GeoArrowArray.from_multipolygons([[[ring(12.0, 40.0)], [ring(13.0, 41.0), ring(13.1, 41.05)]], [], [[ring(16.0, -45.0)]]])
    mps.validity = np.packbits([1, 1, 0], bitorder="little")
    return {"point": pts, "linestring": lines, "polygon": polys, "multipolygon": mps}


@pytest.mark.parametrize("family", ["point", "linestring", "polygon", "multipolygon"])
def test_nesting_and_validity_are_carried_over(gpk, family):
    a = _nested_columns()[family]
    out = GeoSeries(a).reproject("OGC:CRS84", "epsg:32633").array
    assert out.geom_type == a.geom_type and out.n_geoms == a.n_geoms
    for name in ("geom_offsets", "part_offsets", "ring_offsets", "validity"):
        x, y = getattr(a, name), getattr(out, name)
        assert (x is None and y is None) or np.array_equal(x, y), name
    want = R.np_transform(4326, 32633, a.xy)
    assert out.xy.shape == a.xy.shape and np.abs(out.xy - want).max() < 1e-6  # only xy changes, and every coordinate of it (null rows too)
    back = GeoSeries(out).reproject(32633, 4326).array.xy
    assert R.error_metres(4326, back, a.xy).max() <= 2 * R.TOL_M


def test_device_and_host_outputs_are_the_same_bits_and_n_failed_may_be_null(gpk):
    import torch

    _, s, d, a, b = CASES["tm:3857->32634"]
    host = points(a).reproject(s, d).array.xy
    xy = torch.from_numpy(a).to("cuda:0")
    dev = DeviceGeoArray.from_device_buffers(gpk.GEOM_POINT, xy)
    out = torch.empty((len(a), 2), dtype=torch.float64, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    gpk.check(gpk.lib().gpk_reproject(dev.handle, s, d, out.data_ptr(), None, gpk.MEM_DEVICE, stream))  # no count: nothing read back
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), host)
    host2 = np.empty_like(a)
    gpk.check(gpk.lib().gpk_reproject(dev.handle, s, d, host2.ctypes.data, None, gpk.MEM_HOST, stream))
    assert np.array_equal(host2, host)
    bad = np.array([[0.0, 91.0], [1.0, 2.0]])
    gpk.check(gpk.lib().gpk_reproject(points(bad).device().handle, 4326, 3395, host2.ctypes.data, None, gpk.MEM_HOST, None))
    assert np.isnan(host2[0]).all() and np.isfinite(host2[1]).all()


def test_failed_coordinates_are_nan_and_counted(gpk):
    nan, inf = np.nan, np.inf
    geo = np.array([[10.0, 50.0], [nan, 1.0], [11.0, 51.0], [1.0, nan], [inf, 0.0], [0.0, -inf], [12.0, -52.0], [0.0, 90.0001], [5.0, 90.0], [5.0, -90.0], [20.0, 40.0]])
    failing = [1, 3, 4, 5, 7, 8, 9]
    s = points(geo)
    clean = points(np.delete(geo, failing, axis=0)).reproject(4326, 3857).array.xy
    with pytest.raises(ValueError, match=r"7 of 11 coordinates failed"):
        s.reproject(4326, 3857)
    got = s.reproject(4326, 3857, errors="nan").array.xy
    assert np.isnan(got[failing]).all()
    assert np.array_equal(np.delete(got, failing, axis=0), clean)  # the neighbours are untouched
    nf = C.c_int64(0)
    out = np.empty_like(geo)
    gpk.check(gpk.lib().gpk_reproject(s.device().handle, 4326, 3857, out.ctypes.data, C.byref(nf), gpk.MEM_HOST, None))
    assert nf.value == len(failing)
    # 95 degrees from the central meridian of zone 33 fails; 89 does not; +-90 is the limit itself
    far = points([[15.0 + 95.0, 10.0], [15.0 + 89.0, 10.0], [15.0 - 95.0, -10.0], [15.0 + 90.0, 0.0], [15.0, 10.0]])
    with pytest.raises(ValueError, match="3 of 5"):
        far.reproject(4326, 32633)
    g = far.reproject(4326, 32633, errors="nan").array.xy
    assert np.isnan(g[[0, 2, 3]]).all() and np.isfinite(g[[1, 4]]).all()
    # many waves: one failure every 97 coordinates of a column longer than a block
    _, sc, dc, a, b = CASES["world:4326->3395"]
    a = a.copy()
    a[::97, 1] = 90.5
    out = np.empty_like(a)
    gpk.check(gpk.lib().gpk_reproject(points(a).device().handle, sc, dc, out.ctypes.data, C.byref(nf), gpk.MEM_HOST, None))
    assert nf.value == len(a[::97]) and np.isnan(out[::97]).all() and np.isfinite(np.delete(out, np.s_[::97], axis=0)).all()


@pytest.mark.parametrize("group,epsg", [("world", 3857), ("world", 3395), ("tm", 32633), ("tm", 32733), ("anti", 32601), ("anti", 32660)])
def test_round_trip_through_every_projected_kind(gpk, group, epsg):
    geo = FX[f"{group}_4326"][np.isfinite(FX[f"{group}_{epsg}"]).all(axis=1)]
    back = points(geo).reproject(4326, epsg).reproject(epsg, 4326).array.xy
    err = R.error_metres(4326, back, geo)
    print(f"{group} 4326 -> {epsg} -> 4326: worst {err.max():.3e} m")
    assert err.max() <= 2 * R.TOL_M


@pytest.mark.parametrize("crs", [4326, 3857, 3395, 32633, 32733])
def test_same_to_same_is_a_bit_exact_copy(gpk, crs):
    xy = np.array([[1.5, 2.5], [np.nan, 0.0], [1e300, -1e-300], [-0.0, 95.0]])
    got = points(xy).reproject(crs, f"EPSG:{crs}").array.xy
    assert got.tobytes() == xy.tobytes()


def test_estimate_utm_crs_on_the_datasets(gpk):
    z = np.load(os.path.join(GOLD, "naturalearth_cities.npz"))
    xy = GeoArrowArray.from_wkb(z["wkb_values"], z["wkb_offsets"]).xy
    for lo, hi, south, want in ((12.0, 18.0, False, "EPSG:32633"), (-48.0, -42.0, True, "EPSG:32723"), (138.0, 144.0, False, "EPSG:32654"), (-78.0, -72.0, False, "EPSG:32618")):
        sel = xy[(xy[:, 0] >= lo) & (xy[:, 0] < hi) & ((xy[:, 1] < 0) == south)]
        assert len(sel) >= 1, (lo, hi)
        assert points(sel).estimate_utm_crs() == want  # every point of the subset lies in the zone, so the centre of its bounds does
    # nybb is in the New York state plane (feet), outside the analytic set: its boroughs are brought to lon/lat by the affine map
    # that sends the column's bounds to the city's geographic bounds (-74.26..-73.70, 40.49..40.92) — a zone estimate needs no more
    nz = np.load(os.path.join(GOLD, "nybb.npz"))
    nybb = GeoSeries(GeoArrowArray.from_wkb(nz["wkb_values"], nz["wkb_offsets"]))
    b = nybb.bounds()
    x0, y0, x1, y1 = b[:, 0].min(), b[:, 1].min(), b[:, 2].max(), b[:, 3].max()
    sx, sy = (-73.70 + 74.26) / (x1 - x0), (40.92 - 40.49) / (y1 - y0)
    lonlat = nybb.affine_transform([sx, 0.0, -74.26 - sx * x0, 0.0, sy, 40.49 - sy * y0])
    assert lonlat.estimate_utm_crs() == "EPSG:32618"
    utm = lonlat.reproject(4326, lonlat.estimate_utm_crs())
    assert 0.9 < utm.area().sum() / (nz["Shape_Area"].sum() * 0.3048006096**2) < 1.1  # square feet -> square metres: the boroughs keep their size
