"""Analytic reprojection, host side: the supported set, the C ABI entries, the Python argument checks that need no device, and the
kernel's own math (csrc/gpk_crs.h) run on the CPU by a stand-alone program against the mp fixture — plain and under
AddressSanitizer + UBSan."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries, crs_supported, parse_crs, utm_crs_of_bounds
from tests import crs_ref as R
from tests.host_build import build_host_drivers, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SUPPORTED = {4326, 3857, 3395, *range(32601, 32661), *range(32701, 32761)}


def test_supported_set_and_its_neighbours():
    lib = _abi.lib()
    for code in SUPPORTED:
        assert lib.gpk_crs_supported(code) == 1 and crs_supported(code)
    for code in (32600, 32661, 32700, 32761, 0, -1, 4325, 4327, 3856, 3858, 3394, 3396, 4269, 2263, 900913, 2**31 - 1):
        assert lib.gpk_crs_supported(code) == 0 and not crs_supported(code), code
    assert sum(lib.gpk_crs_supported(c) for c in range(0, 40000)) == len(SUPPORTED) == 123


def test_prototypes_exports_and_header():
    assert _abi._PROTOS["gpk_crs_supported"][1] == [_abi.C.c_int32]
    assert len(_abi._PROTOS["gpk_reproject"][1]) == 7
    lib = _abi.lib()
    assert lib.gpk_crs_supported and lib.gpk_reproject  # exported by the built library
    text = open(os.path.join(ROOT, "include", "geopolars_hip.h")).read()
    assert re.search(r"int32_t gpk_crs_supported\(int32_t epsg\);", text)
    assert re.search(r"int32_t gpk_reproject\(const gpk_geoarray\* a, int32_t src_epsg, int32_t dst_epsg, double\* out_xy, int64_t\* n_failed,\s+int32_t out_space, void\* stream\);", text)


def test_unsupported_code_is_refused_by_the_library_before_any_device_work():
    lib = _abi.lib()
    for src, dst, named in ((4326, 2263, "2263"), (32661, 3857, "32661")):
        rc = lib.gpk_reproject(None, src, dst, None, None, _abi.MEM_HOST, None)  # not even a handle: the codes are looked at first
        assert rc == _abi.GPK_ERR_INVALID_ARGUMENT
        assert f"EPSG:{named}" in _abi.last_error()


def test_crs_argument_forms():
    assert parse_crs("EPSG:4326") == parse_crs("epsg:4326") == parse_crs("Epsg:4326") == parse_crs("OGC:CRS84") == parse_crs("ogc:crs84") == parse_crs(4326) == 4326
    assert parse_crs(np.int64(32633)) == parse_crs(" EPSG:32633 ") == 32633
    assert parse_crs("EPSG:3857") == 3857 and parse_crs(3395) == 3395 and parse_crs("EPSG:32760") == 32760


@pytest.mark.parametrize("bad", ["EPSG:2263", "EPSG:32661", 32600, "WGS84", "+proj=utm +zone=33", "EPSG:", "EPSG:43x6", None, 4326.0, True, "OGC:CRS83"])
def test_unsupported_crs_raises_value_error_before_the_device(no_device, bad):
    s = GeoSeries(GeoArrowArray.from_points([(0.0, 0.0)]))
    for call in (lambda: s.reproject(bad, 4326), lambda: s.reproject("EPSG:4326", bad)):
        with pytest.raises(ValueError) as e:
            call()
        msg = str(e.value)
        assert "EPSG:4326 (OGC:CRS84), EPSG:3857, EPSG:3395, EPSG:32601-32660, EPSG:32701-32760" in msg and "PROJ" in msg and "to_crs" in msg
    with pytest.raises(ValueError, match="errors must be"):
        s.reproject(4326, 3857, errors="ignore")
    assert s._dev is None


def test_to_crs_still_points_off_the_accelerated_path():
    s = GeoSeries(GeoArrowArray.from_points([(0.0, 0.0)]))
    with pytest.raises(NotImplementedError, match="not on the accelerated path"):
        s.to_crs("EPSG:4326", "EPSG:3857")
    assert "reproject" in GeoSeries.to_crs.__doc__
    assert "Norway" in GeoSeries.estimate_utm_crs.__doc__ and "Svalbard" in GeoSeries.estimate_utm_crs.__doc__


@pytest.mark.parametrize("bounds,want", [
    ([[13.0, 52.0, 14.0, 53.0]], "EPSG:32633"),
    ([[-74.3, 40.4, -73.6, 41.0]], "EPSG:32618"),
    ([[-47.0, -24.0, -46.0, -23.0]], "EPSG:32723"),
    ([[-180.0, 10.0, -179.0, 11.0]], "EPSG:32601"),
    ([[179.0, -11.0, 180.0, -10.0]], "EPSG:32760"),
    ([[180.0, 0.0, 180.0, 0.0]], "EPSG:32660"),  # floor(360 / 6) + 1 = 61 is clamped
    ([[12.0, 0.0, 12.0, 0.0]], "EPSG:32633"),  # a zone edge belongs to the zone east of it; latitude 0 is north
    ([[11.0, -1e-9, 12.9999, -1e-9]], "EPSG:32732"),
    ([[0.0, 50.0, 1.0, 51.0], [np.nan] * 4, [29.0, 59.0, 30.0, 60.0]], "EPSG:32633"),  # total bounds 0..30 x 50..60; the empty row is ignored
    ([[5.0, 60.0, 6.0, 61.0]], "EPSG:32631"),  # Norway: the grid's 32V exception would say 32 — not applied
])
def test_estimate_utm_crs_arithmetic(bounds, want, monkeypatch):
    assert utm_crs_of_bounds(np.array(bounds, dtype=np.float64)) == want
    s = GeoSeries(GeoArrowArray.from_points([(0.0, 0.0)]))
    monkeypatch.setattr(GeoSeries, "bounds", lambda self: np.array(bounds, dtype=np.float64))  # stubbed bounds: no device
    assert s.estimate_utm_crs() == want and s._dev is None


def test_estimate_utm_crs_refuses_what_is_not_lon_lat():
    with pytest.raises(ValueError):
        utm_crs_of_bounds(np.array([[913175.0, 120121.0, 1067382.0, 272844.0]]))
    with pytest.raises(ValueError):
        utm_crs_of_bounds(np.full((2, 4), np.nan))


# ---- the kernel's math on the CPU --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "crs", fp_contract_off=True)


def _run_driver(exe, workdir, jobs):
    fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
    with open(fin, "wb") as f:
        for s, d, xy in jobs:
            f.write(struct.pack("<iiq", s, d, len(xy)))
            f.write(np.ascontiguousarray(xy, dtype=np.float64).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = open(fout, "rb").read()
    res, o = [], 0
    for s, d, xy in jobs:
        (nf,) = struct.unpack_from("<q", raw, o)
        res.append((nf, np.frombuffer(raw, dtype=np.float64, count=2 * len(xy), offset=o + 8).reshape(-1, 2)))
        o += 8 + 16 * len(xy)
    assert o == len(raw)
    return res


@pytest.fixture(scope="module")
def cases():
    return R.fixture_cases(np.load(os.path.join(HERE, "golden", "crs_reference.npz")))


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_driver_matches_the_fixture(drivers, cases, build):
    """every instance, every fixture row, on the CPU: 1e-7 m against the mp reference; no failures inside the pinned domain"""
    built, workdir = drivers
    res = _run_driver(built[build], workdir, [(s, d, a) for _, s, d, a, _ in cases])
    worst = {}
    for (name, s, d, a, b), (nf, got) in zip(cases, res):
        assert nf == 0, name
        worst[name] = R.error_metres(d, got, b).max()
    print({k: f"{v:.2e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= R.TOL_M}
    assert not bad, bad


def test_host_driver_failure_rules(drivers):
    built, workdir = drivers
    nan, inf = np.nan, np.inf
    geo = np.array([[10.0, 50.0], [nan, 1.0], [1.0, nan], [inf, 0.0], [0.0, -inf], [0.0, 90.0001], [0.0, -90.0001], [5.0, 90.0], [5.0, -90.0], [20.0, 40.0]])
    far = np.array([[15.0 + 95.0, 10.0], [15.0 - 95.0, -10.0], [15.0 + 90.0, 0.0], [15.0 + 89.0, 5.0], [15.0, 90.0], [15.0, -90.0]])
    same = np.array([[nan, 1.0], [3.0, 4.0]])
    for exe in built.values():
        (nf, merc), (nf2, tm), (nf3, cp), (nf4, emp) = _run_driver(exe, workdir, [(4326, 3857, geo), (4326, 32633, far), (3395, 3395, same), (4326, 3395, np.zeros((0, 2)))])
        assert nf == 8 and np.isnan(merc[1:9]).all() and np.isfinite(merc[[0, 9]]).all()
        assert nf2 == 3 and np.isnan(tm[:3]).all() and np.isfinite(tm[3:]).all()  # the pole is a point of every zone
        assert abs(tm[4, 0] - 500000.0) < 1e-6 and abs(tm[4, 1] - 0.9996 * 10001965.729313) < 1e-5 and abs(tm[5, 1] + 0.9996 * 10001965.729313) < 1e-5
        assert nf3 == 0 and np.array_equal(cp, same, equal_nan=True) and nf4 == 0 and len(emp) == 0
        # longitudes come out wrapped; +-180 stay
        (_, back), = _run_driver(exe, workdir, [(32660, 4326, np.array([[500000.0 + 400000.0, 1000000.0], [500000.0, 0.0]]))])
        assert -180.0 <= back[0, 0] < -170.0 and back[1, 0] == 177.0
        (_, w), = _run_driver(exe, workdir, [(4326, 3857, np.array([[180.0, 0.0], [-180.0, 0.0], [540.0, 0.0], [181.0, 0.0]]))])
        assert w[0, 0] == -w[1, 0] and abs(w[0, 0] - 20037508.342789243) < 1e-7 and abs(abs(w[2, 0]) - 20037508.342789243) < 1e-7 and w[3, 0] < -1.99e7
