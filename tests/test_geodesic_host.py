"""Geodesic area / perimeter / inverse / direct, host side: prototypes, exports and header text, the refusals that need no device, and the
kernels' own math (csrc/gpk_geodesic.h) run on the CPU by a stand-alone program over the mp fixture — plain and under AddressSanitizer +
UBSan.  The program's worst errors per regime are what the named tolerances of tests/geodesic_measure_ref.py record."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from tests import geodesic_measure_ref as R
from tests.host_build import build_host_drivers, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "geodesic_measures_mp.npz")


def test_prototypes_exports_and_header():
    assert len(_abi._PROTOS["gpk_geodesic_area"][1]) == 6 and _abi._PROTOS["gpk_geodesic_area"][1][1] is C.c_uint32
    assert len(_abi._PROTOS["gpk_geodesic_inverse"][1]) == 8 and len(_abi._PROTOS["gpk_geodesic_direct"][1]) == 9
    assert _abi._PROTOS["gpk_geodesic_direct"][1][2] is C.c_int64 and _abi._PROTOS["gpk_geodesic_direct"][1][4] is C.c_int64
    lib = _abi.lib()
    assert lib.gpk_geodesic_area and lib.gpk_geodesic_inverse and lib.gpk_geodesic_direct  # exported by the built library
    text = open(os.path.join(ROOT, "include", "geopolars_hip.h")).read()
    assert re.search(r"#define GPK_GEODESIC_AREA_SIGNED 1u", text) and _abi.GEODESIC_AREA_SIGNED == 1
    assert re.search(r"int32_t gpk_geodesic_area\(const gpk_geoarray\* a, uint32_t flags, double\* out_area, double\* out_perimeter, int32_t out_space,\s+void\* stream\);", text)
    assert re.search(r"int32_t gpk_geodesic_inverse\(const gpk_geoarray\* a, const gpk_geoarray\* b, const uint32_t\* b_rows, double\* out_s12, double\* out_azi1,\s+double\* out_azi2, int32_t out_space, void\* stream\);", text)
    assert re.search(r"int32_t gpk_geodesic_direct\(const gpk_geoarray\* a, const double\* azi1, int64_t n_azi, const double\* s12, int64_t n_s12, double\* out_xy,\s+double\* out_azi2, int32_t out_space, void\* stream\);", text)
    for phrase in ("to the LEFT of its direction of travel", "HOLES INCLUDED", "reports its complement", "(-A0/2, A0/2]", "same bits from run to run"):
        assert phrase in text, phrase


def test_null_handles_are_refused_by_the_library():
    lib = _abi.lib()
    assert lib.gpk_geodesic_area(None, 0, None, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert lib.gpk_geodesic_inverse(None, None, None, None, None, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert lib.gpk_geodesic_direct(None, None, 1, None, 1, None, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT


def test_python_refusals_come_before_the_device(no_device):
    pts = GeoSeries(GeoArrowArray.from_points([(0.0, 0.0), (1.0, 1.0)]))
    three = GeoSeries(GeoArrowArray.from_points([(0.0, 0.0), (1.0, 1.0), (2.0, 2.0)]))
    lines = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)], [(0.0, 0.0), (1.0, 1.0)]]))
    for call in (lambda: pts.geodesic_distance(lines), lambda: lines.geodesic_distance(pts), lambda: pts.geodesic_bearing(lines),
                 lambda: lines.geodesic_destination(0.0, 1.0)):
        with pytest.raises(_abi.MismatchedGeometry):
            call()
    for call in (lambda: pts.geodesic_distance(three), lambda: pts.geodesic_distance(three, other_rows=[0]), lambda: pts.geodesic_bearing(pts, final=1),
                 lambda: pts.geodesic_destination([0.0, 1.0, 2.0], 1.0), lambda: pts.geodesic_destination(0.0, [[1.0, 2.0]]),
                 lambda: pts.geodesic_destination("north", 1.0), lambda: pts.geodesic_area(signed="yes")):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            call()
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    assert pts._dev is None and lines._dev is None


# ---- the kernels' math on the CPU --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "geodesic", fp_contract_off=True)


def run_driver(exe, workdir, fx):
    fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
    ne, nd, nr, nc = len(fx["edge_xy"]), len(fx["direct_in"]), len(fx["ring_off"]) - 1, len(fx["ring_xy"])
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()  # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).tobytes()  # noqa: E731
    with open(fin, "wb") as f:
        f.write(struct.pack("<qqqq", ne, nd, nr, nc))
        f.write(f64(fx["edge_xy"]))
        f.write(f64(np.stack([fx["edge_s12"], fx["edge_azi1"], fx["edge_azi2"], fx["edge_m12"].astype(np.float64), fx["edge_S12"]], axis=1)))
        f.write(i32(fx["edge_regime"]))
        f.write(f64(fx["direct_in"]))
        f.write(f64(fx["direct_out"]))
        f.write(i32(fx["ring_off"]))
        f.write(i32(fx["ring_regime"]))
        f.write(f64(fx["ring_xy"]))
        f.write(f64(np.stack([fx["ring_area"], fx["ring_perimeter"]], axis=1)))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = np.fromfile(fout, dtype=np.float64)
    assert len(raw) == 7 * ne + 3 * nd + 2 * nr
    # an edge's record: s12, azi1, azi2, m12, S12 of inverse<true>, then haversine_m and vincenty_m of the same edge
    return raw[: 7 * ne].reshape(ne, 7), raw[7 * ne: 7 * ne + 3 * nd].reshape(nd, 3), raw[7 * ne + 3 * nd:].reshape(nr, 2), r.stdout


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture(FIXTURE)


def same_bits(got, want):
    """the same NaN positions, and the same bits everywhere else"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_driver_against_the_fixture(drivers, fixture, oracle, build):
    """the header on the CPU against the mp fixture, every regime, within the MEASURED tolerances (no GPU_FACTOR here); the driver prints
    the worst error per regime.  The three length functions of gpk_geodesic_length (inverse's s12, haversine_m, vincenty_m) are the
    operations of oracle/gpk_oracle.c in the same order: on the host they give its bits, edge by edge"""
    built, workdir = drivers
    edges, direct, rings, text = run_driver(built[build], workdir, fixture)
    print(text)
    R.check_edges(fixture, edges[:, 0], edges[:, 1], edges[:, 2], edges[:, 4], factor=1)
    R.check_direct(fixture, direct[:, :2], direct[:, 2], factor=1)
    R.check_rings(fixture, rings[:, 0], rings[:, 1], factor=1)
    assert "differs: 1" not in text  # inverse<false> gives the distance and azimuths of inverse<true>, bit for bit
    n = len(fixture["edge_xy"])
    lines = GeoArrowArray(_abi.GEOM_LINESTRING, np.ascontiguousarray(fixture["edge_xy"], dtype=np.float64).reshape(2 * n, 2),
                          geom_offsets=np.arange(0, 2 * n + 1, 2, dtype=np.int32))
    for column, method in ((0, "geodesic"), (5, "haversine"), (6, "vincenty")):
        want = oracle.geodesic_length(lines, method)
        assert same_bits(np.ascontiguousarray(edges[:, column]), want), method
        assert method != "vincenty" or 0 < np.isnan(want).sum() < n  # the fixture has edges Vincenty's iteration gives up on


def test_host_driver_refusals_and_reduction(drivers, oracle):
    """NaN and out-of-range latitudes give NaN in every field; the transit count and the area reduction on hand-made rings.  The length
    functions on the same edges: NaN for a NaN coordinate and zero for identical points like inverse; haversine and Vincenty, like geo's,
    do not look at the latitude's range, so there they are held to the oracle's bits instead"""
    built, workdir = drivers
    nan = np.nan
    fx = {"edge_xy": np.array([[0.0, 90.0001, 1.0, 0.0], [0.0, 0.0, 1.0, -91.0], [nan, 0.0, 1.0, 1.0], [0.0, 0.0, 1.0, nan], [5.0, 5.0, 5.0, 5.0]]),
          "direct_in": np.array([[0.0, 91.0, 10.0, 5.0], [nan, 1.0, 10.0, 5.0], [0.0, 1.0, nan, 5.0], [0.0, 1.0, 10.0, nan], [179.5, 0.0, 90.0, 200000.0],
                                 [12.0, 34.0, 56.0, 0.0]]),
          # a ring around the north pole, counter-clockwise seen from above it (eastwards), and its reverse: the cap, then minus the cap
          "ring_xy": np.array([[0.0, 80.0], [120.0, 80.0], [-120.0, 80.0], [0.0, 80.0], [0.0, 80.0], [-120.0, 80.0], [120.0, 80.0], [0.0, 80.0]]),
          "ring_off": np.array([0, 4, 8], dtype=np.int32)}
    n, m = len(fx["edge_xy"]), len(fx["direct_in"])
    fx.update(edge_s12=np.zeros(n), edge_azi1=np.zeros(n), edge_azi2=np.zeros(n), edge_m12=np.zeros(n, dtype=np.float32), edge_S12=np.zeros(n),
              edge_regime=np.zeros(n, dtype=np.int32), direct_out=np.zeros((m, 3)), ring_regime=np.zeros(2, dtype=np.int32), ring_area=np.zeros(2),
              ring_perimeter=np.zeros(2))
    lines = GeoArrowArray(_abi.GEOM_LINESTRING, fx["edge_xy"].reshape(2 * n, 2), geom_offsets=np.arange(0, 2 * n + 1, 2, dtype=np.int32))
    for exe in built.values():
        edges, direct, rings, _ = run_driver(exe, workdir, fx)
        assert np.isnan(edges[:4, :5]).all() and np.array_equal(edges[4, [0, 3, 4]], [0.0, 0.0, 0.0])
        assert np.isnan(edges[2:4, 5:]).all() and np.array_equal(edges[4, 5:], [0.0, 0.0])
        for column, method in ((0, "geodesic"), (5, "haversine"), (6, "vincenty")):
            assert same_bits(np.ascontiguousarray(edges[:, column]), oracle.geodesic_length(lines, method)), method
        assert np.isnan(direct[:4]).all()
        assert -180.0 <= direct[4, 0] < -178.0 and abs(direct[4, 1]) < 1e-9  # across the antimeridian: wrapped
        assert np.abs(direct[5] - [12.0, 34.0, 56.0]).max() < 1e-12  # no distance: the point itself
        assert 0 < rings[0, 0] < 4e12 and rings[1, 0] == -rings[0, 0] and rings[0, 1] == rings[1, 1]
