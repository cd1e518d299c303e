"""Intersection area and length, host side: the kernel's pair terms (csrc/gpk_overlay.h) run on the CPU by a stand-alone program
against the exact fixture — plain and under AddressSanitizer + UBSan, at the lattice placement and at a georeferenced one — and the
checks that need no device: the C ABI symbols, the header's row rules, the refusal of a bad min_measure by the library, and the Python
family and shape refusals that come before the library is opened."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import (
    SpatialJoinIntersectionArgs,
    intersection_measure_pairs,
    intersection_measure_pairs_device,
    spatial_join_intersection,
)
from tests import overlay_ref as O
from tests.host_build import build_host_drivers, exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the kernel's math on the CPU --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "overlay", fp_contract_off=True)


@pytest.fixture(scope="module")
def golden():
    return np.load(O.GOLDEN)


def _run_driver(exe, workdir, what, a, b):
    fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
    with open(fin, "wb") as f:
        f.write(O.driver_records(0 if what == "area" else 1, a, b))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.fromfile(fout, dtype=np.float64)
    assert len(got) == a.n_geoms
    return got


@pytest.mark.parametrize("placement", ["lattice", "georeferenced"])
@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_driver_matches_the_fixture(drivers, golden, build, placement):
    """every fixture pair of every family on the CPU: |got - exact| <= 1e-9 * (d_A^2 + d_B^2) for the area, 1e-9 * length(L) for the
    length.  The translation by (500000, 4649776) keeps the lattice exact and the answers and scales unchanged: without the pair-local
    origin the Green terms there are 1e13 and the area misses the bound by orders of magnitude."""
    built, workdir = drivers
    offset = (0.0, 0.0) if placement == "lattice" else O.TRANSLATION
    worst = {}
    for what, ka, kb in O.families():
        key = O.fixture_key(what, ka, kb)
        got = _run_driver(built[build], workdir, what, O.unpack(golden, key + "a_", ka, offset), O.unpack(golden, key + "b_", kb, offset))
        exact, scale = golden[key + "exact"], golden[key + "scale"]
        assert np.isfinite(got).all() and (got >= 0).all(), key
        err = np.abs(got - exact)
        worst[key] = float(np.max(err / np.maximum(scale, 1.0)))
        bad = np.nonzero(~(err <= O.REL_TOL * scale))[0]
        assert len(bad) == 0, (key, [(int(i), got[i], exact[i], scale[i]) for i in bad[:5]])
    print({k: f"{v:.2e}" for k, v in worst.items()})


def test_host_driver_row_rules(drivers):
    """NaN for a row without a non-empty member or without a coordinate, exactly 0.0 for boxes strictly apart"""
    built, workdir = drivers
    from tests import exact_ref as X

    a = X.column(O.PG, [[O.S10], [], [O.S10]])
    b = X.column(O.PG, [[O.sq(40, 40, 50, 50)], [O.S10], [O.S10]])
    lines = X.column(O.LS, [[(0, 0), (5, 5)], [], [(20, 20), (30, 30)]])
    for exe in built.values():
        got = _run_driver(exe, workdir, "area", a, b)
        assert got[0] == 0.0 and not np.signbit(got[0]) and np.isnan(got[1]) and got[2] == 100.0
        got = _run_driver(exe, workdir, "length", lines, X.column(O.PG, [[O.S10]] * 3))
        assert abs(got[0] - 50.0**0.5) < 1e-12 and np.isnan(got[1]) and got[2] == 0.0


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_exported_symbols_name_the_intersection_calls():
    assert "gpk_intersection_measure" in _abi.EXPORTED_SYMBOLS and "gpk_intersection_measure_join" in _abi.EXPORTED_SYMBOLS
    assert len(_abi._PROTOS["gpk_intersection_measure"][1]) == 6
    args = _abi._PROTOS["gpk_intersection_measure_join"][1]
    assert len(args) == 12 and args[3] is C.c_double and args[4] is C.c_uint32


def test_built_library_exports_the_intersection_calls():
    names = exported_symbols()
    assert {"gpk_intersection_measure", "gpk_intersection_measure_join"} <= names


def test_header_states_the_calls_the_row_rules_the_tie_rule_and_the_tolerance():
    text = open(os.path.join(ROOT, "include", "geopolars_hip.h")).read()
    flat = " ".join(text.split())
    assert "int32_t gpk_intersection_measure(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* b_rows, double* out, int32_t out_space, void* stream);" in flat
    assert ("int32_t gpk_intersection_measure_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, double min_measure, "
            "uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, double* out_measure, int64_t pair_capacity, int64_t* n_pairs, "
            "int32_t out_space, void* stream);") in flat
    for line in ("null, no non-empty member (no coordinate), on either side: NaN", "a line with a NaN or infinite coordinate: NaN",
                 "an entry >= n_geoms(b) gives NaN", "|out - exact| <= 1e-9 * (d_a^2 + d_b^2)", "|out - exact| <= 1e-9 * length(a)",
                 "strictly apart give exactly 0.0", "swap the arguments", "translation of b by (+eps1, +eps2), eps1 << eps2",
                 "a pair that only touches may appear with a value at rounding level", "a stretch the line runs over twice counts twice"):
        assert line in flat, line
    kernel = " ".join(open(os.path.join(ROOT, "geopolars_amd", "csrc", "gpk_overlay.h")).read().split())
    assert "A line that runs over the same stretch twice counts it twice" in kernel and "(min, max]" in kernel and "[min, max)" in kernel


@pytest.mark.parametrize("bad", [-1.0, -1e-300, float("nan"), float("inf"), -float("inf")])
def test_bad_min_measure_is_refused_by_the_library_before_any_device_work(bad):
    lib = _abi.lib()
    n = C.c_int64(7)
    rc = lib.gpk_intersection_measure_join(None, None, None, bad, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None)  # not even a handle
    assert rc == _abi.GPK_ERR_INVALID_ARGUMENT and "min_measure" in _abi.last_error()


# ---- Python: refusals before the library is opened -------------------------------------------------------------------------------------
def _series():
    pts = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]]))
    lines = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)]]))
    sq = [[(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0), (0.0, 0.0)]]
    return pts, lines, GeoSeries(GeoArrowArray.from_polygons([sq, sq, sq])), GeoSeries(GeoArrowArray.from_polygons([sq, sq]))


def test_family_and_shape_errors_come_before_the_device(no_device):
    pts, lines, polys, two = _series()
    for call in (lambda: polys.intersection_area(lines), lambda: lines.intersection_area(polys), lambda: pts.intersection_area(polys),
                 lambda: polys.intersection_length(polys), lambda: lines.intersection_length(lines), lambda: pts.intersection_length(polys),
                 lambda: intersection_measure_pairs(polys, lines), lambda: intersection_measure_pairs(pts, polys),
                 lambda: intersection_measure_pairs(lines, lines, 1.0),
                 lambda: intersection_measure_pairs_device(polys, lines, None, 0.0, None, None)):
        with pytest.raises(_abi.MismatchedGeometry):
            call()
    with pytest.raises(_abi.MismatchedGeometry, match="swap"):
        polys.intersection_length(lines)
    with pytest.raises(_abi.MismatchedGeometry, match="swap"):
        intersection_measure_pairs(polys, lines)
    for call in (
        lambda: polys.intersection_area(two),  # 3 rows against 2
        lambda: polys.intersection_area(two, other_rows=[0, 1]),  # one entry per row of self
        lambda: lines.intersection_length(two, other_rows=[[0, 1, 0]]),
        lambda: lines.intersection_length(two, other_rows=["a", "b", "c"]),
        lambda: lines.intersection_length(two),
        lambda: intersection_measure_pairs(polys, two, -1.0),
        lambda: intersection_measure_pairs(polys, two, float("nan")),
        lambda: intersection_measure_pairs(lines, two, float("inf")),
        lambda: intersection_measure_pairs(lines, two, "much"),
    ):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            call()
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    assert pts._dev is None and lines._dev is None and polys._dev is None and two._dev is None


def test_table_join_checks_its_options_first(no_device):
    pa = pytest.importorskip("pyarrow")
    t = pa.table({"id": pa.array([0]), "geometry": pa.array([b"\x00"], type=pa.binary())})
    for opts in (SpatialJoinIntersectionArgs(join_type="outer"), SpatialJoinIntersectionArgs(min_measure=-2.0),
                 SpatialJoinIntersectionArgs(min_measure=float("nan")), SpatialJoinIntersectionArgs(measure_col=None)):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            spatial_join_intersection(t, t, opts)
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
