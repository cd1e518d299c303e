"""The polygon clip, host side: the header's host-callable logic (csrc/gpk_polyclip.h: the kept table, the side of a shared edge, the
one value of a crossing, the arc state machine, the junction order, the stitcher) run on the CPU by a stand-alone program over every
fixture pair — plain and under AddressSanitizer + UBSan, at the lattice placement and at a georeferenced one — and the checks that need
no device: the C ABI symbol, the header's text, the refusals of the library that come before any device work, and the Python refusals
that come before the library is opened."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import polygon_clip_pairs, spatial_join_overlay
from tests import polyclip_ref as L
from tests.host_build import build_host_drivers, exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "polyclip", fp_contract_off=True)


@pytest.fixture(scope="module")
def golden():
    return np.load(L.GOLDEN)


@pytest.mark.parametrize("placement", ["lattice", "georeferenced"])
@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_driver_matches_the_fixture(drivers, golden, build, placement):
    """Every fixture pair, both modes: the driver gets the exact touch points of every segment of both ring walks in reverse order,
    with the exact class of every piece, and must return the reference's rings — parts, rings, coordinates per ring, ring starts and
    status exactly, input coordinates bit for bit, computed crossings within 1e-9 * d of both carrying edges.  The translation by
    (500000, 4649776) keeps the lattice exact: there the determinants of raw coordinates would lose the crossing parameter."""
    built, workdir = drivers
    offset = (0.0, 0.0) if placement == "lattice" else L.TRANSLATION
    worst = 0.0
    for ka, kb in L.FAMILIES:
        ca, cb = L.load(golden, ka, kb, offset)
        for mode in L.MODES:
            fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
            with open(fin, "wb") as f:
                f.write(L.driver_records(ka, kb, mode, ca, cb))
            r = subprocess.run([built[build], fin, fout], capture_output=True, text=True)
            assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
            got, status = L.parse_driver_output(open(fout, "rb").read(), ca.n_geoms)
            worst = max(worst, L.check_result(golden, ka, kb, mode, ca, cb, got, status, offset))
    print(f"worst crossing distance / (1e-9 d), {placement}: {worst:.3e}")


def test_kept_table_sides_and_junction_order_in_the_header():
    """the rule's tables as the header states them (the driver above runs them; this pins their text)"""
    rule = " ".join(open(os.path.join(ROOT, "geopolars_amd", "csrc", "gpk_polyclip.h")).read().replace("//", " ").split())
    for line in ("∂a against b INTERIOR; BOUNDARY same side EXTERIOR; BOUNDARY opposite side", "∂b against a INTERIOR only INTERIOR only, emitted backwards",
                 "Shared boundary always comes from a, never from b", "first outgoing arc met when turning clockwise", "the leftmost turn",
                 "parts of the result that touch at a point stay separate rings", "status 1", "Arcs are linked by identity, never by comparing computed coordinates",
                 "A crossing has ONE coordinate value wherever it is emitted", "correct and slow", "1e-6 |segment|", "is not enclosed by it"):
        assert line in rule, line


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_exported_symbols_name_the_clip_call():
    assert "gpk_polygon_clip" in _abi.EXPORTED_SYMBOLS
    args = _abi._PROTOS["gpk_polygon_clip"][1]
    assert len(args) == 14 and args[4] is C.c_int64
    assert (_abi.PCLIP_INTERSECTION, _abi.PCLIP_DIFFERENCE) == (0, 1)
    assert (_abi.PCLIP_OK, _abi.PCLIP_TOUCH, _abi.PCLIP_EMPTY, _abi.PCLIP_NULL, _abi.PCLIP_UNRESOLVED) == (0, 1, 2, 3, 4)


def test_built_library_exports_the_clip_call():
    from geopolars_amd import build

    assert "gpk_polygon_clip" in exported_symbols()
    assert "gpk_polyclip.hip" in build.SOURCES


def test_header_states_the_call_the_rows_and_the_contract():
    flat = " ".join(open(os.path.join(ROOT, "include", "geopolars_hip.h")).read().split())
    assert ("int32_t gpk_polygon_clip(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* a_rows, const uint32_t* b_rows, int64_t n_rows, "
            "int32_t rows_space, int32_t mode, int32_t flags, int32_t* out_src, int32_t src_space, uint8_t* out_status, int32_t status_space, "
            "void* stream, gpk_geoarray** out);") in flat
    for line in ("#define GPK_PCLIP_INTERSECTION 0", "#define GPK_PCLIP_DIFFERENCE 1", "a valid row with zero parts", "REGULARISED", "1e-9 * d",
                 "1e-6 * |segment|", "never a guessed geometry", "The call waits twice", "correct and slow", "4 unresolved"):
        assert line in flat, line


@pytest.mark.parametrize("mode,flags,src,n", [(2, 0, None, 0), (-1, 0, None, 0), (0, 2, None, 0), (1, 3, None, 0), (0, 0, 64, 0), (0, 1, None, -1)])
def test_bad_plain_arguments_are_refused_by_the_library_before_any_device_work(mode, flags, src, n):
    """an unknown mode, unknown flag bits, out_src without DROP_EMPTY, a negative count: refused with not even a handle handed over"""
    out = C.c_void_p(7)
    rc = _abi.lib().gpk_polygon_clip(None, None, None, None, n, _abi.MEM_HOST, mode, flags, src, _abi.MEM_HOST, None, _abi.MEM_HOST, None, C.byref(out))
    assert rc == _abi.GPK_ERR_INVALID_ARGUMENT and "polygon_clip" in _abi.last_error()


# ---- Python: refusals before the library is opened -------------------------------------------------------------------------------------
def _series():
    pts = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]]))
    lines = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)]]))
    sq = [[(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0), (0.0, 0.0)]]
    return pts, lines, GeoSeries(GeoArrowArray.from_polygons([sq, sq, sq])), GeoSeries(GeoArrowArray.from_polygons([sq, sq]))


def test_family_and_shape_errors_come_before_the_device(no_device):
    pts, lines, polys, two = _series()
    for call in (lambda: polys.polygon_intersection(lines), lambda: lines.polygon_intersection(polys), lambda: pts.polygon_difference(polys),
                 lambda: polys.polygon_difference(pts), lambda: polygon_clip_pairs(polys, lines, [0], [0]), lambda: polygon_clip_pairs(lines, polys, [0], [0]),
                 lambda: spatial_join_overlay(lines, polys), lambda: spatial_join_overlay(polys, pts, "difference")):
        with pytest.raises(_abi.MismatchedGeometry):
            call()
    for call in (
        lambda: polys.polygon_intersection(two),  # 3 rows against 2
        lambda: polys.polygon_intersection(two, other_rows=[0, 1]),  # one entry per row of self
        lambda: polys.polygon_difference(two, other_rows=["a", "b", "c"]),
        lambda: polygon_clip_pairs(polys, two, [0, 1], [0]),
        lambda: polygon_clip_pairs(polys, two, [0], [0], how="union"),
        lambda: polygon_clip_pairs(polys, two, ["a"], ["b"]),
        lambda: spatial_join_overlay(polys, two, how="symmetric_difference"),
    ):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            call()
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    assert pts._dev is None and lines._dev is None and polys._dev is None and two._dev is None


def test_no_pair_needs_no_device(no_device):
    _pts, _lines, polys, two = _series()
    out, src, status = polygon_clip_pairs(polys, two, [], [], drop_empty=True, return_status=True)
    assert len(out) == 0 and len(src) == 0 and len(status) == 0 and out.array.geom_type == _abi.GEOM_MULTIPOLYGON


def test_the_existing_entry_points_keep_their_refusals(no_device):
    """intersection / difference still refuse polygon x polygon: the geometry comes under the new names"""
    _pts, _lines, polys, _two = _series()
    for call in (lambda: polys.intersection(polys), lambda: polys.difference(polys)):
        with pytest.raises(_abi.MismatchedGeometry):
            call()
