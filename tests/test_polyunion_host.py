"""The polygon union, host side: the header's host-callable logic (csrc/gpk_polyunion.h: the kept table as a rule type and the
innermost-shell nesting, over the arc machine and the stitcher of csrc/gpk_polyclip.h) run on the CPU by a stand-alone program over
every fixture pair — plain and under AddressSanitizer + UBSan, at the lattice placement and at a georeferenced one — and the checks
that need no device: the C ABI symbols, the headers' text, the refusals of the library that come before any device work, and the Python
refusals that come before the library is opened."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import polygon_union_pairs
from tests import polyunion_ref as U
from tests.host_build import build_host_drivers, exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "polyunion", fp_contract_off=True)


@pytest.fixture(scope="module")
def golden():
    return np.load(U.GOLDEN)


@pytest.mark.parametrize("placement", ["lattice", "georeferenced"])
@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_driver_matches_the_fixture(drivers, golden, build, placement):
    """Every fixture pair: the driver gets the exact touch points of every segment of both ring walks in reverse order, with the exact
    class of every piece, and must return the reference's rings — parts, rings, coordinates per ring, ring starts and status exactly,
    input coordinates bit for bit, computed crossings within 1e-9 * d of both carrying edges."""
    built, workdir = drivers
    offset = (0.0, 0.0) if placement == "lattice" else U.TRANSLATION
    worst = 0.0
    for ka, kb in U.FAMILIES:
        ca, cb = U.load(golden, ka, kb, offset)
        for mode in U.MODES:
            fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
            with open(fin, "wb") as f:
                f.write(U.driver_records(ka, kb, mode, ca, cb))
            r = subprocess.run([built[build], fin, fout], capture_output=True, text=True)
            assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
            got, status = U.parse_driver_output(open(fout, "rb").read(), ca.n_geoms)
            worst = max(worst, U.check_result(golden, ka, kb, mode, ca, cb, got, status, offset))
    print(f"worst crossing distance / (1e-9 d), {placement}: {worst:.3e}")


def test_kept_table_and_nesting_in_the_header():
    """the rule as the new header states it, and the sentences of the old one it builds on, which stay"""
    flat = lambda name: " ".join(open(os.path.join(ROOT, "geopolars_amd", "csrc", name)).read().replace("//", " ").split())  # noqa: E731
    rule = flat("gpk_polyunion.h")
    for line in ("∂a against b EXTERIOR; BOUNDARY same side", "∂b against a EXTERIOR only", "Shared boundary comes from a, never from b",
                 "equal polygons unite to a", "Nothing is emitted backwards", "At most one arc starts at any computed crossing", "INNERMOST enclosing shell",
                 "does NOT treat an empty row as the neutral element", "1e-6 |segment|", "No covered-by claim", "correct and slow", '#include "gpk_polyclip.h"'):
        assert line in rule, line
    old = flat("gpk_polyclip.h")
    for line in ("∂a against b INTERIOR; BOUNDARY same side EXTERIOR; BOUNDARY opposite side", "each hole goes to the first shell in key order that encloses it"):
        assert line in old, line


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_exported_symbols_name_the_union_calls():
    assert "gpk_polygon_union" in _abi.EXPORTED_SYMBOLS and "gpk_union_all_pairs" in _abi.EXPORTED_SYMBOLS
    assert _abi._PROTOS["gpk_polygon_union"] == _abi._PROTOS["gpk_polygon_clip"]
    args = _abi._PROTOS["gpk_union_all_pairs"][1]
    assert len(args) == 10 and args[2] is C.c_int64 and args[3] is C.c_int64
    assert _abi.PUNION_UNION == 0


def test_built_library_exports_the_union_calls():
    from geopolars_amd import build

    names = exported_symbols()
    assert {"gpk_polygon_union", "gpk_union_all_pairs", "gpk_polygon_clip"} <= names
    assert "gpk_polyunion.hip" in build.SOURCES and "gpk_polyclip.hip" in build.SOURCES


def test_header_states_the_calls():
    flat = " ".join(open(os.path.join(ROOT, "include", "geopolars_hip.h")).read().split())
    assert ("int32_t gpk_polygon_union(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* a_rows, const uint32_t* b_rows, int64_t n_rows, "
            "int32_t rows_space, int32_t mode, int32_t flags, int32_t* out_src, int32_t src_space, uint8_t* out_status, int32_t status_space, "
            "void* stream, gpk_geoarray** out);") in flat
    assert ("int32_t gpk_union_all_pairs(const int32_t* group, const uint32_t* rows, int64_t n, int64_t base, uint32_t* a_rows, uint32_t* b_rows, "
            "int32_t* next_group, uint32_t* next_rows, int64_t* out_counts, void* stream);") in flat
    for line in ("#define GPK_PUNION_UNION 0", "does NOT treat an empty row as the neutral element", "INNERMOST shell", "an odd last row passes through"):
        assert line in flat, line


@pytest.mark.parametrize("mode,flags,src,n", [(2, 0, None, 0), (-1, 0, None, 0), (1, 0, None, 0), (0, 2, None, 0), (0, 3, None, 0), (0, 0, 64, 0), (0, 1, None, -1)])
def test_bad_plain_arguments_are_refused_by_the_library_before_any_device_work(mode, flags, src, n):
    """an unknown mode, unknown flag bits, out_src without DROP_EMPTY, a negative count: refused with not even a handle handed over"""
    out = C.c_void_p(7)
    rc = _abi.lib().gpk_polygon_union(None, None, None, None, n, _abi.MEM_HOST, mode, flags, src, _abi.MEM_HOST, None, _abi.MEM_HOST, None, C.byref(out))
    assert rc == _abi.GPK_ERR_INVALID_ARGUMENT and "polygon_union" in _abi.last_error()


def test_the_pairing_refuses_bad_sizes_and_needs_no_device_for_no_row():
    counts = (C.c_int64 * 2)(5, 5)
    lib = _abi.lib()
    assert lib.gpk_union_all_pairs(None, None, -1, 0, None, None, None, None, counts, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert lib.gpk_union_all_pairs(None, None, 4, 2**32, None, None, None, None, counts, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert lib.gpk_union_all_pairs(None, None, 4, 0, None, None, None, None, counts, None) == _abi.GPK_ERR_INVALID_ARGUMENT  # NULL lists
    assert lib.gpk_union_all_pairs(None, None, 0, 0, None, None, None, None, None, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert lib.gpk_union_all_pairs(None, None, 0, 0, None, None, None, None, counts, None) == _abi.GPK_OK and list(counts) == [0, 0]


# ---- Python: refusals before the library is opened -------------------------------------------------------------------------------------
def _series():
    pts = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]]))
    lines = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)]]))
    sq = [[(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0), (0.0, 0.0)]]
    return pts, lines, GeoSeries(GeoArrowArray.from_polygons([sq, sq, sq])), GeoSeries(GeoArrowArray.from_polygons([sq, sq]))


def test_family_shape_and_how_errors_come_before_the_device(no_device):
    pts, lines, polys, two = _series()
    for call in (lambda: polys.polygon_union(lines), lambda: lines.polygon_union(polys), lambda: pts.polygon_union(polys), lambda: polys.polygon_union(pts),
                 lambda: polygon_union_pairs(polys, lines, [0], [0]), lambda: polygon_union_pairs(lines, polys, [0], [0]), lambda: lines.union_all(),
                 lambda: pts.union_all(by=[0, 0, 1])):
        with pytest.raises(_abi.MismatchedGeometry):
            call()
    for call in (
        lambda: polys.polygon_union(two),  # 3 rows against 2
        lambda: polys.polygon_union(two, other_rows=[0, 1]),  # one entry per row of self
        lambda: polys.polygon_union(two, other_rows=["a", "b", "c"]),
        lambda: polygon_union_pairs(polys, two, [0, 1], [0]),
        lambda: polygon_union_pairs(polys, two, [0], [0], how="intersection"),
        lambda: polygon_union_pairs(polys, two, [0], [0], how="dissolve"),
        lambda: polygon_union_pairs(polys, two, ["a"], ["b"]),
    ):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            call()
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    assert pts._dev is None and lines._dev is None and polys._dev is None and two._dev is None


def test_union_all_refuses_a_by_of_the_wrong_length_or_dtype_before_the_device(no_device):
    _pts, _lines, polys, _two = _series()
    for by in ([0, 1], [0, 1, 2, 3], [0.0, 1.0, 2.0], ["a", "b", "c"], [[0, 1, 2]], np.zeros((3, 1), dtype=np.int64), [True, False, True]):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            polys.union_all(by=by)
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT, by
    assert polys._dev is None


def test_no_pair_and_no_live_row_need_no_device(no_device):
    _pts, _lines, polys, two = _series()
    out, src, status = polygon_union_pairs(polys, two, [], [], drop_empty=True, return_status=True)
    assert len(out) == 0 and len(src) == 0 and len(status) == 0 and out.array.geom_type == _abi.GEOM_MULTIPOLYGON
    none = GeoSeries(GeoArrowArray.from_polygons([[], []]))
    out, status = none.union_all(by=np.array([7, 3]), return_status=True)
    assert len(out) == 2 and out.array.geom_type == _abi.GEOM_MULTIPOLYGON and list(status) == [_abi.PCLIP_EMPTY] * 2
    assert out.array.validity is None and list(out.array.geom_offsets) == [0, 0, 0]
