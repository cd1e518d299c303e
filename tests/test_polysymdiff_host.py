"""The polygon symmetric difference, host side: the header's host-callable logic (csrc/gpk_polysymdiff.h: the table with the direction
of a piece by its class, over the arc machine with direction changes, the junction at computed crossings and the stitcher of
csrc/gpk_polyclip.h) run on the CPU by a stand-alone program over every fixture pair — plain and under AddressSanitizer + UBSan, at the
lattice placement and at a georeferenced one, and with a and b exchanged — and the checks that need no device: the C ABI symbols, the
headers' text, the refusals of the library that come before any device work, and the Python refusals that come before the library is
opened."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import polygon_symdiff_pairs
from tests import polysymdiff_ref as S
from tests.host_build import build_host_drivers, exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "polysymdiff", fp_contract_off=True)


@pytest.fixture(scope="module")
def golden():
    return np.load(S.GOLDEN)


def run_driver(exe, workdir, records, n):
    fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
    with open(fin, "wb") as f:
        f.write(records)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return S.parse_driver_output(open(fout, "rb").read(), n)


@pytest.mark.parametrize("placement", ["lattice", "georeferenced"])
@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_driver_matches_the_fixture(drivers, golden, build, placement):
    """Every fixture pair: the driver gets the exact touch points of every segment of both ring walks in reverse order, with the exact
    class of every piece, and must return the reference's rings — parts, rings, coordinates per ring, ring starts and status exactly,
    input coordinates bit for bit, computed crossings within 1e-9 * d of both carrying edges."""
    built, workdir = drivers
    offset = (0.0, 0.0) if placement == "lattice" else S.TRANSLATION
    worst = 0.0
    for ka, kb in S.FAMILIES:
        ca, cb = S.load(golden, ka, kb, offset)
        got, status = run_driver(built[build], workdir, S.driver_records(ka, kb, S.SYMDIFF, ca, cb), ca.n_geoms)
        worst = max(worst, S.check_result(golden, ka, kb, S.SYMDIFF, ca, cb, got, status, offset))
    print(f"worst crossing distance / (1e-9 d), {placement}: {worst:.3e}")


def test_host_driver_counts_the_arcs_the_reference_counts(drivers, golden):
    """The number of arcs the header's walks hand to the sink is the reference's, pair by pair: on every fixture pair of one family,
    and on the pairs tests/test_gpu_polysymdiff.py puts on either side of the stitch's LDS slice — 7, 8, 9 arcs and 31, 32, 33, which
    that test takes from the reference."""
    import re

    from tests import exact_ref as X

    built, workdir = drivers
    arcs_file = str(workdir / "arcs.bin")

    def counts(records, n):
        fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
        with open(fin, "wb") as f:
            f.write(records)
        r = subprocess.run([built["sanitized"], fin, fout, arcs_file], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        got = np.fromfile(arcs_file, dtype=np.int32)
        assert len(got) == n
        return got.tolist()

    ka, kb = S.MPG, S.MPG
    ca, cb = S.load(golden, ka, kb)
    A, B, av, bv, _names = S.rows(ka, kb)
    want = [S.arc_count(ka, a, kb, b) if S.results(ka, kb)[i][0] is not None else -1 for i, (a, b) in enumerate(zip(A, B))]
    assert counts(S.driver_records(ka, kb, S.SYMDIFF, ca, cb), ca.n_geoms) == want and max(want) > 8
    per_lane = int(re.search(r"constexpr int STITCH_LDS_ARCS_PER_LANE = (\d+);",
                             open(os.path.join(ROOT, "geopolars_amd", "csrc", "gpk_polyclip_run.h")).read()).group(1))
    for lanes, shapes in S.SLICE_SHAPES.items():
        pairs = [S.comb_pair(teeth, free) for teeth, free in shapes]
        rows = ([a for a, _b in pairs], [b for _a, b in pairs], [1] * 3, [1] * 3, None)
        xa, xb = X.column(S.MPG, rows[0]), X.column(S.PG, rows[1])
        got = counts(S.driver_records(S.MPG, S.PG, S.SYMDIFF, xa, xb, rows), 3)
        assert got == [per_lane * lanes - 1, per_lane * lanes, per_lane * lanes + 1] == [S.arc_count(S.MPG, a, S.PG, b) for a, b in pairs], (lanes, got)


def rows_of(col, status):
    """every row of a MULTIPOLYGON column as parts -> rings -> coordinate tuples (None: a null row)"""
    g, p, r, xy = col.geom_offsets, col.part_offsets, col.ring_offsets, col.xy
    out = []
    for i in range(col.n_geoms):
        if status[i] in (S.ST_NULL, S.ST_UNRESOLVED):
            out.append(None)
            continue
        out.append([[[tuple(v) for v in xy[r[k]:r[k + 1]].tolist()] for k in range(p[j], p[j + 1])] for j in range(g[i], g[i + 1])])
    return out


@pytest.mark.parametrize("placement", ["lattice", "georeferenced"])
def test_host_driver_gives_the_same_rings_for_b_a(drivers, golden, placement):
    """The swap property: the result for (b, a) has the rings of the result for (a, b), up to ring rotation and part order.  Input
    coordinates are compared bit for bit.  The one value of a crossing is taken along the edge of the FIRST operand, so a crossing of
    (b, a) is the crossing of (a, b) only up to the bound on either: each is matched to the nearest one within 2e-9 * d."""
    built, workdir = drivers
    offset = (0.0, 0.0) if placement == "lattice" else S.TRANSLATION
    for ka, kb in S.FAMILIES:
        ca, cb = S.load(golden, ka, kb, offset)
        ab, st_ab = run_driver(built["plain"], workdir, S.driver_records(ka, kb, S.SYMDIFF, ca, cb), ca.n_geoms)
        ba, st_ba = run_driver(built["plain"], workdir, S.driver_records(kb, ka, S.SYMDIFF, cb, ca, S.swapped_rows(ka, kb)), ca.n_geoms)
        assert (st_ab == st_ba).all()
        diag = S.L.pair_diagonals(ca, cb)
        inputs = set(map(tuple, ca.xy.tolist())) | set(map(tuple, cb.xy.tolist()))
        for i, (u, v) in enumerate(zip(rows_of(ab, st_ab), rows_of(ba, st_ba))):
            assert (u is None) == (v is None), i
            if u is None:
                continue
            computed = {pt for part in u for ring in part for pt in ring if pt not in inputs}

            def snap(pt):
                if pt in inputs:
                    return pt
                near = min(computed, key=lambda c: max(abs(c[0] - pt[0]), abs(c[1] - pt[1])))
                assert max(abs(near[0] - pt[0]), abs(near[1] - pt[1])) <= 2e-9 * diag[i], (i, pt, near)
                return near

            assert S.canonical(u) == S.canonical([[[snap(pt) for pt in ring] for ring in part] for part in v]), i


def test_rule_in_the_headers():
    """the rule as the new header states it, and the sentences of the old ones it builds on, which stay"""
    flat = lambda name: " ".join(open(os.path.join(ROOT, "geopolars_amd", "csrc", name)).read().replace("//", " ").split())  # noqa: E731
    rule = flat("gpk_polysymdiff.h")
    for line in ("∂a against b kept, emitted forwards kept, emitted BACKWARDS dropped", "∂b against a kept, emitted forwards kept, emitted BACKWARDS dropped",
                 "equal polygons give an empty row", "neighbours that share an edge give their union", "a hole of b is then a shell inside that hole",
                 "Key convention: the key of an arc is that of its start in the emitted direction", "ARC_WHOLE | ARC_BACKWARDS", "two arcs END",
                 "INNERMOST enclosing shell", "not treated as the neutral element", "without the covered-by claim", '#include "gpk_polyclip.h"'):
        assert line in rule, line
    old = flat("gpk_polyclip.h")
    for line in ("∂a against b INTERIOR; BOUNDARY same side EXTERIOR; BOUNDARY opposite side", "each hole goes to the first shell in key order that encloses it",
                 "Rule::DIRECTION_BY_CLASS", "rekey(int key)", "CROSSINGS (gpk_polysymdiff.h"):
        assert line in old, line
    assert "At most one arc starts at any computed crossing" in flat("gpk_polyunion.h")
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())
    assert "### 4.3w" in design and "gpk_polygon_symdiff" in design


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_exported_symbols_name_the_call():
    assert "gpk_polygon_symdiff" in _abi.EXPORTED_SYMBOLS
    assert _abi._PROTOS["gpk_polygon_symdiff"] == _abi._PROTOS["gpk_polygon_clip"]
    assert _abi.PSYMDIFF_SYMMETRIC_DIFFERENCE == 0


def test_built_library_exports_the_call():
    from geopolars_amd import build

    assert {"gpk_polygon_symdiff", "gpk_polygon_union", "gpk_polygon_clip"} <= exported_symbols()
    assert "gpk_polysymdiff.hip" in build.SOURCES


def test_header_states_the_call():
    flat = " ".join(open(os.path.join(ROOT, "include", "geopolars_hip.h")).read().split())
    assert ("int32_t gpk_polygon_symdiff(const gpk_geoarray* a, const gpk_geoarray* b, const uint32_t* a_rows, const uint32_t* b_rows, int64_t n_rows, "
            "int32_t rows_space, int32_t mode, int32_t flags, int32_t* out_src, int32_t src_space, uint8_t* out_status, int32_t status_space, "
            "void* stream, gpk_geoarray** out);") in flat
    for line in ("#define GPK_PSYMDIFF_SYMMETRIC_DIFFERENCE 0", "NOT treated as the neutral element", "INNERMOST shell", "No covered-by claim",
                 "touch at the crossing and stay separate rings"):
        assert line in flat, line


@pytest.mark.parametrize("mode,flags,src,n", [(2, 0, None, 0), (-1, 0, None, 0), (1, 0, None, 0), (0, 2, None, 0), (0, 3, None, 0), (0, 0, 64, 0), (0, 1, None, -1)])
def test_bad_plain_arguments_are_refused_by_the_library_before_any_device_work(mode, flags, src, n):
    """an unknown mode, unknown flag bits, out_src without DROP_EMPTY, a negative count: refused with not even a handle handed over"""
    out = C.c_void_p(7)
    rc = _abi.lib().gpk_polygon_symdiff(None, None, None, None, n, _abi.MEM_HOST, mode, flags, src, _abi.MEM_HOST, None, _abi.MEM_HOST, None, C.byref(out))
    assert rc == _abi.GPK_ERR_INVALID_ARGUMENT and "polygon_symdiff" in _abi.last_error()


# ---- Python: refusals before the library is opened -------------------------------------------------------------------------------------
def _series():
    pts = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]]))
    lines = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)]]))
    sq = [[(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0), (0.0, 0.0)]]
    return pts, lines, GeoSeries(GeoArrowArray.from_polygons([sq, sq, sq])), GeoSeries(GeoArrowArray.from_polygons([sq, sq]))


def test_family_shape_and_how_errors_come_before_the_device(no_device):
    pts, lines, polys, two = _series()
    for call in (lambda: polys.polygon_symmetric_difference(lines), lambda: lines.polygon_symmetric_difference(polys),
                 lambda: pts.polygon_symmetric_difference(polys), lambda: polys.polygon_symmetric_difference(pts),
                 lambda: polygon_symdiff_pairs(polys, lines, [0], [0]), lambda: polygon_symdiff_pairs(lines, polys, [0], [0])):
        with pytest.raises(_abi.MismatchedGeometry):
            call()
    for call in (
        lambda: polys.polygon_symmetric_difference(two),  # 3 rows against 2
        lambda: polys.polygon_symmetric_difference(two, other_rows=[0, 1]),  # one entry per row of self
        lambda: polys.polygon_symmetric_difference(two, other_rows=["a", "b", "c"]),
        lambda: polygon_symdiff_pairs(polys, two, [0, 1], [0]),
        lambda: polygon_symdiff_pairs(polys, two, [0], [0], how="union"),
        lambda: polygon_symdiff_pairs(polys, two, [0], [0], how="xor"),
        lambda: polygon_symdiff_pairs(polys, two, ["a"], ["b"]),
    ):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            call()
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    assert pts._dev is None and lines._dev is None and polys._dev is None and two._dev is None


def test_no_pair_needs_no_device(no_device):
    _pts, _lines, polys, two = _series()
    out, src, status = polygon_symdiff_pairs(polys, two, [], [], drop_empty=True, return_status=True)
    assert len(out) == 0 and len(src) == 0 and len(status) == 0 and out.array.geom_type == _abi.GEOM_MULTIPOLYGON
