"""gpk_triangulate, host side: the rule of csrc/gpk_triangulate.h run on one lane by a stand-alone program — plain and under
AddressSanitizer + UBSan — over every row of the validity corpora and the real countries, held to the exact checker of
tests/triangulate_ref.py; and the checks that need no device: the C ABI symbol, the header's text, the library's refusals before any
device work and the Python refusals that come before the library is opened."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import DeviceGeoArray, GeoArrowArray
from geopolars_amd.geoseries import GeoSeries, triangulate_device
from tests import triangulate_ref as T
from tests import validity_ref as V
from tests.host_build import build_host_drivers, exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PG, MPG = V.PG, V.MPG
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "triangulate", fp_contract_off=True)


def run(exe, workdir, kind, rows, valid=None):
    fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
    with open(fin, "wb") as f:
        f.write(T.driver_records(kind, rows, valid))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    with open(fout, "rb") as f:
        return T.driver_answers(f.read(), len(rows))


def check(kind, rows, valid, codes, answers):
    """every row safe; every valid row status 0 (1 without a member) and through the checker; returns the valid rows seen"""
    n_valid = 0
    for i, (row, (st, tris)) in enumerate(zip(rows, answers)):
        ok = valid is None or valid[i]
        T.check_safe(kind, row, st, tris)
        if not T.has_member(kind, row, ok):
            assert st != T.TRI_OK, i
        if codes[i] == V.VALID:
            n_valid += 1
            assert st == (T.TRI_OK if T.has_member(kind, row, ok) else T.TRI_EMPTY), (i, st, row)
            try:
                T.check_row(kind, row, tris)
            except T.TriangulationError as e:
                raise AssertionError(f"row {i}: {e}\n{row}") from None
        elif codes[i] in (V.NULL, V.COORDINATE, V.RING_SHAPE):
            assert st == (T.TRI_EMPTY if codes[i] == V.NULL else T.TRI_FAILED), (i, st, int(codes[i]))
    return n_valid


def columns(kind):
    return [V.known_column(kind)[:3]] + [V.random_column(kind, 480, seed)[:3] for seed in (5, 6, 7)]


@pytest.mark.parametrize("build,pad", [("plain", 0), ("plain", 1), ("plain", 2), ("sanitized", 0), ("sanitized", 2)])
@pytest.mark.parametrize("kind", [PG, MPG])
def test_every_corpus_row(drivers, kind, build, pad):
    """known_column and random_column(kind, 480, seed), seeds 5 - 7, plain and padded: the valid rows (9 + 391 POLYGON, 13 + 237
    MULTIPOLYGON) pass (a) - (e); the invalid ones terminate inside their row and share, NaN / infinite / short rings are FAILED,
    null rows EMPTY"""
    built, workdir = drivers
    n_valid = 0
    for rows, valid, codes in columns(kind):
        prows = V.padded(kind, rows, pad)
        pcodes = codes
        if pad:  # (a three-coordinate ring grows into a spike: code 2 becomes 3, nothing else moves)
            pcodes = np.where(codes == V.RING_SHAPE, V.SELF_INTERSECTION, codes)
        n_valid += check(kind, prows, valid, pcodes, run(built[build], workdir, kind, prows, valid))
    assert n_valid == (400 if kind == PG else 250)


@pytest.mark.parametrize("kind", [PG, MPG])
def test_placements_and_repeats_give_identical_indices(drivers, kind):
    built, workdir = drivers
    rings = lambda row: row if kind == PG else [q for p in row for q in p]  # noqa: E731
    for rows, valid, codes in columns(kind)[:2]:
        keep = [i for i, r in enumerate(rows) if np.isfinite([v for ring in rings(r) for pt in ring for v in pt]).all()]
        rows, valid = [rows[i] for i in keep], [valid[i] for i in keep]
        base = run(built["plain"], workdir, kind, rows, valid)
        for scale, shift in V.PLACEMENTS:
            got = run(built["plain"], workdir, kind, V.placed(kind, rows, scale, shift), valid)
            assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(base, got)), (scale, shift)
        san = run(built["sanitized"], workdir, kind, rows, valid)
        assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(base, san))


def test_unusable_rows(drivers):
    built, workdir = drivers
    sq = V.sq(0, 0, 4, 4)
    rows = [[sq], [[(0, 0), (4, 0), (NAN, 4), (0, 0)]], [[(0, 0), (INF, 0), (4, 4), (0, 0)]], [sq, [(1, 1), (2, -INF), (2, 2), (1, 1)]],
            [[(0, 0), (4, 0), (0, 0)]], [[(0, 0), (4, 0), (4, 4), (0, 4)]], [[(0, 0), (4, 0), (8, 0), (0, 0)]], [[(3, 3)] * 5], [], [[]], None]
    want = [T.TRI_OK] + [T.TRI_FAILED] * 7 + [T.TRI_EMPTY] * 3
    for exe in built.values():
        got = run(exe, workdir, PG, rows)
        assert [g[0] for g in got] == want
        assert [len(g[1]) for g in got] == [2] + [0] * 10
        got = run(exe, workdir, MPG, [[[], r] if r is not None else None for r in rows] + [[[], [[]]]])
        assert [g[0] for g in got] == want + [T.TRI_EMPTY]


def test_work_group_sized_rows(drivers):
    """the six 4096-coordinate rows of the validity tests: the two valid ones pass the checker, the four faulty ones stay safe"""
    built, workdir = drivers
    rows, codes, _ = V.large_column()
    got = run(built["plain"], workdir, PG, rows)
    assert check(PG, rows, None, codes, got) == 2
    assert [len(g[1]) for g, c in zip(got, codes) if c == V.VALID] == [4093, 4099]  # N' - 2, and N' + 2 h - 2 with the hole
    san = run(built["sanitized"], workdir, PG, rows[1:4])
    assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(got[1:4], san))


def test_countries(drivers):
    """177 real rows with non-integer coordinates: every one status 0 and through the full checker"""
    built, workdir = drivers
    z = np.load(os.path.join(HERE, "golden", "naturalearth_lowres.npz"))
    kind, rows = T.array_rows(GeoArrowArray.from_wkb(z["wkb_values"], z["wkb_offsets"]))
    assert len(rows) == 177
    assert check(kind, rows, None, np.zeros(177, dtype=int), run(built["plain"], workdir, kind, rows)) == 177


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_documented():
    assert len(_abi._PROTOS["gpk_triangulate"][1]) == 8
    assert "gpk_triangulate" in exported_symbols()
    flat = " ".join(open(os.path.join(ROOT, "include", "geopolars_hip.h")).read().split())
    assert ("int32_t gpk_triangulate(const gpk_geoarray* a, uint32_t* out_index, int64_t tri_capacity, int32_t* out_tri_offsets, uint8_t* out_status, "
            "int64_t* n_triangles, int32_t out_space, void* stream);") in flat
    for line in ("#define GPK_TRI_OK 0", "#define GPK_TRI_EMPTY 1", "#define GPK_TRI_FAILED 2", "tri_capacity >= n_coords(a) + 3 * n_rings(a) always suffices",
                 "never a ring's closing coordinate", "strictly positive exact orientation", "no T-junctions", "GeoSeries.is_valid", "one read-back"):
        assert line in flat, line
    assert (_abi.TRI_OK, _abi.TRI_EMPTY, _abi.TRI_FAILED) == (T.TRI_OK, T.TRI_EMPTY, T.TRI_FAILED)
    assert "gpk_triangulate" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    header = open(os.path.join(ROOT, "geopolars_amd", "csrc", "gpk_triangulate.h")).read()
    assert f"constexpr int TRI_G_SMALL = {T.TRI_G_SMALL}, TRI_G_LARGE = {T.TRI_G_LARGE};" in header
    for v, name in ((T.TRI_SLICE_SMALL, "TRI_SLICE_SMALL"), (T.TRI_SLICE_LARGE, "TRI_SLICE_LARGE"), (T.TRI_LDS_NODES, "TRI_LDS_NODES")):
        assert f"constexpr int {name} = {v};" in header, name
    source = open(os.path.join(ROOT, "geopolars_amd", "csrc", "gpk_triangulate.hip")).read()
    assert "cu_count()" not in source + header and "group_grid(" not in source + header  # uncapped grids: one group / work-group per row


def test_refusals_come_before_any_device_work():
    """NULL arguments and a wrong family are refused on a machine without a device too: the checks come first"""
    lib = _abi.lib()
    off = (C.c_int32 * 4)()
    n = C.c_int64(-1)
    assert lib.gpk_triangulate(None, None, 0, off, None, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert "NULL" in _abi.last_error()
    fake = (C.c_int64 * 64)()  # a zeroed handle: geometry type 0, POINT — never dereferenced further
    assert lib.gpk_triangulate(fake, None, 0, None, None, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert lib.gpk_triangulate(fake, None, 0, off, None, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    for t in (_abi.GEOM_POINT, _abi.GEOM_LINESTRING, _abi.GEOM_MULTIPOINT, _abi.GEOM_MULTILINESTRING):
        C.cast(fake, C.POINTER(C.c_int32))[0] = t
        n.value = -1
        assert lib.gpk_triangulate(fake, None, 0, off, None, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
        assert n.value == 0 and "POLYGON | MULTIPOLYGON" in _abi.last_error()
    C.cast(fake, C.POINTER(C.c_int32))[0] = _abi.GEOM_POLYGON
    assert lib.gpk_triangulate(fake, None, -1, off, None, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT


# ---- Python: refusals before the library is opened -------------------------------------------------------------------------------------
def test_bad_arguments_come_before_the_device(no_device):
    s = GeoSeries(GeoArrowArray.from_polygons([[[(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 0.0)]]]))
    for bad in ("yes", 1, 0, None, 2.0, [True]):
        for call in (lambda: s.triangulate(return_status=bad), lambda: s.triangles(return_parents=bad)):
            with pytest.raises(_abi.GeopolarsHipError) as e:
                call()
            assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    for other in (GeoSeries.from_points([(0.0, 0.0)]), GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)]]))):
        for call in (other.triangulate, other.triangles):
            with pytest.raises(_abi.MismatchedGeometry):
                call()
    with pytest.raises(_abi.GeopolarsHipError) as e:
        triangulate_device(s, None, None)  # a GeoSeries is no DeviceGeoArray
    assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    with pytest.raises(_abi.MismatchedGeometry):
        triangulate_device(DeviceGeoArray(1, _abi.GEOM_POINT, 3, 3), None, None)
    dev = DeviceGeoArray(1, PG, 3, 15)  # (never dereferenced: the buffers are refused first)
    for off in (None, np.zeros(4, dtype=np.int32)):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            triangulate_device(dev, None, off)
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    dev._h = C.c_void_p()
    assert s._dev is None
