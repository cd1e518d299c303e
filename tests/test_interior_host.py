"""representative_point, host side: the kernel's rules (csrc/gpk_interior.h) run on the CPU by a stand-alone program against the exact
fixture — plain and under AddressSanitizer + UBSan, at the lattice placement and at a georeferenced one — and the checks that need no
device: the C ABI symbol, the header's rules, the library's refusal of NULL arguments, and the Python refusals that come before the
library is opened."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import DeviceGeoArray, GeoArrowArray
from geopolars_amd.geoseries import GeoSeries, representative_point_device, return_width_arg
from tests import interior_ref as I
from tests.host_build import build_host_drivers, exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "interior", fp_contract_off=True)


@pytest.fixture(scope="module")
def golden():
    return np.load(I.GOLDEN)


def _run_driver(exe, workdir, col):
    """per row: (valid, x, y, width, [(scan, crossings) per non-empty member])"""
    fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
    with open(fin, "wb") as f:
        f.write(I.driver_records(col))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    flat = np.fromfile(fout, dtype=np.float64)
    rows, k = [], 0
    while k < len(flat):
        m = int(flat[k + 4])
        rows.append((bool(flat[k]), flat[k + 1], flat[k + 2], flat[k + 3], [(flat[k + 5 + 2 * j], int(flat[k + 6 + 2 * j])) for j in range(m)]))
        k += 5 + 2 * m
    assert len(rows) == col.n_geoms
    return rows


@pytest.mark.parametrize("placement", list(I.PLACEMENTS))
@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_driver_matches_the_fixture(drivers, golden, build, placement):
    """every fixture row of every family on the CPU.  Polygonal: scanY bit-equal to the reference and the crossing count equal, member
    by member; the point's y bit-equal to a scanY; x within tol = 1e-9 * diagonal + 4 ulp(max |x|) of the midpoint of some section whose
    exact width is at least (exact maximum - tol); degenerate rows the first coordinate with width 0.  Lineal and puntal: a coordinate
    of the row bit for bit, interior whenever there is one, its exact squared distance at most the exact minimum + 1e-9 * diagonal^2."""
    built, workdir = drivers
    worst = 0.0
    for fam, kind in I.FAMILIES.items():
        col = I.fixture_column(golden, fam, I.PLACEMENTS[placement])
        rows = I.column_rows(col)
        for name, row, (ok, x, y, width, members) in zip(golden[f"{fam}_names"], rows, _run_driver(built[build], workdir, col)):
            has = len(I.row_coords(kind, row)) > 0
            assert ok == has, (fam, name)
            if not has:
                assert np.isnan(x) and np.isnan(y) and np.isnan(width), (fam, name)
                continue
            if kind in (I.PG, I.MPG):
                ref = I.polygon_row(kind, row)
                assert [(m["scan"], len(m["crossings"])) for m in ref["members"]] == members, (fam, name)
                worst = max(worst, I.check_polygon_answer(kind, row, float(x), float(y), float(width)))
            else:
                assert np.isnan(width), (fam, name)
                I.check_vertex_answer(kind, row, float(x), float(y))
    print(f"worst x error: {worst:.3g} of tol")
    assert worst <= 1.0


def test_host_driver_pins_ties_and_fallbacks(drivers, golden):
    """rows whose answer the rules fix bit for bit, at the lattice placement"""
    built, workdir = drivers
    want = {
        ("pg", "u_shape"): (1.0, 4.0, 2.0), ("pg", "ring_shape"): (1.5, 5.0, 3.0), ("pg", "l_shape"): (1.0, 4.0, 2.0),
        ("pg", "comb_17"): (0.5, 5.5, 1.0), ("pg", "comb_wide_17"): (28.0, 5.5, 2.0), ("pg", "hole2_widest_middle"): (9.5, 5.0, 11.0),
        ("pg", "flat_diagonal"): (0.0, 0.0, 0.0), ("pg", "flat_horizontal"): (0.0, 0.0, 0.0), ("pg", "flat_vertical"): (3.0, 0.0, 0.0),
        ("mpg", "equal_first_wins"): (2.5, 2.0, 5.0), ("mpg", "equal_after_narrow"): (12.5, 2.0, 5.0), ("mpg", "widest_last"): (33.5, 2.0, 7.0),
        ("mpg", "flat_then_square"): (11.0, 2.0, 2.0), ("ls", "equidistant_first_wins"): (0.0, 2.0, None), ("ls", "closed"): (4.0, 0.0, None),
        ("ls", "two_point"): (0.0, 0.0, None), ("mls", "no_interior"): (1.0, 0.0, None), ("mpt", "tie_first_wins"): (0.0, 0.0, None),
        ("mpt", "duplicates"): (4.0, 0.0, None), ("pt", "b"): (-7.0, 30.0, None),
    }
    for fam in I.FAMILIES:
        col = I.fixture_column(golden, fam)
        got = dict(zip(golden[f"{fam}_names"], _run_driver(built["plain"], workdir, col)))
        for (f, name), (x, y, w) in want.items():
            if f == fam:
                ok, gx, gy, gw, _ = got[name]
                assert ok and (gx, gy) == (x, y) and (np.isnan(gw) if w is None else gw == w), (fam, name, gx, gy, gw)


def test_host_driver_non_finite_rows(drivers):
    built, workdir = drivers
    from tests import exact_ref as X

    sq = I.rect(0, 0, 4, 4)
    bad = [list(sq)]
    bad[0][2] = (float("nan"), 4.0)
    cols = [X.column(I.PG, [[sq], bad, [[(0, 0), (float("inf"), 0), (1, 1), (0, 0)]]]), X.column(I.LS, [[(0, 0), (1, 1), (2, 0)], [(0, 0), (float("nan"), 1), (2, 0)]]),
            X.column(I.MPT, [[(0, 0)], [(0, 0), (float("-inf"), 1)]])]
    for exe in built.values():
        for col in cols:
            got = _run_driver(exe, workdir, col)
            assert got[0][0] and all(not g[0] and np.isnan(g[1]) for g in got[1:])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_documented():
    assert "gpk_representative_point" in _abi.EXPORTED_SYMBOLS and len(_abi._PROTOS["gpk_representative_point"][1]) == 6
    assert "gpk_representative_point" in exported_symbols()
    flat = " ".join(open(os.path.join(ROOT, "include", "geopolars_hip.h")).read().split())
    assert ("int32_t gpk_representative_point(const gpk_geoarray* a, double* out_xy, uint8_t* out_valid, double* out_width, int32_t out_space, "
            "void* stream);") in flat
    for line in ("scanY = (loY + hiY) / 2", "meets the line only at its upper end", "x0 + (scanY - y0) * ((x1 - x0) / (y1 - y0))",
                 "ties broken by edge index", "a later section only when strictly wider", "answers its first coordinate with out_width exactly 0",
                 "a later vertex only when strictly nearer", "A POINT answers itself", "Lineal and puntal rows give out_width = NaN",
                 "a NaN or infinite coordinate give out_valid = 0"):
        assert line in flat, line
    assert "gpk_representative_point" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_null_arguments_are_refused_by_the_library_before_any_device_work():
    lib = _abi.lib()
    xy = (C.c_double * 2)()
    assert lib.gpk_representative_point(None, xy, None, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert "NULL" in _abi.last_error()


# ---- Python: refusals before the library is opened -------------------------------------------------------------------------------------
def test_bad_arguments_come_before_the_device(no_device):
    s = GeoSeries(GeoArrowArray.from_polygons([[I.rect(0.0, 0.0, 4.0, 4.0)]]))
    for bad in ("yes", 1, None, 0.5, [True]):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            s.representative_point(return_width=bad)
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
        with pytest.raises(_abi.GeopolarsHipError):
            s.point_on_surface(bad)
    assert return_width_arg(np.True_) is True and return_width_arg(False) is False
    with pytest.raises(_abi.GeopolarsHipError) as e:
        representative_point_device(s, None)  # a GeoSeries is no DeviceGeoArray
    assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    dev = DeviceGeoArray(1, I.PG, 3, 15)  # (never dereferenced: the buffers are refused first)
    for xy in (None, np.zeros((3, 2))):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            representative_point_device(dev, xy)
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    dev._h = C.c_void_p()
    assert s._dev is None
