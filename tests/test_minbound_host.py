"""minimum_rotated_rectangle and minimum_bounding_circle, host side: the kernels' rules (csrc/gpk_minbound.h) run on the CPU by a
stand-alone program against the exact fixture — plain and under AddressSanitizer + UBSan, at the lattice placement and at a georeferenced
one — and the checks that need no device: the C ABI symbols, the header's rules, the library's refusal of NULL arguments, and the
Python refusals that come before the library is opened."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import DeviceGeoArray, GeoArrowArray
from geopolars_amd.geoseries import GeoSeries, minimum_bounding_circle_device, minimum_rotated_rectangle_device, quad_segs_arg
from tests import exact_ref as X
from tests import minbound_ref as M
from tests.host_build import build_host_drivers, exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return build_host_drivers(tmp_path_factory, "minbound", fp_contract_off=True)


@pytest.fixture(scope="module")
def golden():
    return np.load(M.GOLDEN)


def _run_driver(exe, workdir, col):
    """per row: (valid, ring of 5 (x, y), (cx, cy, radius), circle iterations, chosen edge, the full scan's ring, size of the circle's support)"""
    fin, fout = str(workdir / "in.bin"), str(workdir / "out.bin")
    with open(fin, "wb") as f:
        f.write(M.driver_records(col))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    flat = np.fromfile(fout, dtype=np.float64).reshape(-1, 27)
    assert len(flat) == col.n_geoms
    return [(bool(v[0]), [tuple(map(float, p)) for p in v[1:11].reshape(5, 2)], tuple(map(float, v[11:14])), v[14], v[15],
             [tuple(map(float, p)) for p in v[16:26].reshape(5, 2)], v[26]) for v in flat]


def _check_rows(kind, rows, valid, answers, what):
    """every row against the acceptance; returns (worst rectangle error, worst circle error) as shares of tol and the most iterations"""
    worst_r = worst_c = 0.0
    iters = 0
    for name, row, is_valid, (ok, ring, (cx, cy, rad), it, _, scan, _) in zip(what, rows, valid, answers):
        has = bool(is_valid) and M.has_answer(kind, row)
        assert ok == has, name
        if not has:
            assert np.isnan(np.array(ring)).all() and np.isnan([cx, cy, rad]).all(), name
            continue
        coords = M.row_coords(kind, row)
        worst_r = max(worst_r, M.check_rectangle(coords, ring), M.check_rectangle(coords, scan))  # (the calipers above 128 hull vertices, and the full scan)
        worst_c = max(worst_c, M.check_circle(coords, cx, cy, rad))
        iters = max(iters, int(it))
    return worst_r, worst_c, iters


@pytest.mark.parametrize("placement", list(M.PLACEMENTS))
@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_driver_matches_the_fixture(drivers, golden, build, placement):
    """every fixture row of every family on the CPU, held to the acceptance of tests/minbound_ref.py: the rectangle's corners within
    tol = 1e-9 * diagonal + 4 ulp(max |coordinate|) of the exact rectangle on an edge whose exact area is at most the exact minimum *
    (1 + 1e-9) + tol * perimeter, the ring closed bit for bit and counter-clockwise; the circle's centre and radius within tol of the exact
    ones and every coordinate within radius + tol; the circle iteration far from its bound"""
    built, workdir = drivers
    worst_r = worst_c = 0.0
    iters = 0
    for fam, kind in M.FAMILIES.items():
        col = M.fixture_column(golden, fam, M.PLACEMENTS[placement])
        r, c, it = _check_rows(kind, M.column_rows(col), col.is_valid(), _run_driver(built[build], workdir, col), [f"{fam}:{n}" for n in golden[f"{fam}_names"]])
        worst_r, worst_c, iters = max(worst_r, r), max(worst_c, c), max(iters, it)
    print(f"worst rectangle corner error: {worst_r:.3g} of tol; worst circle error: {worst_c:.3g} of tol; most circle iterations: {iters}")
    assert worst_r <= 1.0 and worst_c <= 1.0
    assert iters <= M.CIRCLE_ITERS // 2


def test_host_driver_random_sweep(drivers):
    """2000 rows of 3 .. 40 random doubles at the georeferenced placement against the exact reference (which reads the doubles as
    rationals): every row passes the acceptance — the bound is the reference's to meet"""
    built, workdir = drivers
    rows = M.sweep_rows()
    col = X.column(M.MPT, rows)
    r, c, it = _check_rows(M.MPT, rows, [True] * len(rows), _run_driver(built["plain"], workdir, col), range(len(rows)))
    print(f"sweep: worst rectangle corner error {r:.3g} of tol; worst circle error {c:.3g} of tol; most circle iterations {it}")
    assert it <= M.CIRCLE_ITERS // 2


def test_host_driver_hard_rows(drivers):
    """double rows of more than 128 hull vertices that are no parabolas (tests/minbound_ref.py hard_rows): ulp-adjacent hull vertices on a
    circle near the origin, ellipses, and a three-point circle reached in steps.  The calipers in the work-group's chunks and the full scan
    both pass the acceptance, so they agree within 2 tol; the circle of `arcs` takes at least two steps to a three-point support"""
    built, workdir = drivers
    named = M.hard_rows()
    rows = [r for _, r in named]
    assert all(len(M.row_reference(r)["hull"]) > M.SMALL_HULL for r in rows)
    assert max(len(M.row_reference(r)["hull"]) for r in rows) > 3 * M.BIG_THREADS  # (several edges a thread)
    for exe in built.values():
        got = _run_driver(exe, workdir, X.column(M.MPT, rows))
        r, c, it = _check_rows(M.MPT, rows, [True] * len(rows), got, [n for n, _ in named])
        arcs = got[[n for n, _ in named].index("arcs")]
        assert arcs[3] >= 2 and arcs[6] == 3, arcs[3:]
    print(f"hard rows: worst rectangle corner error {r:.3g} of tol; worst circle error {c:.3g} of tol; most circle iterations {it}")


PINS = {  # (family, row) -> (ring or None, (cx, cy, radius) or None), bit for bit at the lattice placement
    ("mpt", "rect_axis"): ([(0, 0), (6, 0), (6, 3), (0, 3), (0, 0)], None),  # its own hull ring
    ("pg", "diamond"): ([(0, 2), (2, 0), (4, 2), (2, 4), (0, 2)], (2.0, 2.0, 2.0)),  # its own corners: every edge ties, edge 0 wins
    ("ls", "triangle_acute"): ([(0, 0), (4, 0), (4, 3), (0, 3), (0, 0)], None),  # all three edges tie: the rectangle on edge 0
    ("mls", "triangle_right"): (None, (2.0, 1.5, 2.5)),  # between two and three support points
    ("mpt", "two_points"): ([(1, 2), (7, 10), (7, 10), (1, 2), (1, 2)], (4.0, 6.0, 5.0)),
    ("mpg", "collinear"): ([(0, 0), (4, 4), (4, 4), (0, 0), (0, 0)], (2.0, 2.0, float(np.sqrt(8.0)))),  # p q q p p
    ("pg", "single"): ([(3, 4)] * 5, (3.0, 4.0, 0.0)), ("mpt", "repeated"): ([(5, 5)] * 5, (5.0, 5.0, 0.0)),
    ("pt", "b"): ([(-7, 30)] * 5, (-7.0, 30.0, 0.0)),
    ("mpt", "circle5"): (None, (0.0, 0.0, 5.0)),
}


def check_pins(fam, names, answers):
    """answers: per row (valid, ring, (cx, cy, radius), ...)"""
    got = dict(zip(names, answers))
    for (f, name), (ring, circle) in PINS.items():
        if f != fam:
            continue
        ok, gring, gcircle = got[name][:3]
        assert ok, (fam, name)
        if ring is not None:
            assert gring == [(float(x), float(y)) for x, y in ring], (fam, name, gring)
        if circle is not None:
            assert tuple(gcircle) == circle, (fam, name, gcircle)


def test_host_driver_pins_ties_and_degenerates(drivers, golden):
    """rows whose answer the rules fix bit for bit, at the lattice placement"""
    built, workdir = drivers
    for fam in M.FAMILIES:
        col = M.fixture_column(golden, fam)
        check_pins(fam, golden[f"{fam}_names"], _run_driver(built["plain"], workdir, col))


def test_host_driver_non_finite_rows(drivers):
    built, workdir = drivers
    nan, inf = float("nan"), float("inf")
    cols = [X.column(M.MPT, [[(0, 0), (4, 0), (1, 3)], [(0, 0), (nan, 0), (1, 3)], [(0, 0), (4, inf), (1, 3)], [(0, -inf)]]),
            X.column(M.PG, [[[(0, 0), (4, 0), (1, 3), (0, 0)]], [[(0, 0), (4, 0), (1, nan), (0, 0)]]])]
    for exe in built.values():
        for col in cols:
            got = _run_driver(exe, workdir, col)
            assert got[0][0] and all(not g[0] and np.isnan(np.array(g[1])).all() and np.isnan(g[2]).all() for g in got[1:])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_documented():
    assert len(_abi._PROTOS["gpk_minimum_rotated_rectangle"][1]) == 5 and len(_abi._PROTOS["gpk_minimum_bounding_circle"][1]) == 6
    exported = exported_symbols()
    assert {"gpk_minimum_rotated_rectangle", "gpk_minimum_bounding_circle"} <= exported
    flat = " ".join(open(os.path.join(ROOT, "include", "geopolars_hip.h")).read().split())
    assert "int32_t gpk_minimum_rotated_rectangle(const gpk_geoarray* a, double* out_xy, uint8_t* out_valid, int32_t out_space, void* stream);" in flat
    assert ("int32_t gpk_minimum_bounding_circle(const gpk_geoarray* a, double* out_center_xy, double* out_radius, uint8_t* out_valid, "
            "int32_t out_space, void* stream);") in flat
    assert f"#define MBG_CIRCLE_ITERS {M.CIRCLE_ITERS}" in flat
    for line in ("u = w - a taken first", "A_i = (smax - smin) * tmax", "A_i * L2_j < A_j * L2_i", "equal areas on exactly representable data go to the lowest edge index",
                 "c2 = c1 + (tmax / L2) (-d_y, d_x)", "the fifth coordinate is the first bit for bit", "that point five times", "p q q p p",
                 "A two-point support has its midpoint as centre", "circumcentre formula on differences",
                 "radius exactly 0", "a NaN or infinite coordinate give out_valid = 0", "a circle that still contains the row"):
        assert line in flat, line
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "gpk_minimum_rotated_rectangle" in text and "gpk_minimum_bounding_circle" in text
    header = open(os.path.join(ROOT, "geopolars_amd", "csrc", "gpk_minbound.h")).read()
    for v, name in ((M.G, "MBG_G"), (M.SMALL_HULL, "MBG_SMALL_HULL"), (M.BIG_THREADS, "MBG_BIG_THREADS"), (M.BIG_BLOCKS, "MBG_BIG_BLOCKS"), (M.LDS_HULL, "MBG_LDS_HULL")):
        assert f"constexpr int {name} = {v};" in header, name


def test_null_arguments_are_refused_by_the_library_before_any_device_work():
    lib = _abi.lib()
    buf = (C.c_double * 10)()
    for call in (lambda: lib.gpk_minimum_rotated_rectangle(None, buf, None, _abi.MEM_HOST, None),
                 lambda: lib.gpk_minimum_bounding_circle(None, buf, buf, None, _abi.MEM_HOST, None)):
        assert call() == _abi.GPK_ERR_INVALID_ARGUMENT
        assert "NULL" in _abi.last_error()


# ---- Python: refusals before the library is opened -------------------------------------------------------------------------------------
def test_bad_arguments_come_before_the_device(no_device):
    s = GeoSeries(GeoArrowArray.from_polygons([[[(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 0.0)]]]))
    for bad in ("8", 0, 257, -1, 2.0, None, True, [8]):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            s.minimum_bounding_circle(quad_segs=bad)
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    assert quad_segs_arg(np.int64(256)) == 256 and quad_segs_arg(1) == 1
    for fn in (minimum_rotated_rectangle_device, minimum_bounding_circle_device):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            fn(s, None)  # a GeoSeries is no DeviceGeoArray
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    dev = DeviceGeoArray(1, M.PG, 3, 15)  # (never dereferenced: the buffers are refused first)
    for out in (None, np.zeros((3, 5, 2)), np.zeros(3)):
        for fn in (minimum_rotated_rectangle_device, minimum_bounding_circle_device):
            with pytest.raises(_abi.GeopolarsHipError) as e:
                fn(dev, out)
            assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    dev._h = C.c_void_p()
    assert s._dev is None
