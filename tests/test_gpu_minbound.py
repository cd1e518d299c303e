"""GPU: gpk_minimum_rotated_rectangle and gpk_minimum_bounding_circle (csrc/gpk_minbound.hip) against the exact reference of
tests/minbound_ref.py — the checks of the host driver (tests/test_minbound_host.py) through the C ABI and through GeoSeries, on the
lane-group and the work-group path (hulls in LDS and beyond it), at both placements and in both coordinate layouts; the second trip of the
work-group loop; the agreement with the hull's own output and with the library's exact `contains`; and a random sweep."""
import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import DeviceGeoArray, GeoArrowArray
from geopolars_amd.geoseries import GeoSeries, minimum_bounding_circle_device, minimum_rotated_rectangle_device
from tests import exact_ref as X
from tests import minbound_ref as M
from tests import second_pass as SP
from tests.test_minbound_host import check_pins

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(M.GOLDEN)


def abi_answers(dev: DeviceGeoArray, n: int, space: str = "host", with_valid: bool = True, with_centre: bool = True):
    """(ring (n, 5, 2), rectangle valid or None, centre (n, 2) or None, radius (n,), circle valid or None) through host or device buffers"""
    if space == "host":
        ring, centre, radius = np.full((n, 5, 2), 7.0), np.full((n, 2), 7.0), np.full(n, 7.0)
        v1, v2 = np.full(n, 9, dtype=np.uint8), np.full(n, 9, dtype=np.uint8)
        lib = _abi.lib()
        _abi.check(lib.gpk_minimum_rotated_rectangle(dev.handle, ring.ctypes.data, v1.ctypes.data if with_valid else None, _abi.MEM_HOST, None))
        _abi.check(lib.gpk_minimum_bounding_circle(dev.handle, centre.ctypes.data if with_centre else None, radius.ctypes.data,
                                                   v2.ctypes.data if with_valid else None, _abi.MEM_HOST, None))
        return ring, v1 if with_valid else None, centre if with_centre else None, radius, v2 if with_valid else None
    import torch

    ring = torch.full((n, 5, 2), 7.0, dtype=torch.float64, device="cuda")
    centre = torch.full((n, 2), 7.0, dtype=torch.float64, device="cuda") if with_centre else None
    radius = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    v1 = torch.full((n,), 9, dtype=torch.uint8, device="cuda") if with_valid else None
    v2 = torch.full((n,), 9, dtype=torch.uint8, device="cuda") if with_valid else None
    minimum_rotated_rectangle_device(dev, ring, v1)
    minimum_bounding_circle_device(dev, radius, centre, v2)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return host(ring), host(v1), host(centre), host(radius), host(v2)


def separated(col: GeoArrowArray) -> DeviceGeoArray:
    """the column uploaded from separate x / y arrays"""
    import torch

    t = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device="cuda")  # noqa: E731
    x, y = t(col.xy[:, 0], np.float64), t(col.xy[:, 1], np.float64)
    return DeviceGeoArray.from_device_buffers(col.geom_type, (x, y), t(col.geom_offsets, np.int32), t(col.part_offsets, np.int32), t(col.ring_offsets, np.int32),
                                              t(col.validity, np.uint8))


def check_column(kind, rows, valid_in, answers, only=None):
    """the acceptance of tests/minbound_ref.py, row by row (`only`: these rows); returns the worst rectangle and circle errors as shares of tol"""
    ring, v1, centre, radius, v2 = answers
    worst_r = worst_c = 0.0
    for i, row in enumerate(rows):
        if only is not None and i not in only:
            continue
        has = bool(valid_in[i]) and M.has_answer(kind, row)
        assert bool(v1[i]) == has and bool(v2[i]) == has, i
        if not has:
            assert np.isnan(ring[i]).all() and np.isnan(centre[i]).all() and np.isnan(radius[i]), i
            continue
        coords = M.row_coords(kind, row)
        worst_r = max(worst_r, M.check_rectangle(coords, [tuple(p) for p in ring[i]]))
        worst_c = max(worst_c, M.check_circle(coords, centre[i, 0], centre[i, 1], radius[i]))
    return worst_r, worst_c


def same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("placement", list(M.PLACEMENTS))
@pytest.mark.parametrize("fam", list(M.FAMILIES))
def test_fixture_rows(gpk, golden, fam, placement):
    """every fixture row through the C ABI (host and device buffers, interleaved and separated coordinates, out_valid and out_center_xy
    NULL) and through GeoSeries; the rows the rules pin bit for bit; two calls give identical bits"""
    kind = M.FAMILIES[fam]
    col = M.fixture_column(golden, fam, M.PLACEMENTS[placement])
    rows, valid_in = M.column_rows(col), golden[f"{fam}_valid"]
    s = GeoSeries(col)
    n = len(s)
    got = abi_answers(s.device(), n)
    worst = check_column(kind, rows, valid_in, got)
    print(f"worst rectangle corner error: {worst[0]:.3g} of tol; worst circle error: {worst[1]:.3g} of tol")
    for other in (abi_answers(s.device(), n, "device"), abi_answers(separated(col), n), abi_answers(s.device(), n)):
        assert same_bits(got, other)  # (the same bits: another buffer space, the other layout, a second call)
    for space in ("host", "device"):
        bare = abi_answers(s.device(), n, space, with_valid=False, with_centre=False)
        assert bare[1] is None and bare[2] is None and np.array_equal(bare[0], got[0], equal_nan=True) and np.array_equal(bare[3], got[3], equal_nan=True)
    ring, v1, centre, radius, _ = got
    if placement == "lattice":
        check_pins(fam, golden[f"{fam}_names"], [(bool(v1[i]), [tuple(map(float, p)) for p in ring[i]], (float(centre[i, 0]), float(centre[i, 1]), float(radius[i])))
                                                 for i in range(n)])
    ok = v1.astype(bool)
    for series in (s.minimum_rotated_rectangle(), s.oriented_envelope()):
        a = series.array
        assert a.geom_type == M.PG and np.array_equal(a.xy, ring[ok].reshape(-1, 2)) and np.array_equal(np.diff(a.geom_offsets), ok.astype(np.int32))
        assert np.array_equal(a.ring_offsets, np.arange(0, 5 * ok.sum() + 1, 5)) and np.array_equal(a.is_valid(), col.is_valid())
    assert np.array_equal(s.minimum_bounding_radius(), radius, equal_nan=True)
    pts, r = s.minimum_bounding_circle_parts()
    assert np.array_equal(pts.array.xy, centre, equal_nan=True) and np.array_equal(pts.array.is_valid(), ok) and np.array_equal(r, radius, equal_nan=True)
    for q in (8, 3):
        a = s.minimum_bounding_circle(quad_segs=q).array if q != 8 else s.minimum_bounding_circle().array
        m = 4 * q + 1
        c = a.xy.reshape(-1, m, 2)
        assert len(c) == ok.sum() and np.array_equal(c[:, 0], c[:, -1]) and np.array_equal(np.diff(a.geom_offsets), ok.astype(np.int32))
        assert np.array_equal(c[:, 0], centre[ok] + np.stack([radius[ok], np.zeros(ok.sum())], axis=1))  # t = 0: centre + (r, 0)
        d = np.hypot(*(c - centre[ok][:, None, :]).transpose(2, 0, 1))
        assert np.allclose(d, radius[ok][:, None], rtol=1e-12, atol=1e-9 * (1 + np.abs(centre[ok]).max(initial=0.0)))
        flat = radius[ok] == 0.0
        assert (c[flat] == centre[ok][flat][:, None, :]).all()  # a radius-0 row: the point repeated


def test_lane_group_and_work_group_paths_agree(gpk):
    """a hull of 128 vertices (lane groups) and the same set with one more vertex that changes neither answer (a work-group): the exact
    answers are equal, the two kernels agree within tol.  (At 129 vertices every thread has at most one edge: its supports are walked out
    from the edge's end but never carried to a next edge; test_work_group_kernel_on_rows_that_are_no_parabolas carries them.)"""
    small = [(float(x), float(y)) for x, y in M.parabola(M.SMALL_HULL)]
    big = small + [(60.5, 60.5 * 60.5)]
    ra, rb = M.row_reference(small), M.row_reference(big)
    assert (len(ra["hull"]), len(rb["hull"])) == (M.SMALL_HULL, M.SMALL_HULL + 1)
    assert ra["min_area"] == rb["min_area"] and ra["centre"] == rb["centre"] and ra["r2"] == rb["r2"]
    for off in M.PLACEMENTS.values():
        rows = [[(x + off[0], y + off[1]) for x, y in r] for r in (small, big)]
        col = X.column(M.MPT, rows)
        got = abi_answers(GeoSeries(col).device(), 2)
        check_column(M.MPT, rows, [True, True], got)
        tol = M.tolerance(rows[0])
        ring, _, centre, radius, _ = got
        assert np.abs(ring[0] - ring[1]).max() <= tol and np.abs(centre[0] - centre[1]).max() <= tol and abs(radius[0] - radius[1]) <= tol


def test_work_group_kernel_on_rows_that_are_no_parabolas(gpk):
    """the double rows of tests/minbound_ref.py hard_rows, all above 128 hull vertices: ulp-adjacent hull vertices on a circle near the
    origin (their projections round to equal values: the calipers must not stall there), with two to four edges a thread so that the
    supports advance from edge to edge; ellipses; and a circle with a three-point support reached after at least two steps of the
    work-group's iteration.  Every row is held to the acceptance, in a column and its reverse (another work-group, the same bits)"""
    named = M.hard_rows()
    rows = [r for _, r in named]
    assert all(len(M.row_reference(r)["hull"]) > M.SMALL_HULL for r in rows) and max(len(M.row_reference(r)["hull"]) for r in rows) > 3 * M.BIG_THREADS
    got = abi_answers(GeoSeries(X.column(M.MPT, rows)).device(), len(rows))
    worst = check_column(M.MPT, rows, np.ones(len(rows), bool), got)
    print(f"hard rows: worst rectangle corner error {worst[0]:.3g} of tol; worst circle error {worst[1]:.3g} of tol")
    back = abi_answers(GeoSeries(X.column(M.MPT, rows[::-1])).device(), len(rows))
    assert same_bits(got, tuple(a[::-1] for a in back))


def test_equals_the_answer_on_the_convex_hull(gpk, golden):
    """both shapes are functions of the hull: a column and its convex_hull() answer bit for bit"""
    for fam in ("pg", "mpt", "mls"):
        for placement in M.PLACEMENTS.values():
            s = GeoSeries(M.fixture_column(golden, fam, placement))
            hull = s.convex_hull()
            a, b = abi_answers(s.device(), len(s)), abi_answers(hull.device(), len(s))
            assert same_bits(a, b), fam
            assert np.array_equal(s.minimum_rotated_rectangle().array.xy, hull.minimum_rotated_rectangle().array.xy)
            assert np.array_equal(s.minimum_bounding_radius(), hull.minimum_bounding_radius(), equal_nan=True)


def test_rectangle_contains_the_representative_point(gpk, golden):
    """the library's exact `contains` between the rectangle and the row's representative_point, for rows whose rectangle's shorter side is at
    least 1e-6 of the diagonal"""
    for placement in M.PLACEMENTS.values():
        col = M.fixture_column(golden, "pg", placement)
        s = GeoSeries(col)
        ring, valid, _, _, _ = abi_answers(s.device(), len(s))
        pts = s.representative_point()
        ok = valid.astype(bool) & pts.array.is_valid()
        side = np.minimum(np.hypot(*(ring[:, 1] - ring[:, 0]).T), np.hypot(*(ring[:, 2] - ring[:, 1]).T))
        diag = np.array([np.hypot(*(np.ptp(np.array(M.row_coords(M.PG, r)).reshape(-1, 2), axis=0))) if len(M.row_coords(M.PG, r)) else 0.0
                         for r in M.column_rows(col)])
        ok &= (side >= 1e-6 * diag) & (diag > 0)  # (a single point has no diagonal: its rectangle is the point, with no interior)
        assert ok.sum() >= 20
        rect = GeoSeries(GeoArrowArray.from_polygons([[[tuple(p) for p in r]] for r in ring[ok]], close=False))
        inside = rect.contains(GeoSeries(GeoArrowArray.from_points(pts.array.xy[ok])))
        assert inside.all(), np.flatnonzero(~inside)


def test_work_group_loop_second_trip(gpk):
    """MBG_BIG_BLOCKS + 300 rows of 129 .. 140 vertices in convex position: every work-group of the constant grid takes a second row.  The
    rows tile a small base set (never the same row twice in a row for one work-group); every base row is held to the acceptance, and
    every repeat equals its first occurrence bit for bit.  (This is about the loop over the list: at 129 .. 140 vertices a thread has at most
    one edge, so no support is carried from edge to edge here.)"""
    base = [[(float(x + 3 * k), float(y - k)) for x, y in M.parabola(M.SMALL_HULL + 1 + k)] for k in range(12)]
    assert [len(M.row_reference(r)["hull"]) for r in base] == list(range(M.SMALL_HULL + 1, M.SMALL_HULL + 13))
    n = M.BIG_BLOCKS + 300
    idx = SP.rotating_tiling(len(base), n, M.BIG_BLOCKS)
    rows = [base[i] for i in idx]
    got = abi_answers(GeoSeries(X.column(M.MPT, rows)).device(), n)
    first = {int(b): int(np.flatnonzero(idx == b)[0]) for b in range(len(base))}
    check_column(M.MPT, rows, np.ones(n, bool), got, only=set(first.values()))
    for i, b in enumerate(idx):
        j = first[int(b)]
        assert all(np.array_equal(a[i], a[j]) for a in got), (i, j)


def test_random_sweep(gpk):
    """2000 rows of 3 .. 40 random doubles at the georeferenced placement against the exact reference (which reads the doubles as
    rationals): every row passes the acceptance, no row left out"""
    rows = M.sweep_rows()
    got = abi_answers(GeoSeries(X.column(M.MPT, rows)).device(), len(rows))
    worst = check_column(M.MPT, rows, np.ones(len(rows), bool), got)
    print(f"sweep: worst rectangle corner error {worst[0]:.3g} of tol; worst circle error {worst[1]:.3g} of tol")


def test_non_finite_rows(gpk):
    nan, inf = float("nan"), float("inf")
    big = [(float(x), float(y)) for x, y in M.parabola(200)]
    for kind, rows in ((M.MPT, [[(0, 0), (4, 0), (1, 3)], [(0, 0), (nan, 0), (1, 3)], [(0, 0), (4, inf), (1, 3)], [(0, -inf)], big[:100] + [(nan, nan)] + big[100:]]),
                       (M.PG, [[[(0, 0), (4, 0), (1, 3), (0, 0)]], [[(0, 0), (4, 0), (1, nan), (0, 0)]]]), (M.PT, [(1, 2), (inf, 2), None])):
        ring, v1, centre, radius, v2 = abi_answers(GeoSeries(X.column(kind, rows)).device(), len(rows))
        assert v1[0] == 1 and v2[0] == 1 and not v1[1:].any() and not v2[1:].any()
        assert np.isnan(ring[1:]).all() and np.isnan(centre[1:]).all() and np.isnan(radius[1:]).all() and not np.isnan(ring[0]).any()
