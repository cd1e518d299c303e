"""GPU: gpk_geodesic_area / gpk_geodesic_inverse / gpk_geodesic_direct against the mp fixture tests/golden/geodesic_measures_mp.npz, within
GPU_FACTOR times the tolerances measured on the CPU (tests/geodesic_measure_ref.py), and every layout the strip schedule of the area
kernel can meet, built by tiling fixture rings into columns: the expected row value is the fold of the fixture's ring values."""
import os

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries, geodesic_area_device, geodesic_destination_device, geodesic_inverse_device
from tests import geodesic_measure_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STRIP = 256  # ga::STRIP of csrc/gpk_geodesic.hip: coordinates a work-group
F = R.GPU_FACTOR


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture(os.path.join(HERE, "golden", "geodesic_measures_mp.npz"))


def points(xy, validity=None):
    return GeoSeries(GeoArrowArray.from_points(np.ascontiguousarray(xy), validity=validity))


# ---- inverse and direct ------------------------------------------------------------------------------------------------------------
def test_inverse_fixture_edges(gpk, fx):
    a, b = points(fx["edge_xy"][:, :2]), points(fx["edge_xy"][:, 2:])
    s12, azi1, azi2 = a.geodesic_distance(b), a.geodesic_bearing(b), a.geodesic_bearing(b, final=True)
    R.check_edges(fx, s12, azi1, azi2, None, factor=F)
    assert np.all((azi1 >= -180) & (azi1 <= 180) & (azi2 >= -180) & (azi2 <= 180))
    # all three outputs in one call give the same bits as one at a time
    n = len(s12)
    out = np.empty((3, n))
    _abi.check(gpk.lib().gpk_geodesic_inverse(a.device().handle, b.device().handle, None, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data,
                                              _abi.MEM_HOST, None))
    assert np.array_equal(out, np.stack([s12, azi1, azi2]))


def test_geodesic_length_and_distance_are_one_inverse(gpk, fx):
    """geodesic_length("geodesic") of two-point linestrings and geodesic_distance of the same end points run the same inverse
    (csrc/gpk_geodesic.h): the same bits and the same NaN rows, on the fixture's edges and on the hand-made ones"""
    nan = np.nan
    hand = np.array([[12.5, -33.25, 12.5, -33.25],  # identical points
                     [0.0, 90.0, 0.0, -90.0],  # pole to pole
                     [0.0, 0.0, 179.5, 0.5],  # Karney 2013's nearly antipodal pair
                     [0.0, 0.0, 180.0, 0.0],  # antipodal on the equator
                     [0.0, 90.0001, 1.0, 0.0],  # a latitude out of range
                     [nan, 0.0, 1.0, 1.0]])  # a NaN coordinate
    e = np.concatenate([fx["edge_xy"], hand])
    n = len(e)
    lines = GeoSeries(GeoArrowArray(_abi.GEOM_LINESTRING, np.ascontiguousarray(e).reshape(2 * n, 2), geom_offsets=np.arange(0, 2 * n + 1, 2, dtype=np.int32)))
    length = lines.geodesic_length("geodesic")
    s12 = points(e[:, :2]).geodesic_distance(points(e[:, 2:]))
    bad = np.isnan(length)
    assert np.array_equal(np.isnan(s12), bad) and np.array_equal(np.flatnonzero(bad), [n - 2, n - 1])
    assert np.array_equal(length[~bad].view(np.uint64), s12[~bad].view(np.uint64))
    assert length[n - 6] == 0.0 and np.all(length[n - 5:n - 2] > 1.99e7)


def test_direct_fixture_and_round_trip(gpk, fx):
    din = fx["direct_in"]
    a = points(din[:, :2])
    dest = a.geodesic_destination(din[:, 2], din[:, 3])
    n = len(din)
    azi2 = np.empty(n)
    xy = np.empty((n, 2))
    azi1, s12 = np.ascontiguousarray(din[:, 2]), np.ascontiguousarray(din[:, 3])  # (named: they must outlive the call)
    _abi.check(gpk.lib().gpk_geodesic_direct(a.device().handle, azi1.ctypes.data, n, s12.ctypes.data, n, xy.ctypes.data, azi2.ctypes.data, _abi.MEM_HOST, None))
    assert np.array_equal(xy, dest.array.xy) and np.all(np.abs(xy[:, 0]) <= 180)
    R.check_direct(fx, xy, azi2, factor=F)
    # inverse(direct(p)): where the run is a shortest geodesic (the reference's arc is under pi and its longitude step under 180 degrees
    # would be the full rule; distances up to 19 000 km are safely that), the distance comes back within the Karney bound
    short = (din[:, 3] >= 0) & (din[:, 3] <= 1.9e7)
    back = a.geodesic_distance(dest)
    assert short.sum() > 300 and np.all(np.abs(back[short] - din[short, 3]) <= R.karney_bound_m(din[short, 3]) + F * R.DIRECT_ERR_M)
    bearing = a.geodesic_bearing(dest)
    far = short & (din[:, 3] > 1e3)
    m12 = 6.4e6  # (an upper bound of the reduced length)
    assert np.all(np.abs(R.wrap180(bearing[far] - din[far, 2])) * (np.pi / 180) * np.minimum(din[far, 3], m12) <= F * (R.AZIMUTH_ERR_M["whole"] + R.DIRECT_ERR_M))


def test_b_rows_broadcast_nan_and_range_rules(gpk, fx):
    e = fx["edge_xy"][:40]
    valid = np.ones(40, dtype=bool)
    valid[5] = False
    bxy = e[:, 2:].copy()
    bxy[7] = np.nan  # an empty point
    bxy[9, 1] = 90.5  # a latitude out of range
    a, b = points(e[:, :2]), points(bxy[::-1].copy(), validity=np.packbits(valid[::-1], bitorder="little"))
    rows = np.arange(39, -1, -1, dtype=np.uint32)
    rows[11] = 40  # out of range
    got = a.geodesic_distance(b, other_rows=rows)
    bad = np.zeros(40, dtype=bool)
    bad[[5, 7, 9, 11]] = True
    assert np.array_equal(np.isnan(got), bad) and np.all(np.abs(got[~bad] - fx["edge_s12"][:40][~bad]) <= R.karney_bound_m(fx["edge_s12"][:40][~bad]))
    assert np.array_equal(np.isnan(a.geodesic_bearing(b, other_rows=rows)), bad)
    # b_rows lets the columns differ in length; without it they may not
    assert len(points(e[:3, :2]).geodesic_distance(b, other_rows=[0, 1, 2])) == 3
    assert gpk.lib().gpk_geodesic_inverse(points(e[:3, :2]).device().handle, b.device().handle, None, None, None, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    # direct: one value for every row, or one a row; NaN rules
    din = fx["direct_in"][:30]
    p = points(din[:, :2], validity=np.packbits(np.arange(30) != 3, bitorder="little"))
    one = p.geodesic_destination(45.0, 1000.0).array.xy
    each = p.geodesic_destination(np.full(30, 45.0), np.full(30, 1000.0)).array.xy
    mixed = p.geodesic_destination(45.0, np.full(30, 1000.0)).array.xy
    assert np.array_equal(one, each, equal_nan=True) and np.array_equal(one, mixed, equal_nan=True) and np.isnan(one[3]).all() and np.isfinite(np.delete(one, 3, 0)).all()
    az = np.full(30, 45.0)
    az[4], az[6] = np.nan, np.inf
    s = np.full(30, 1000.0)
    s[8] = np.nan
    got = p.geodesic_destination(az, s).array.xy
    assert np.array_equal(np.isnan(got[:, 0]), np.isin(np.arange(30), [3, 4, 6, 8]))
    lines = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)]]))
    one_pt = points([[0.0, 0.0]])
    assert gpk.lib().gpk_geodesic_inverse(lines.device().handle, one_pt.device().handle, None, None, None, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    z = np.zeros(2)
    assert gpk.lib().gpk_geodesic_direct(lines.device().handle, z.ctypes.data, 1, z.ctypes.data, 1, z.ctypes.data, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    assert gpk.lib().gpk_geodesic_direct(one_pt.device().handle, z.ctypes.data, 2, z.ctypes.data, 1, z.ctypes.data, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert gpk.lib().gpk_geodesic_area(one_pt.device().handle, 2, z.ctypes.data, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT


# ---- area and perimeter ----------------------------------------------------------------------------------------------------------------
def column(fx, rows, multi):
    """rows[i] = None (a null row) or a list of parts, a part a list of fixture ring numbers (the first is the shell); POLYGON columns take
    one part a row"""
    xy, ring_off, part_off, geom_off = [], [0], [0], [0]
    for row in rows:
        for part in row or []:
            for r in part:
                c = fx["ring_xy"][fx["ring_off"][r]:fx["ring_off"][r + 1]]
                xy.append(c)
                ring_off.append(ring_off[-1] + len(c))
            part_off.append(len(ring_off) - 1)
        geom_off.append(len(part_off) - 1 if multi else len(ring_off) - 1)
        assert multi or row is None or len(row) <= 1
    xy = np.concatenate(xy) if xy else np.zeros((0, 2))
    validity = None
    if any(r is None for r in rows):
        validity = np.packbits([r is not None for r in rows], bitorder="little")
    if multi:
        return GeoArrowArray(_abi.GEOM_MULTIPOLYGON, xy, geom_offsets=geom_off, part_offsets=part_off, ring_offsets=ring_off, validity=validity)
    return GeoArrowArray(_abi.GEOM_POLYGON, xy, geom_offsets=geom_off, ring_offsets=ring_off, validity=validity)


def expected(fx, rows):
    """(signed, unsigned, perimeter, area bound, perimeter bound) of every row: the fold of the fixture's ring values and of their bounds"""
    ba, bp = R.ring_bounds(fx, F)
    out = np.zeros((5, len(rows)))
    for i, row in enumerate(rows):
        if row is None:
            out[:3, i] = np.nan
            continue
        for part in row:
            for k, r in enumerate(part):
                out[0, i] += fx["ring_area"][r]
                out[1, i] += abs(fx["ring_area"][r]) if k == 0 else -abs(fx["ring_area"][r])
                out[2, i] += fx["ring_perimeter"][r]
                out[3, i] += ba[r]
                out[4, i] += bp[r]
    return out


def assert_rows(fx, rows, signed, unsigned, perimeter):
    e = expected(fx, rows)
    null = np.array([r is None for r in rows])
    for got, want, bound in ((signed, e[0], e[3]), (unsigned, e[1], e[3]), (perimeter, e[2], e[4])):
        if got is None:
            continue
        assert np.array_equal(np.isnan(got), null)
        bad = np.flatnonzero(~null & ~(np.abs(got - want) <= bound))
        assert len(bad) == 0, (bad[:5], got[bad[:5]], want[bad[:5]], bound[bad[:5]])


@pytest.mark.parametrize("multi", [False, True])
def test_fixture_rings_area_and_perimeter(gpk, fx, multi):
    rows = [[[r]] for r in range(len(fx["ring_area"]))]
    s = GeoSeries(column(fx, rows, multi))
    signed, unsigned, per = s.geodesic_area(signed=True), s.geodesic_area(), s.geodesic_perimeter()
    R.check_rings(fx, signed, per, factor=F)
    assert_rows(fx, rows, signed, unsigned, per)
    assert np.array_equal(unsigned, np.abs(signed))
    # the closed forms themselves: the octant and its reverse
    i = int(np.flatnonzero(fx["ring_regime"] == R.RING_REGIMES.index("closed_form"))[0])
    assert abs(signed[i] - 63758202715511.0637) <= 0.1 and abs(signed[i + 1] + 63758202715511.0637) <= 0.1


def layout_rows(fx, multi):
    """a column of a few thousand coordinates that meets every case of the strip schedule (asserted in the test from its offsets)"""
    rng = np.random.default_rng(3)
    length = np.diff(fx["ring_off"])
    by_len = {}
    for r in np.flatnonzero(length < 30):
        by_len.setdefault(int(length[r]), []).append(int(r))
    rows, pos = [], 0

    def add(row):
        nonlocal pos
        rows.append(row)
        pos += sum(int(length[r]) for part in row or [] for r in part)

    def fill_to(target):  # single-ring rows that end exactly at `target`
        while pos < target:
            left = target - pos
            if left in by_len:
                L = left
            else:
                L = int(rng.choice([k for k in by_len if left - k >= 4 or left == k] if left < 40 else list(by_len)))
            add([[int(rng.choice(by_len[L]))]])
        assert pos == target

    four = by_len[4]
    for i in range(16):  # strip 0: full of 4-coordinate rings, a shell and three holes a row
        add([[four[(4 * i + k) % len(four)] for k in range(4)]])
    assert pos == STRIP
    add([] if multi else [[]])  # an empty geometry (and, in a polygon column, an empty part) whose position is a strip base
    fill_to(2 * STRIP)  # ... the last ring ends exactly at a strip boundary
    add([[]] if multi else [[]])
    for _ in range(12):  # shells with holes, rows of several parts: rings straddle the next boundaries
        k = [int(rng.choice(by_len[int(rng.choice(list(by_len)))])) for _ in range(int(rng.integers(2, 6)))]
        add([k[:2], [], k[2:]] if multi and len(k) > 2 else [k])
    dense = [int(r) for r in np.flatnonzero(length > 1000)]
    add([[dense[0], four[0]]])  # one ring longer than two strips, with a hole
    add(None)
    add([[dense[1]]])
    fill_to((pos // STRIP + 2) * STRIP)  # the coordinate count is exactly k * STRIP ...
    add([] if multi else [[]])  # ... followed by empty and null rows
    add(None)
    add([] if multi else [[]])
    return rows


@pytest.mark.parametrize("multi", [False, True])
def test_layouts_of_the_strip_schedule(gpk, fx, multi):
    import torch

    rows = layout_rows(fx, multi)
    col = column(fx, rows, multi)
    ro, n = col.ring_offsets.astype(np.int64), len(rows)
    nonempty = ro[1:] > ro[:-1]
    assert len(col.xy) % STRIP == 0 and 2000 < len(col.xy) < 8000 and rows[-1] == ([] if multi else [[]]) and rows[-2] is None
    assert np.any((ro[1:] % STRIP == 0) & nonempty)  # a ring ending exactly at a strip boundary
    assert np.any((ro[:-1] // STRIP != (ro[1:] - 1) // STRIP) & nonempty & (np.diff(ro) < 30))  # a short ring straddling one
    assert np.any((ro[1:] - 1) // STRIP - ro[:-1] // STRIP >= 3)  # a ring longer than two strips
    assert np.all(np.diff(ro[:65]) == 4) and ro[64] == STRIP  # a strip full of 4-coordinate rings
    assert rows[16] in ([], [[]]) and ro[64] == STRIP  # an empty geometry whose position is a strip base
    assert col.validity is not None
    s = GeoSeries(col)
    signed, unsigned, per = s.geodesic_area(signed=True), s.geodesic_area(), s.geodesic_perimeter()
    assert_rows(fx, rows, signed, unsigned, per)
    # both outputs in one call, host and device space, each pointer NULL in turn: the same bits
    lib, h = gpk.lib(), s.device().handle
    for flags, area in ((_abi.GEODESIC_AREA_SIGNED, signed), (0, unsigned)):
        a, p = np.empty(n), np.empty(n)
        _abi.check(lib.gpk_geodesic_area(h, flags, a.ctypes.data, p.ctypes.data, _abi.MEM_HOST, None))
        assert np.array_equal(a, area, equal_nan=True) and np.array_equal(p, per, equal_nan=True)
        ta, tp = torch.full((n,), 7.0, dtype=torch.float64, device="cuda"), torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
        geodesic_area_device(s.device(), ta, tp, signed=bool(flags))
        torch.cuda.synchronize()
        assert np.array_equal(ta.cpu().numpy(), area, equal_nan=True) and np.array_equal(tp.cpu().numpy(), per, equal_nan=True)
        ta2, tp2 = torch.full((n,), 7.0, dtype=torch.float64, device="cuda"), torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
        geodesic_area_device(s.device(), ta2, None, signed=bool(flags))
        geodesic_area_device(s.device(), None, tp2)
        torch.cuda.synchronize()
        assert torch.equal(ta2.nan_to_num(1.0), ta.nan_to_num(1.0)) and torch.equal(tp2.nan_to_num(1.0), tp.nan_to_num(1.0))
    _abi.check(lib.gpk_geodesic_area(h, 0, None, None, _abi.MEM_HOST, None))  # nothing asked for: nothing done
    # two identical calls: the same bits
    assert np.array_equal(s.geodesic_area(signed=True), signed, equal_nan=True) and np.array_equal(s.geodesic_perimeter(), per, equal_nan=True)


def test_device_forms_of_inverse_and_direct(gpk, fx):
    import torch

    e = fx["edge_xy"][:500]
    a, b = points(e[:, :2]), points(e[:, 2:])
    d, z1, z2 = (torch.empty(500, dtype=torch.float64, device="cuda") for _ in range(3))
    geodesic_inverse_device(a.device(), b.device(), d, z1, z2)
    only = torch.empty(500, dtype=torch.float64, device="cuda")
    geodesic_inverse_device(a.device(), b.device(), out_final_bearing=only)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), a.geodesic_distance(b)) and np.array_equal(z1.cpu().numpy(), a.geodesic_bearing(b))
    assert np.array_equal(z2.cpu().numpy(), a.geodesic_bearing(b, final=True)) and torch.equal(only, z2)
    xy, az = torch.empty((500, 2), dtype=torch.float64, device="cuda"), torch.empty(500, dtype=torch.float64, device="cuda")
    geodesic_destination_device(a.device(), z1, d, xy, az)
    torch.cuda.synchronize()
    assert np.array_equal(xy.cpu().numpy(), a.geodesic_destination(z1.cpu().numpy(), d.cpu().numpy()).array.xy)
    got = xy.cpu().numpy()
    ok = fx["edge_regime"][:500] == 0  # (the whole-ellipsoid pairs: no pole, no antipode)
    assert np.all(R.small_distance_m(got[ok, 0], got[ok, 1], e[ok, 2], e[ok, 3]) <= F * (R.DIRECT_ERR_M + R.AZIMUTH_ERR_M["whole"]) + R.karney_bound_m(fx["edge_s12"][:500][ok]))


def test_perimeter_is_the_geodesic_length_of_a_hole_free_column(gpk):
    from geopolars_amd import synth

    polys = synth.clustered_polygons(3000, seed=4, domain=60.0)
    assert polys.n_rings == len(polys)  # hole-free: every polygon is its exterior
    s = GeoSeries(polys)
    per, length = s.geodesic_perimeter(), s.geodesic_length("geodesic")
    edges = np.diff(polys.ring_offsets)[np.asarray(polys.geom_offsets[:-1])] - 1
    assert np.all(np.abs(per - length) <= 1e-9 * length + 2e-8 * edges) and per.min() > 0
    lines = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)], [(5.0, 5.0), (6.0, 6.0), (7.0, 5.0)]]))
    assert np.array_equal(lines.geodesic_area(), [0.0, 0.0]) and np.array_equal(lines.geodesic_perimeter(), [0.0, 0.0])
    assert np.array_equal(points([[1.0, 2.0]]).geodesic_area(signed=True), [0.0])
    bad = GeoSeries(GeoArrowArray.from_polygons([[[(0.0, 0.0), (1.0, 0.0), (1.0, 90.5), (0.0, 0.0)]], [[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 0.0)]]]))
    for got in (bad.geodesic_area(), bad.geodesic_area(signed=True), bad.geodesic_perimeter()):
        assert np.isnan(got[0]) and got[1] > 0  # a latitude outside [-90, 90]: NaN for that row alone
