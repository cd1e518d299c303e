"""GPU: polygon x polygon union and the grouped union (gpk_polygon_union, gpk_union_all_pairs, csrc/gpk_polyunion.hip) against the exact
rational reference (tests/polyunion_ref.py; tests/test_polyunion_ref.py pins it) and against the kernels the library already has.

Contract (include/geopolars_hip.h): offsets, validity, status and ring starts exactly; input coordinates bit for bit; a computed
crossing within 1e-9 * d of both carrying edges, d = the diagonal of the pair's joint box.

  1. every fixture row, both lane-group sizes, both placements; 2. the hand cases by name; 3. exact areas of the returned rings;
  4. the area identity against area and intersection_area on 20 000 random pairs, and the union of a column with itself; 5. row lists,
  an out-of-range index, DROP_EMPTY with out_src, refusals with real handles; 6. many blocks; 7. arc tables around the LDS slice;
  8. union_all."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import polygon_union_pairs, polygon_union_pairs_device
from tests import clip_abi
from tests import exact_ref as X
from tests import overlay_ref as O
from tests import polyclip_ref as L
from tests import polyunion_ref as U
from tests.test_gpu_lineclip import N_BALLAST, lanes_of, with_ballast
from tests.test_gpu_polyclip import _exact_ring_area2, _perimeter, _rows_of, comb, lattice_triangles

pytestmark = pytest.mark.gpu

PG, MPG = U.PG, U.MPG
FAMILY_IDS = [f"{U.NAMES[a]}-{U.NAMES[b]}" for a, b in U.FAMILIES]
MODE_IDS = [U.MODES[m] for m in U.MODES]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "geopolars_amd", "csrc")


@pytest.fixture(scope="module")
def golden():
    return np.load(U.GOLDEN)


def columns(golden, ka, kb, lanes, offset=(0.0, 0.0)):
    """the two fixture columns; for 16 lanes b carries ballast rows that no pair names (they lift its mean coordinate count past 32)"""
    ca, cb = U.load(golden, ka, kb, offset)
    both = cb if lanes == 4 else with_ballast(cb, N_BALLAST)
    assert lanes_of(both) == lanes, (both.n_coords, both.n_geoms)
    return ca, cb, GeoSeries(ca), GeoSeries(both)


def union_rows(a: GeoSeries, b: GeoSeries, mode, rows):
    call = {U.UNION: a.polygon_union}[mode]
    out, status = call(b, other_rows=rows, return_status=True)
    return out.array, status


def structure(col: GeoArrowArray, k):
    """(rings per part, coordinates per ring) of row k"""
    p0, p1 = col.geom_offsets[k], col.geom_offsets[k + 1]
    r0, r1 = col.part_offsets[p0], col.part_offsets[p1]
    return np.diff(col.part_offsets[p0:p1 + 1]).tolist(), np.diff(col.ring_offsets[r0:r1 + 1]).tolist()


# ---- 1. every fixture row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["lattice", "georeferenced"])
@pytest.mark.parametrize("lanes", [4, 16])
@pytest.mark.parametrize("mode", list(U.MODES), ids=MODE_IDS)
@pytest.mark.parametrize("ka,kb", U.FAMILIES, ids=FAMILY_IDS)
def test_every_fixture_row(golden, ka, kb, mode, lanes, placement):
    """offsets, validity, status and ring starts exactly, input coordinates bit for bit, crossings within the bound — through
    GeoSeries.polygon_union with a row map, and once more, byte for byte, through device buffers.  No row is unresolved."""
    offset = (0.0, 0.0) if placement == "lattice" else U.TRANSLATION
    ca, cb, a, b = columns(golden, ka, kb, lanes, offset)
    rows = np.arange(ca.n_geoms, dtype=np.uint32)
    got, status = union_rows(a, b, mode, rows)
    print("status counts:", np.bincount(status, minlength=5).tolist())
    worst = U.check_result(golden, ka, kb, mode, ca, cb, got, status, offset)
    assert (status != U.ST_UNRESOLVED).all()
    print(f"{FAMILY_IDS[U.FAMILIES.index((ka, kb))]} {U.MODES[mode]} G={lanes} {placement}: worst crossing distance / bound = {worst:.3e}")
    r = torch.from_numpy(rows.view(np.int32)).cuda()
    st = torch.full((len(rows),), 255, dtype=torch.uint8, device="cuda")
    dev = polygon_union_pairs_device(a.device(), b.device(), None, r, U.MODES[mode], out_status=st).array
    assert dev.xy.tobytes() == got.xy.tobytes() and (dev.ring_offsets == got.ring_offsets).all() and (dev.part_offsets == got.part_offsets).all()
    assert (dev.geom_offsets == got.geom_offsets).all() and (dev.is_valid() == got.is_valid()).all() and (st.cpu().numpy() == status).all()


# ---- 2. the hand cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [4, 16])
def test_hand_cases(lanes):
    """the smallest shapes that can go wrong, by name, with parts, rings, coordinates per ring and status stated by hand (they are rows
    of the fixture too)"""
    ka, kb = MPG, MPG
    A, B, av, bv, names = U.rows(ka, kb)
    want = U.hand_expectations(ka, kb)
    assert len(want) == len(U.HAND_CASES) == 20
    idx = list(want)
    ca, cb = X.column(ka, [A[i] for i in idx], [av[i] for i in idx]), X.column(kb, [B[i] for i in idx], [bv[i] for i in idx])
    if lanes == 16:
        cb = with_ballast(cb, N_BALLAST)
    assert lanes_of(cb) == lanes
    by_name = {names[i]: k for k, i in enumerate(idx)}
    for mode in U.MODES:
        got, status = union_rows(GeoSeries(ca), GeoSeries(cb), mode, np.arange(len(idx), dtype=np.uint32))
        assert got.is_valid().all()
        for k, i in enumerate(idx):
            w = want[i][mode]
            if w is not None:
                assert (*structure(got, k), int(status[k])) == w, (names[i], structure(got, k), status[k], w)
    got, status = union_rows(GeoSeries(ca), GeoSeries(cb), U.UNION, np.arange(len(idx), dtype=np.uint32))

    def ring(k, j=0):
        r0 = got.part_offsets[got.geom_offsets[k]] + j
        return got.xy[got.ring_offsets[r0]:got.ring_offsets[r0 + 1]].tolist()

    def same_cycle(got_ring, want_ring):
        """the same closed ring in the same direction, from whichever start (the fixture test pins the starts)"""
        g, w = got_ring[:-1], [list(map(float, v)) for v in want_ring[:-1]]
        return got_ring[0] == got_ring[-1] and len(g) == len(w) and any(g == w[s:] + w[:s] for s in range(len(w)))

    # equal polygons unite to a itself, a's own coordinates from a's own start
    assert ring(by_name["equal squares"]) == [list(map(float, v)) for v in U.S10]
    # the shared edge is gone and its two ends stay, collinear as they are
    assert same_cycle(ring(by_name["squares sharing a whole edge"]), [(0, 0), (10, 0), (20, 0), (20, 10), (10, 10), (0, 10), (0, 0)])
    assert same_cycle(ring(by_name["squares overlapping at a corner"]), [(0, 0), (10, 0), (10, 5), (15, 5), (15, 15), (5, 15), (5, 10), (0, 10), (0, 0)])
    # two touch points around a gap: two parts and no hole, b's vertices on a's edge become coordinates of a's ring
    k = by_name["touching at two points around a gap"]
    assert same_cycle(ring(k), [(0, 0), (10, 0), (10, 2), (10, 8), (10, 10), (0, 10), (0, 0)]) and same_cycle(ring(k, 1), U.NOTCHED)
    # the gap closed by overlap is a hole made of arcs of both rows: a clockwise ring through both crossings
    k = by_name["a C closed by a bar that overlaps both ends"]
    assert same_cycle(ring(k, 1), [(8, 3), (3, 3), (3, 7), (8, 7), (8, 3)])
    # ... closed by a point touch it fuses into the shell, which passes twice through (10, 7)
    k = by_name["a C closed by a wedge that overlaps one end and touches the other at a point"]
    assert (*structure(got, k), int(status[k])) == ([1], [12], U.ST_TOUCH) and ring(k)[:-1].count([10.0, 7.0]) == 2
    # the innermost shell: each annulus keeps its own hole
    k = by_name["annulus b inside the hole of annulus a: the innermost shell"]
    assert [sorted(ring(k, j))[0] for j in range(4)] == [[0, 0], [4, 4], [6, 6], [8, 8]]
    assert same_cycle(ring(by_name["b equal to a's hole"]), U.DONUT[0])


# ---- 3. exact areas of the returned rings ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(U.MODES), ids=MODE_IDS)
@pytest.mark.parametrize("ka,kb", U.FAMILIES, ids=FAMILY_IDS)
def test_exact_area_of_the_returned_rings(golden, ka, kb, mode):
    """For every OK row the exact (Fraction) area of the RETURNED rings differs from the exact result — area(a) + area(b) minus
    overlay_ref.exact_area, which shares no code with the union or its reference — by at most 1e-9 * d * (perimeter(a) + perimeter(b)):
    every moved vertex moves by at most 1e-9 * d (the fixture holds the correctly rounded exact crossing), and the output's perimeter is
    at most the operands' sum."""
    ca, cb, a, b = columns(golden, ka, kb, 4)
    A, B, _av, _bv, _names = U.rows(ka, kb)
    got, status = union_rows(a, b, mode, np.arange(ca.n_geoms, dtype=np.uint32))
    key = U.fixture_key(ka, kb) + U.MODES[mode] + "_"
    exact_xy, tag = golden[key + "xy"], golden[key + "tag"]
    assert len(exact_xy) == len(got.xy)
    d = L.pair_diagonals(ca, cb)
    sa, sb = np.append(L._row_starts(ca), len(ca.xy)), np.append(L._row_starts(cb), len(cb.xy))
    so = np.append(got.ring_offsets[got.part_offsets[got.geom_offsets[:-1]]], len(got.xy))
    worst_area, worst_move, n_ok = 0.0, 0.0, 0
    for i in range(ca.n_geoms):
        if status[i] not in (U.ST_OK, U.ST_TOUCH):
            continue
        n_ok += 1
        c0, c1 = so[i], so[i + 1]
        moved = np.hypot(*(got.xy[c0:c1] - exact_xy[c0:c1]).T)
        assert (moved[tag[c0:c1] == L.TAG_IN] == 0).all()
        worst_move = max(worst_move, float(moved.max()) / (U.REL_TOL * d[i]))
        r0, r1 = got.part_offsets[got.geom_offsets[i]], got.part_offsets[got.geom_offsets[i + 1]]
        area = sum((_exact_ring_area2(got.xy[got.ring_offsets[r]:got.ring_offsets[r + 1]]) for r in range(r0, r1)), Fraction(0)) / 2
        want = U.row_area(ka, A[i]) + U.row_area(kb, B[i]) - O.exact_area(ka, A[i], kb, B[i])
        pa, pb = _perimeter(ca, i, sa), _perimeter(cb, i, sb)
        worst_area = max(worst_area, float(abs(area - want)) / (U.REL_TOL * d[i] * (pa + pb)))
        assert _perimeter(got, i, so) <= (pa + pb) * (1 + 1e-12)
    print(f"{FAMILY_IDS[U.FAMILIES.index((ka, kb))]} {U.MODES[mode]}: {n_ok} rows, worst |area - exact| / bound = {worst_area:.3e}, worst move / bound = {worst_move:.3e}")
    assert n_ok > 50 and worst_area <= 1.0 and worst_move <= 1.0


# ---- 4. random pairs -------------------------------------------------------------------------------------------------------------------
def test_area_identity_on_random_pairs_and_the_union_with_itself():
    """20 000 lattice triangle pairs (coincident vertices, vertices on edges and shared edge pieces are frequent): area(a ∪ b) is
    area(a) + area(b) - intersection_area within that kernel's documented 1e-9 * (d_a^2 + d_b^2) plus the union's own 1e-9 * d *
    perimeter (the bound of test_gpu_polyclip.test_cross_checks_on_random_pairs); no row is unresolved, null or empty.  The union of
    the column with itself returns every row's own coordinates: the ring as stored when it is counter-clockwise, reversed when not."""
    rng = np.random.default_rng(41)
    n, size = 20000, 16
    assert 1.0 / (2 * size * size) ** 2 > 1e-6  # the gap, by construction
    ta, tb = lattice_triangles(n, rng, size), lattice_triangles(n, rng, size)
    a, b = GeoSeries(X.column(PG, ta)), GeoSeries(X.column(PG, tb))
    uni, st = a.polygon_union(b, return_status=True)
    print("status counts, union:", np.bincount(st, minlength=5).tolist())
    assert np.isin(st, (U.ST_OK, U.ST_TOUCH)).all() and uni.array.is_valid().all()
    area_a, area_b, shared, au = a.area(), b.area(), a.intersection_area(b), uni.area()
    d2 = 2.0 * size * size
    tol_measure, tol_clip = 2e-9 * d2, 6e-9 * d2
    worst = float(np.abs(au - (area_a + area_b - shared)).max())
    print(f"worst |area(union) - (area(a) + area(b) - intersection_area)| = {worst:.3e} (bound {tol_measure + tol_clip:.3e})")
    assert (np.abs(au - (area_a + area_b - shared)) <= tol_measure + tol_clip).all()
    same, st = a.polygon_union(a, return_status=True)
    s = same.array
    assert (st == U.ST_OK).all() and (np.diff(s.geom_offsets) == 1).all() and (np.diff(s.part_offsets) == 1).all() and (np.diff(s.ring_offsets) == 4).all()
    src = a.array.xy.reshape(n, 4, 2)
    ccw = np.array([L._shoelace2(t[0]) > 0 for t in ta])
    want = np.where(ccw[:, None, None], src, src[:, ::-1])
    assert s.xy.tobytes() == np.ascontiguousarray(want).tobytes()


# ---- 5. row lists --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(U.MODES), ids=MODE_IDS)
def test_row_lists_and_drop_empty(golden, mode):
    """permuted row lists give the rows of the identity call; an index past the end of either column gives a null row of status 3; with
    DROP_EMPTY the column is the undropped one with its null rows removed, byte for byte, and out_src names them"""
    ka, kb = MPG, MPG
    ca, cb = U.load(golden, ka, kb)
    a, b = GeoSeries(ca), GeoSeries(cb)
    base = union_rows(a, b, mode, None)[0]
    n = ca.n_geoms
    perm = np.random.default_rng(3).permutation(n).astype(np.uint32)
    got = polygon_union_pairs(a, b, perm, perm, U.MODES[mode]).array
    assert _rows_of(got, range(n)) == _rows_of(base, perm)
    li, ri = np.concatenate([perm, [n, 0, 2**32 - 1]]).astype(np.uint32), np.concatenate([perm, [0, cb.n_geoms, 1]]).astype(np.uint32)
    got, status = polygon_union_pairs(a, b, li, ri, U.MODES[mode], return_status=True)
    got = got.array
    assert _rows_of(got, range(n)) == _rows_of(base, perm)
    assert not got.is_valid()[n:].any() and (np.diff(got.geom_offsets)[n:] == 0).all() and (status[n:] == U.ST_NULL).all()
    dropped, src, status2 = polygon_union_pairs(a, b, li, ri, U.MODES[mode], drop_empty=True, return_status=True)
    keep = np.nonzero(got.is_valid() & (np.diff(got.geom_offsets) > 0))[0]
    assert 0 < len(keep) < n and (src == keep).all() and src.dtype == np.int32 and (status2 == status).all()
    d = dropped.array
    assert d.is_valid().all() and _rows_of(d, range(len(keep))) == _rows_of(got, keep)
    assert d.xy.tobytes() == got.xy.tobytes() and (d.ring_offsets == got.ring_offsets).all() and (d.part_offsets == got.part_offsets).all()
    src_dev = torch.full((len(li),), -1, dtype=torch.int32, device="cuda")
    dd = polygon_union_pairs_device(a.device(), b.device(), torch.from_numpy(li.view(np.int32)).cuda(), torch.from_numpy(ri.view(np.int32)).cuda(),
                                    U.MODES[mode], drop_empty=True, out_src=src_dev)
    torch.cuda.synchronize()
    assert (src_dev.cpu().numpy()[: len(dd)] == keep).all() and dd.array.xy.tobytes() == d.xy.tobytes()
    assert (dd.array.geom_offsets == d.geom_offsets).all()


def test_refusals_with_real_handles(golden):
    """the mode, family and count refusals of the library itself, in gpk_polygon_clip's order, and an empty side, which gives null"""
    ca, cb = U.load(golden, PG, PG)
    a, b = GeoSeries(ca), GeoSeries(cb)
    lines = GeoSeries(X.column(L.R.LS, [[(0, 0), (1, 1)]] * len(a)))
    lib, out = _abi.lib(), C.c_void_p()
    call = lambda x, y, n, mode=0, flags=0: lib.gpk_polygon_union(x.device().handle, y.device().handle, None, None, n, _abi.MEM_HOST, mode, flags, None,  # noqa: E731
                                                                 _abi.MEM_HOST, None, _abi.MEM_HOST, None, C.byref(out))
    assert call(lines, b, len(a)) == _abi.GPK_ERR_MISMATCHED_GEOMETRY and call(a, lines, len(a)) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    assert call(lines, b, len(a), mode=2) == _abi.GPK_ERR_INVALID_ARGUMENT and call(lines, b, len(a), flags=2) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert call(a, b, len(a) - 1) == _abi.GPK_ERR_INVALID_ARGUMENT and not out.value
    got, status = GeoSeries(X.column(PG, [[U.S10], []])).polygon_union(GeoSeries(X.column(PG, [[], [U.S10]])), return_status=True)
    assert not got.array.is_valid().any() and (status == U.ST_NULL).all()  # an empty row is not the neutral element


def test_zero_pairs_through_the_abi():
    """n_rows = 0 with host and with device row lists, with and without DROP_EMPTY (the Python layer never makes this call); the union
    of disjoint shapes is never empty, so there is no "every pair dropped" here"""
    clip_abi.check_zero_pairs("gpk_polygon_union", _abi.PUNION_UNION)


# ---- 6. many blocks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes,n_pairs", [(4, 4099), (16, 4099), (4, 70001)])
def test_many_blocks(golden, lanes, n_pairs):
    """The fixture rows tiled to 4 099 and to 70 001 pairs (no multiple of 256 / G): ragged last blocks, offsets far past one scan
    tile, null rows in between.  Every tile's rows must be the base rows, byte for byte."""
    ka, kb = MPG, MPG
    ca, cb, a, b = columns(golden, ka, kb, lanes)
    n = ca.n_geoms
    for mode in U.MODES:
        base = union_rows(a, b, mode, np.arange(n, dtype=np.uint32))[0]
        idx = (np.arange(n_pairs) % n).astype(np.uint32)
        got, status = polygon_union_pairs(a, b, idx, idx, U.MODES[mode], return_status=True)
        got = got.array
        full, rem = divmod(n_pairs, n)
        tile = lambda off, upto: np.concatenate([np.tile(np.diff(off), full), np.diff(off)[:upto]])  # noqa: E731
        bg, bp, br = base.geom_offsets, base.part_offsets, base.ring_offsets
        assert (np.diff(got.geom_offsets) == tile(bg, rem)).all() and got.geom_offsets[0] == 0
        assert (np.diff(got.part_offsets) == tile(bp, bg[rem])).all() and (np.diff(got.ring_offsets) == tile(br, bp[bg[rem]])).all()
        xy = np.concatenate([np.tile(base.xy, (full, 1)), base.xy[: br[bp[bg[rem]]]]])
        assert got.xy.tobytes() == xy.tobytes()
        assert (got.is_valid() == np.concatenate([np.tile(base.is_valid(), full), base.is_valid()[:rem]])).all()
        assert (status[:n] == golden[U.fixture_key(ka, kb) + U.MODES[mode] + "_status"]).all() and (status[n:2 * n] == status[:n]).all()


# ---- 7. arc tables around the LDS slice ---------------------------------------------------------------------------------------------------
def _lds_arcs_per_lane():
    m = re.search(r"constexpr int STITCH_LDS_ARCS_PER_LANE = (\d+);", open(os.path.join(CSRC, "gpk_polyclip_run.h")).read())
    return int(m.group(1))


# a bar across a comb of T teeth: the union keeps 2 T arcs of the comb (T tooth tops, T - 1 gap bottoms, the base) and 2 T of the bar
UNION_ARCS_PER_TOOTH = 4


@pytest.mark.parametrize("lanes", [4, 16])
def test_arc_tables_around_the_lds_slice(lanes):
    """The stitch reads a pair's arcs from its LDS slice up to STITCH_LDS_ARCS_PER_LANE arcs a lane and from global scratch beyond.  The
    union of a comb of T teeth with a bar has 4 T arcs: the largest comb that fits the slice and the smallest that does not, computed
    from the slice size in the header, and the tooth counts of test_gpu_polyclip ({4, 5} at 4 lanes, {16, 17} at 16), against the
    reference: one shell and the T - 1 holes the bar closes off between the teeth."""
    slice_arcs = _lds_arcs_per_lane() * lanes
    fits = slice_arcs // UNION_ARCS_PER_TOOTH
    assert fits >= 2
    for teeth in (fits, fits + 1, lanes, lanes + 1):
        a_row, b_row = [comb(teeth)], [U.sq(-1, 6, 4 * teeth + 1, 8)]
        cb = X.column(PG, [b_row])
        if lanes == 16:
            cb = with_ballast(cb, N_BALLAST)
        assert lanes_of(cb) == lanes
        a, b = GeoSeries(X.column(PG, [a_row])), GeoSeries(cb)
        ra, rb = L.row_rings(PG, a_row), L.row_rings(PG, b_row)
        n_arcs = len(U._walk_arcs(ra, rb, U.WALK_A, U.UNION, [])) + len(U._walk_arcs(rb, ra, U.WALK_B, U.UNION, []))
        assert n_arcs == UNION_ARCS_PER_TOOTH * teeth and (n_arcs <= slice_arcs) == (teeth <= fits)
        parts, st, _gap = U.union(PG, a_row, PG, b_row, U.UNION)
        got, status = union_rows(a, b, U.UNION, np.zeros(1, dtype=np.uint32))
        assert status[0] == st == U.ST_OK and [len(p) for p in parts] == [teeth]
        want = np.array([(float(x), float(y)) for p in parts for r in p for x, y in r])
        assert got.xy.tobytes() == want.tobytes() and np.diff(got.ring_offsets).tolist() == [len(r) for p in parts for r in p]
        assert np.diff(got.part_offsets).tolist() == [len(p) for p in parts]


# ---- 8. union_all ------------------------------------------------------------------------------------------------------------------------
def _unit_squares(cells):
    return [[U.sq(x, y, x + 1, y + 1)] for x, y in cells]


def _ring_areas2(col, k):
    p0, p1 = col.geom_offsets[k], col.geom_offsets[k + 1]
    return [[_exact_ring_area2(col.xy[col.ring_offsets[r]:col.ring_offsets[r + 1]]) for r in range(col.part_offsets[p], col.part_offsets[p + 1])]
            for p in range(p0, p1)]


def _row_area(col, k):
    return sum((a for part in _ring_areas2(col, k) for a in part), Fraction(0)) / 2


def test_union_all_of_a_grid_of_unit_squares():
    """8 x 8 unit squares: one group gives one ring of area exactly 64 whose coordinates are all input coordinates; grouped by column,
    eight 1 x 8 strips; a checkerboard gives 32 parts; 3 x 3 without its centre one part with one hole"""
    cells = [(x, y) for x in range(8) for y in range(8)]
    s = GeoSeries(X.column(PG, _unit_squares(cells)))
    out, status = s.union_all(return_status=True)
    o = out.array
    assert len(out) == 1 and list(status) == [U.ST_OK] and o.geom_type == _abi.GEOM_MULTIPOLYGON and o.validity is None
    assert structure(o, 0)[0] == [1] and _row_area(o, 0) == 64
    assert {tuple(v) for v in o.xy.tolist()} <= {(float(x), float(y)) for x in range(9) for y in range(9)}
    out, status = s.union_all(by=np.array([x for x, _y in cells]) * 10 - 30, return_status=True)
    o = out.array
    assert len(out) == 8 and (status == U.ST_OK).all()
    for k in range(8):
        assert structure(o, k)[0] == [1] and _row_area(o, k) == 8
        r = o.xy[o.ring_offsets[o.part_offsets[o.geom_offsets[k]]]:o.ring_offsets[o.part_offsets[o.geom_offsets[k]] + 1]]
        assert r[:, 0].min() == k and r[:, 0].max() == k + 1 and r[:, 1].min() == 0 and r[:, 1].max() == 8
    board = GeoSeries(X.column(PG, _unit_squares([c for c in cells if (c[0] + c[1]) % 2 == 0])))
    out, status = board.union_all(return_status=True)
    assert list(status) == [U.ST_OK] and structure(out.array, 0) == ([1] * 32, [5] * 32)
    frame = GeoSeries(X.column(PG, _unit_squares([(x, y) for x in range(3) for y in range(3) if (x, y) != (1, 1)])))
    out, status = frame.union_all(return_status=True)
    assert list(status) == [U.ST_OK] and structure(out.array, 0)[0] == [2] and _ring_areas2(out.array, 0) == [[18, -2]]


def test_union_all_group_sizes_and_dropped_rows():
    """groups of 1, 2, 3 and 5 rows cover the odd pass-through in every round; null and empty rows are dropped first, and a group of
    only such rows gives an empty row, not null; a multipolygon column works the same"""
    sizes = {3: 1, 5: 2, 8: 3, 13: 5}
    rows, by, valid = [], [], []
    for g, n in sizes.items():
        for k in range(n):
            rows.append([U.sq(2 * k, 10 * g, 2 * k + 3, 10 * g + 1)])  # a chain of 3 x 1 bars, each overlapping the next
            by.append(g)
            valid.append(1)
    rows += [[U.sq(0, 0, 1, 1)], [], [], [U.sq(50, 50, 51, 51)]]
    by += [21, 21, 13, 5]
    valid += [0, 1, 1, 0]
    order = np.random.default_rng(5).permutation(len(rows))
    rows, by, valid = [rows[i] for i in order], np.array(by)[order], [valid[i] for i in order]
    for kind in (PG, MPG):
        col = X.column(kind, rows if kind == PG else [([[]] + [r] if r else []) for r in rows], valid)
        out, status = GeoSeries(col).union_all(by=by, return_status=True)
        o = out.array
        assert len(out) == 5 and status.tolist() == [U.ST_OK] * 4 + [U.ST_EMPTY] and o.is_valid().all()
        for k, (g, n) in enumerate(sizes.items()):
            assert structure(o, k)[0] == [1] and _row_area(o, k) == 2 * n + 1, (g, n)
        assert structure(o, 4) == ([], [])
    one = GeoSeries(X.column(PG, [[U.sq(0, 0, 4, 4, cw=True)]])).union_all()
    assert one.array.xy.tolist() == [list(map(float, v)) for v in U.sq(0, 0, 4, 4)]  # normalised: counter-clockwise from the first coordinate


def test_union_all_of_random_rectangles_against_the_integer_grid():
    """200 random axis-parallel integer rectangles in 7 groups: the exact area of every result is the number of unit cells the group
    covers, counted on the integer grid; a shuffle within the groups changes neither the area nor the part count"""
    rng = np.random.default_rng(77)
    n, size = 200, 40
    x0, y0 = rng.integers(0, size - 8, n), rng.integers(0, size - 8, n)
    w, h = rng.integers(1, 9, n), rng.integers(1, 9, n)
    by = rng.integers(0, 7, n)
    rows = [[U.sq(int(x0[i]), int(y0[i]), int(x0[i] + w[i]), int(y0[i] + h[i]))] for i in range(n)]
    out, status = GeoSeries(X.column(PG, rows)).union_all(by=by, return_status=True)
    o = out.array
    print("status:", status.tolist(), "parts:", np.diff(o.geom_offsets).tolist())
    assert len(out) == 7 and np.isin(status, (U.ST_OK, U.ST_TOUCH)).all() and o.is_valid().all()
    for g in range(7):
        grid = np.zeros((size, size), dtype=bool)
        for i in np.nonzero(by == g)[0]:
            grid[x0[i]:x0[i] + w[i], y0[i]:y0[i] + h[i]] = True
        assert _row_area(o, g) == int(grid.sum()), g
    assert {tuple(v) for v in o.xy.tolist()} <= {(float(x), float(y)) for x in range(size + 1) for y in range(size + 1)}
    perm = rng.permutation(n)
    out2 = GeoSeries(X.column(PG, [rows[i] for i in perm])).union_all(by=by[perm]).array
    assert [_row_area(out2, g) for g in range(7)] == [_row_area(o, g) for g in range(7)]
    assert np.diff(out2.geom_offsets).tolist() == np.diff(o.geom_offsets).tolist()


def test_the_pairing_kernel_against_its_host_statement():
    """gpk_union_all_pairs on sorted group ids with runs of every small length, over more than one block and more than one scan tile:
    pairs, pass-through rows and the next round's rows as the loop in Python states them"""
    rng = np.random.default_rng(9)
    runs = np.concatenate([[1, 2, 3, 4, 5, 7, 8], rng.integers(1, 12, 1500)])
    group = np.repeat(np.arange(len(runs)) * 3, runs).astype(np.int32)
    n, base = len(group), 100000
    rows = rng.permutation(base)[:n].astype(np.uint32)
    want_a, want_b, want_g, want_r = [], [], [], []
    i = 0
    while i < n:
        if i + 1 < n and group[i + 1] == group[i]:
            want_r.append(base + len(want_a)), want_a.append(rows[i]), want_b.append(rows[i + 1]), want_g.append(group[i])
            i += 2
        else:
            want_r.append(rows[i]), want_g.append(group[i])
            i += 1
    dev = lambda x: torch.from_numpy(x.view(np.int32)).cuda()  # noqa: E731
    g, r = dev(group), dev(rows)
    a_rows, b_rows = (torch.full((n // 2,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    ng, nr = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    counts = (C.c_int64 * 2)()
    assert n > 4096
    _abi.check(_abi.lib().gpk_union_all_pairs(g.data_ptr(), r.data_ptr(), n, base, a_rows.data_ptr(), b_rows.data_ptr(), ng.data_ptr(), nr.data_ptr(), counts, None))
    assert list(counts) == [len(want_a), len(want_g)]
    assert a_rows.cpu().numpy()[: len(want_a)].tolist() == want_a and b_rows.cpu().numpy()[: len(want_a)].tolist() == want_b
    assert ng.cpu().numpy()[: len(want_g)].tolist() == want_g and nr.cpu().numpy()[: len(want_g)].tolist() == want_r
    assert (ng.cpu().numpy()[len(want_g):] == -1).all() and (a_rows.cpu().numpy()[len(want_a):] == -1).all()
