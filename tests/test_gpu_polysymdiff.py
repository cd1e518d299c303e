"""GPU: polygon x polygon symmetric difference (gpk_polygon_symdiff, csrc/gpk_polysymdiff.hip) against the exact rational reference
(tests/polysymdiff_ref.py; tests/test_polysymdiff_ref.py pins it) and against the kernels the library already has.

Contract (include/geopolars_hip.h): offsets, validity, status and ring starts exactly; input coordinates bit for bit; a computed
crossing within 1e-9 * d of both carrying edges, d = the diagonal of the pair's joint box.

  1. every fixture row, both lane-group sizes, both placements; 2. the hand cases by name; 3. exact areas of the returned rings;
  4. the area identity against area and intersection_area on 20 000 random pairs, is_valid, a column against itself, and 2 000 pairs
  against the three-call route; 5. row lists, an out-of-range index, DROP_EMPTY with out_src, refusals with real handles, zero pairs;
  6. many blocks; 7. arc tables around the LDS slice; 8. the rows on which the orientation filter fails on a non-zero sign."""
import ctypes as C
import os
import re
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest
import torch

from geopolars_amd import _abi
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import polygon_symdiff_pairs, polygon_symdiff_pairs_device
from tests import clip_abi
from tests import exact_ref as X
from tests import hard_clip as K
from tests import hard_orient as H
from tests import overlay_ref as O
from tests import polyclip_ref as L
from tests import polysymdiff_ref as S
from tests.test_gpu_lineclip import N_BALLAST, lanes_of, with_ballast
from tests.test_gpu_polyclip import _exact_ring_area2, _perimeter, _rows_of, lattice_triangles
from tests.test_gpu_polyunion import structure

pytestmark = pytest.mark.gpu

PG, MPG = S.PG, S.MPG
FAMILY_IDS = [f"{S.NAMES[a]}-{S.NAMES[b]}" for a, b in S.FAMILIES]
HOW = S.MODES[S.SYMDIFF]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "geopolars_amd", "csrc")


@pytest.fixture(scope="module")
def golden():
    return np.load(S.GOLDEN)


def columns(golden, ka, kb, lanes, offset=(0.0, 0.0)):
    """the two fixture columns; for 16 lanes b carries ballast rows that no pair names (they lift its mean coordinate count past 32)"""
    ca, cb = S.load(golden, ka, kb, offset)
    both = cb if lanes == 4 else with_ballast(cb, N_BALLAST)
    assert lanes_of(both) == lanes, (both.n_coords, both.n_geoms)
    return ca, cb, GeoSeries(ca), GeoSeries(both)


def symdiff_rows(a: GeoSeries, b: GeoSeries, rows):
    out, status = a.polygon_symmetric_difference(b, other_rows=rows, return_status=True)
    return out.array, status


def second_column(col, lanes):
    if lanes == 16 and lanes_of(col) != 16:
        col = with_ballast(col, N_BALLAST)
    assert lanes_of(col) == lanes, (col.n_coords, col.n_geoms)
    return col


# ---- 1. every fixture row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["lattice", "georeferenced"])
@pytest.mark.parametrize("lanes", [4, 16])
@pytest.mark.parametrize("ka,kb", S.FAMILIES, ids=FAMILY_IDS)
def test_every_fixture_row(golden, ka, kb, lanes, placement):
    """offsets, validity, status and ring starts exactly, input coordinates bit for bit, crossings within the bound — through
    GeoSeries.polygon_symmetric_difference with a row map, and once more, byte for byte, through device buffers.  No row is
    unresolved."""
    offset = (0.0, 0.0) if placement == "lattice" else S.TRANSLATION
    ca, cb, a, b = columns(golden, ka, kb, lanes, offset)
    rows = np.arange(ca.n_geoms, dtype=np.uint32)
    got, status = symdiff_rows(a, b, rows)
    print("status counts:", np.bincount(status, minlength=5).tolist())
    worst = S.check_result(golden, ka, kb, S.SYMDIFF, ca, cb, got, status, offset)
    assert (status != S.ST_UNRESOLVED).all()
    print(f"{FAMILY_IDS[S.FAMILIES.index((ka, kb))]} G={lanes} {placement}: worst crossing distance / bound = {worst:.3e}")
    r = torch.from_numpy(rows.view(np.int32)).cuda()
    st = torch.full((len(rows),), 255, dtype=torch.uint8, device="cuda")
    dev = polygon_symdiff_pairs_device(a.device(), b.device(), None, r, out_status=st).array
    assert dev.xy.tobytes() == got.xy.tobytes() and (dev.ring_offsets == got.ring_offsets).all() and (dev.part_offsets == got.part_offsets).all()
    assert (dev.geom_offsets == got.geom_offsets).all() and (dev.is_valid() == got.is_valid()).all() and (st.cpu().numpy() == status).all()


# ---- 2. the hand cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [4, 16])
def test_hand_cases(lanes):
    """the smallest shapes that can go wrong, by name, with parts, rings, coordinates per ring and status stated by hand (they are rows
    of the fixture too)"""
    ka, kb = MPG, MPG
    A, B, av, bv, names = S.rows(ka, kb)
    want = S.hand_expectations(ka, kb)
    assert len(want) == len(S.HAND_CASES) == 17
    idx = list(want)
    ca = X.column(ka, [A[i] for i in idx], [av[i] for i in idx])
    cb = second_column(X.column(kb, [B[i] for i in idx], [bv[i] for i in idx]), lanes)
    got, status = symdiff_rows(GeoSeries(ca), GeoSeries(cb), np.arange(len(idx), dtype=np.uint32))
    assert got.is_valid().all()
    for k, i in enumerate(idx):
        assert (*structure(got, k), int(status[k])) == want[i], (names[i], structure(got, k), status[k], want[i])

    def ring(k, j=0):
        r0 = got.part_offsets[got.geom_offsets[k]] + j
        return got.xy[got.ring_offsets[r0]:got.ring_offsets[r0 + 1]].tolist()

    def same_cycle(got_ring, want_ring):
        g, w = got_ring[:-1], [list(map(float, v)) for v in want_ring[:-1]]
        return got_ring[0] == got_ring[-1] and len(g) == len(w) and any(g == w[s:] + w[:s] for s in range(len(w)))

    row = lambda name: S.hand_row(ka, kb, name)  # noqa: E731
    # the parts touch at the two crossings and stay separate rings, each with the crossing's one value
    k = row("squares overlapping at a corner")
    for want_ring in ([(0, 0), (10, 0), (10, 5), (5, 5), (5, 10), (0, 10), (0, 0)], [(10, 5), (15, 5), (15, 15), (5, 15), (5, 10), (10, 10), (10, 5)]):
        assert sum(same_cycle(ring(k, j), want_ring) for j in range(2)) == 1
    # the shared edge is gone and its two ends stay
    assert same_cycle(ring(row("edge neighbours")), [(0, 0), (10, 0), (20, 0), (20, 10), (10, 10), (0, 10), (0, 0)])
    # b as a hole: clockwise, b's own coordinates
    k = row("b inside a: a hole")
    assert ring(k, 0) == [list(map(float, v)) for v in S.S10] and same_cycle(ring(k, 1), [(2, 2), (2, 5), (5, 5), (5, 2), (2, 2)])
    # the hole of b is a shell inside the hole b leaves in a: its own part
    k = row("annulus b inside a")
    assert [sorted(ring(k, j))[0] for j in range(3)] == [[0, 0], [6, 6], [8, 8]] and structure(got, k)[0] == [2, 1]
    # one ring twice through (5, 0)
    k = row("b touching a from inside at a vertex")
    assert ring(k)[:-1].count([5.0, 0.0]) == 2
    # a ring whose first piece is kept backwards: both rings start at the crossing (10, 5), where a's first segment leaves b
    k = row("a ring whose first piece is kept backwards")
    assert ring(k, 0)[0] == [10.0, 5.0] and ring(k, 1)[0] == [10.0, 5.0]
    assert sum(same_cycle(ring(k, j), [(0, 0), (10, 0), (10, 5), (5, 5), (5, 10), (0, 10), (0, 0)]) for j in range(2)) == 1


# ---- 3. exact areas of the returned rings ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ka,kb", S.FAMILIES, ids=FAMILY_IDS)
def test_exact_area_of_the_returned_rings(golden, ka, kb):
    """For every OK row the exact (Fraction) area of the RETURNED rings differs from the exact result — area(a) + area(b) minus twice
    overlay_ref.exact_area, which shares no code with the kernel or its reference — by at most 1e-9 * d * (perimeter(a) +
    perimeter(b)), the clip's own bound: every moved vertex moves by at most 1e-9 * d (the fixture holds the correctly rounded exact
    crossing), and the output's perimeter is at most the operands' sum."""
    ca, cb, a, b = columns(golden, ka, kb, 4)
    A, B, _av, _bv, _names = S.rows(ka, kb)
    got, status = symdiff_rows(a, b, np.arange(ca.n_geoms, dtype=np.uint32))
    key = S.fixture_key(ka, kb) + HOW + "_"
    exact_xy, tag = golden[key + "xy"], golden[key + "tag"]
    assert len(exact_xy) == len(got.xy)
    d = L.pair_diagonals(ca, cb)
    sa, sb = np.append(L._row_starts(ca), len(ca.xy)), np.append(L._row_starts(cb), len(cb.xy))
    so = np.append(got.ring_offsets[got.part_offsets[got.geom_offsets[:-1]]], len(got.xy))
    worst_area, worst_move, n_ok = 0.0, 0.0, 0
    for i in range(ca.n_geoms):
        if status[i] not in (S.ST_OK, S.ST_TOUCH):
            continue
        n_ok += 1
        c0, c1 = so[i], so[i + 1]
        moved = np.hypot(*(got.xy[c0:c1] - exact_xy[c0:c1]).T)
        assert (moved[tag[c0:c1] == L.TAG_IN] == 0).all()
        worst_move = max(worst_move, float(moved.max()) / (S.REL_TOL * d[i]))
        r0, r1 = got.part_offsets[got.geom_offsets[i]], got.part_offsets[got.geom_offsets[i + 1]]
        area = sum((_exact_ring_area2(got.xy[got.ring_offsets[r]:got.ring_offsets[r + 1]]) for r in range(r0, r1)), Fraction(0)) / 2
        want = S.row_area(ka, A[i]) + S.row_area(kb, B[i]) - 2 * O.exact_area(ka, A[i], kb, B[i])
        pa, pb = _perimeter(ca, i, sa), _perimeter(cb, i, sb)
        worst_area = max(worst_area, float(abs(area - want)) / (S.REL_TOL * d[i] * (pa + pb)))
        assert _perimeter(got, i, so) <= (pa + pb) * (1 + 1e-12)
    print(f"{FAMILY_IDS[S.FAMILIES.index((ka, kb))]}: {n_ok} rows, worst |area - exact| / bound = {worst_area:.3e}, worst move / bound = {worst_move:.3e}")
    assert n_ok > 50 and worst_area <= 1.0 and worst_move <= 1.0


# ---- 4. random pairs -------------------------------------------------------------------------------------------------------------------
def _row_areas(col):
    """the exact area of every row of a MULTIPOLYGON column (Fractions of the returned doubles)"""
    g, p, r = col.geom_offsets, col.part_offsets, col.ring_offsets
    return [sum((_exact_ring_area2(col.xy[r[k]:r[k + 1]]) for k in range(p[g[i]], p[g[i + 1]])), Fraction(0)) / 2 for i in range(col.n_geoms)]


def test_area_identity_validity_self_and_the_three_call_route():
    """20 000 lattice triangle pairs (coincident vertices, vertices on edges and shared edge pieces are frequent): the area of the
    result is area(a) + area(b) - 2 intersection_area within twice that kernel's documented 1e-9 * (d_a^2 + d_b^2) plus the clip's own
    1e-9 * d * perimeter (the bounds of test_gpu_polyclip.test_cross_checks_on_random_pairs); every row of status 0 is_valid; no row
    is unresolved; the column against itself is all empty.  2 000 of the pairs through difference, difference, union: the same exact
    ring area — a crossing has the value along the edge of the call's first operand, so b \\ a moves its crossings by the bound, which
    the area tolerance 1e-9 * d * perimeter covers."""
    rng = np.random.default_rng(43)
    n, size = 20000, 16
    assert 1.0 / (2 * size * size) ** 2 > 1e-6  # the gap, by construction
    ta, tb = lattice_triangles(n, rng, size), lattice_triangles(n, rng, size)
    a, b = GeoSeries(X.column(PG, ta)), GeoSeries(X.column(PG, tb))
    sym, st = a.polygon_symmetric_difference(b, return_status=True)
    print("status counts:", np.bincount(st, minlength=5).tolist())
    assert (st != S.ST_UNRESOLVED).all() and (st != S.ST_NULL).all() and sym.array.is_valid().all()
    area_a, area_b, shared, got = a.area(), b.area(), a.intersection_area(b), sym.area()
    d2 = 2.0 * size * size
    tol_measure, tol_clip = 2 * 2e-9 * d2, 6e-9 * d2
    worst = float(np.abs(got - (area_a + area_b - 2 * shared)).max())
    print(f"worst |area(result) - (area(a) + area(b) - 2 intersection_area)| = {worst:.3e} (bound {tol_measure + tol_clip:.3e})")
    assert worst <= tol_measure + tol_clip
    ok = st == S.ST_OK
    valid = sym.is_valid()
    assert ok.sum() > n // 2 and np.asarray(valid)[ok].all()
    same, st2 = a.polygon_symmetric_difference(a, return_status=True)
    assert (st2 == S.ST_EMPTY).all() and same.array.is_valid().all() and (np.diff(same.array.geom_offsets) == 0).all() and len(same.array.xy) == 0
    m = 2000
    a2, b2 = GeoSeries(X.column(PG, ta[:m])), GeoSeries(X.column(PG, tb[:m]))
    one, st_one = a2.polygon_symmetric_difference(b2, return_status=True)
    d_ab, d_ba = a2.polygon_difference(b2), b2.polygon_difference(a2)
    three, st3 = d_ab.polygon_union(d_ba, return_status=True)
    # (the union makes an empty side a null row: there the result is the other difference)
    areas_one, areas_ab, areas_ba, areas_three = _row_areas(one.array), _row_areas(d_ab.array), _row_areas(d_ba.array), _row_areas(three.array)
    worst = 0.0
    for i in range(m):
        route = areas_three[i] if st3[i] in (S.ST_OK, S.ST_TOUCH) else areas_ab[i] + areas_ba[i]
        per = sum(float(np.hypot(*np.diff(np.array(t[0], dtype=np.float64), axis=0).T).sum()) for t in (ta[i], tb[i]))
        bound = 1e-9 * np.sqrt(d2) * per
        worst = max(worst, float(abs(areas_one[i] - route)) / bound)
    print(f"three-call route: worst |exact ring area difference| / (1e-9 d perimeter) = {worst:.3e}")
    assert worst <= 1.0


# ---- 5. row lists --------------------------------------------------------------------------------------------------------------------
def test_row_lists_and_drop_empty(golden):
    """permuted row lists give the rows of the identity call; an index past the end of either column gives a null row of status 3; with
    DROP_EMPTY the column is the undropped one with its empty and null rows removed, byte for byte, and out_src names them"""
    ka, kb = MPG, MPG
    ca, cb = S.load(golden, ka, kb)
    a, b = GeoSeries(ca), GeoSeries(cb)
    base = symdiff_rows(a, b, None)[0]
    n = ca.n_geoms
    perm = np.random.default_rng(3).permutation(n).astype(np.uint32)
    got = polygon_symdiff_pairs(a, b, perm, perm).array
    assert _rows_of(got, range(n)) == _rows_of(base, perm)
    li, ri = np.concatenate([perm, [n, 0, 2**32 - 1]]).astype(np.uint32), np.concatenate([perm, [0, cb.n_geoms, 1]]).astype(np.uint32)
    got, status = polygon_symdiff_pairs(a, b, li, ri, return_status=True)
    got = got.array
    assert _rows_of(got, range(n)) == _rows_of(base, perm)
    assert not got.is_valid()[n:].any() and (np.diff(got.geom_offsets)[n:] == 0).all() and (status[n:] == S.ST_NULL).all()
    dropped, src, status2 = polygon_symdiff_pairs(a, b, li, ri, drop_empty=True, return_status=True)
    keep = np.nonzero(got.is_valid() & (np.diff(got.geom_offsets) > 0))[0]
    assert 0 < len(keep) < n and (src == keep).all() and src.dtype == np.int32 and (status2 == status).all()
    assert (status == S.ST_EMPTY).any()  # (equal polygons: an empty row that DROP_EMPTY leaves out)
    d = dropped.array
    assert d.is_valid().all() and _rows_of(d, range(len(keep))) == _rows_of(got, keep)
    assert d.xy.tobytes() == got.xy.tobytes() and (d.ring_offsets == got.ring_offsets).all() and (d.part_offsets == got.part_offsets).all()
    src_dev = torch.full((len(li),), -1, dtype=torch.int32, device="cuda")
    dd = polygon_symdiff_pairs_device(a.device(), b.device(), torch.from_numpy(li.view(np.int32)).cuda(), torch.from_numpy(ri.view(np.int32)).cuda(),
                                      drop_empty=True, out_src=src_dev)
    torch.cuda.synchronize()
    assert (src_dev.cpu().numpy()[: len(dd)] == keep).all() and dd.array.xy.tobytes() == d.xy.tobytes()
    assert (dd.array.geom_offsets == d.geom_offsets).all()


def test_refusals_with_real_handles(golden):
    """the mode, family and count refusals of the library itself, in gpk_polygon_clip's order, and an empty side, which gives null"""
    ca, cb = S.load(golden, PG, PG)
    a, b = GeoSeries(ca), GeoSeries(cb)
    lines = GeoSeries(X.column(L.R.LS, [[(0, 0), (1, 1)]] * len(a)))
    lib, out = _abi.lib(), C.c_void_p()
    call = lambda x, y, n, mode=0, flags=0: lib.gpk_polygon_symdiff(x.device().handle, y.device().handle, None, None, n, _abi.MEM_HOST, mode, flags, None,  # noqa: E731
                                                                   _abi.MEM_HOST, None, _abi.MEM_HOST, None, C.byref(out))
    assert call(lines, b, len(a)) == _abi.GPK_ERR_MISMATCHED_GEOMETRY and call(a, lines, len(a)) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    assert call(lines, b, len(a), mode=1) == _abi.GPK_ERR_INVALID_ARGUMENT and call(lines, b, len(a), flags=2) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert call(a, b, len(a), mode=1) == _abi.GPK_ERR_INVALID_ARGUMENT and call(a, b, len(a), mode=2) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert call(a, b, len(a) - 1) == _abi.GPK_ERR_INVALID_ARGUMENT and not out.value
    got, status = GeoSeries(X.column(PG, [[S.S10], []])).polygon_symmetric_difference(GeoSeries(X.column(PG, [[], [S.S10]])), return_status=True)
    assert not got.array.is_valid().any() and (status == S.ST_NULL).all()  # an empty row is not the neutral element


def test_zero_pairs_through_the_abi():
    """n_rows = 0 with host and with device row lists, with and without DROP_EMPTY (the Python layer never makes this call)"""
    clip_abi.RESULT_TYPE.setdefault("gpk_polygon_symdiff", _abi.GEOM_MULTIPOLYGON)  # (the shared helper learns the new entry's result type)
    clip_abi.check_zero_pairs("gpk_polygon_symdiff", _abi.PSYMDIFF_SYMMETRIC_DIFFERENCE)


# ---- 6. many blocks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes,n_pairs", [(4, 4099), (16, 4099), (4, 70001)])
def test_many_blocks(golden, lanes, n_pairs):
    """The fixture rows tiled to 4 099 and to 70 001 pairs (no multiple of 256 / G): ragged last blocks, offsets far past one scan
    tile, null and empty rows in between.  Every tile's rows must be the base rows, byte for byte."""
    ka, kb = MPG, MPG
    ca, cb, a, b = columns(golden, ka, kb, lanes)
    n = ca.n_geoms
    base = symdiff_rows(a, b, np.arange(n, dtype=np.uint32))[0]
    idx = (np.arange(n_pairs) % n).astype(np.uint32)
    got, status = polygon_symdiff_pairs(a, b, idx, idx, return_status=True)
    got = got.array
    full, rem = divmod(n_pairs, n)
    tile = lambda off, upto: np.concatenate([np.tile(np.diff(off), full), np.diff(off)[:upto]])  # noqa: E731
    bg, bp, br = base.geom_offsets, base.part_offsets, base.ring_offsets
    assert (np.diff(got.geom_offsets) == tile(bg, rem)).all() and got.geom_offsets[0] == 0
    assert (np.diff(got.part_offsets) == tile(bp, bg[rem])).all() and (np.diff(got.ring_offsets) == tile(br, bp[bg[rem]])).all()
    xy = np.concatenate([np.tile(base.xy, (full, 1)), base.xy[: br[bp[bg[rem]]]]])
    assert got.xy.tobytes() == xy.tobytes()
    assert (got.is_valid() == np.concatenate([np.tile(base.is_valid(), full), base.is_valid()[:rem]])).all()
    assert (status[:n] == golden[S.fixture_key(ka, kb) + HOW + "_status"]).all() and (status[n:2 * n] == status[:n]).all()


# ---- 7. arc tables around the LDS slice ---------------------------------------------------------------------------------------------------
def _lds_arcs_per_lane():
    m = re.search(r"constexpr int STITCH_LDS_ARCS_PER_LANE = (\d+);", open(os.path.join(CSRC, "gpk_polyclip_run.h")).read())
    return int(m.group(1))


@pytest.mark.parametrize("lanes", [4, 16])
def test_arc_tables_around_the_lds_slice(lanes):
    """The stitch reads a pair's arcs from its LDS slice up to STITCH_LDS_ARCS_PER_LANE arcs a lane and from global scratch beyond:
    pairs of one arc less than the slice, exactly the slice and one arc more — 7, 8, 9 at 4 lanes, 31, 32, 33 at 16, counted for this
    rule by the reference — against the reference.  That the header's arc machine hands the sink exactly these counts is pinned on
    the CPU: tests/test_polysymdiff_host.py runs the host driver on the same pairs and compares its arc count."""
    slice_arcs = _lds_arcs_per_lane() * lanes
    for (teeth, free), n_arcs in zip(S.SLICE_SHAPES[lanes], (slice_arcs - 1, slice_arcs, slice_arcs + 1)):
        a_row, b_row = S.comb_pair(teeth, free)
        assert S.arc_count(MPG, a_row, PG, b_row) == n_arcs, (teeth, free, S.arc_count(MPG, a_row, PG, b_row))
        cb = second_column(X.column(PG, [b_row]), lanes)
        a, b = GeoSeries(X.column(MPG, [a_row])), GeoSeries(cb)
        parts, st, gap = S.symdiff(MPG, a_row, PG, b_row)
        assert gap >= S.MIN_GAP
        got, status = symdiff_rows(a, b, np.zeros(1, dtype=np.uint32))
        assert status[0] == st == S.ST_OK
        want = np.array([(float(x), float(y)) for p in parts for r in p for x, y in r])
        assert got.xy.tobytes() == want.tobytes() and np.diff(got.ring_offsets).tolist() == [len(r) for p in parts for r in p]
        assert np.diff(got.part_offsets).tolist() == [len(p) for p in parts]


# ---- 8. rows on which the orientation filter fails on a non-zero sign ----------------------------------------------------------------------
# (the cases of test_gpu_hard_clip.CLIP_CASES: every figure of hard_clip.FORMS at both lane-group sizes — the 16-lane runs of the short
# forms take ballast rows, the long form of the pass figure has 16 lanes by itself: rings of 48 coordinates, longer than the group)
HARD_CASES = [("pass", "short", 4), ("pass", "short", 16), ("pass", "long", 16), ("pass", "multi", 4), ("spike", "short", 4), ("spike", "short", 16),
              ("nested", "short", 4), ("nested", "short", 16), ("hinge", "short", 4), ("hinge", "short", 16)]


def hard_selection(figure, gen, form):
    """The rows of hard_clip.poly_rows a case runs: all of them, but of the long form every fourth row of each (kind, sign) of its
    triples — the arc of the long ring is one construction (tests/test_hard_orient.py samples it too) and the exact reference takes
    0.04 s a row there: 50 rows, 24 of them hard, every kind and sign among them."""
    ts = K.poly_rows(figure, gen, form)[0]
    if form != "long":
        return list(range(len(ts)))
    seen, sel = {}, []
    for i, t in enumerate(ts):
        k = (t.kind, t.sign)
        if seen.get(k, 0) % 4 == 0:
            sel.append(i)
        seen[k] = seen.get(k, 0) + 1
    return sel


@lru_cache(maxsize=None)
def hard_expected(figure, gen, form, swapped):
    """[hard_clip.PolyResult] of the symmetric difference over the rows of hard_selection, by the exact reference on each pair's
    integer grid"""
    _ts, ka, A, kb, B = K.poly_rows(figure, gen, form)
    if swapped:
        ka, A, kb, B = kb, B, ka, A
    out = []
    for i in hard_selection(figure, gen, form):
        ia, ib = H.on_integer_grid(A[i], B[i])
        parts, status, _gap = S.symdiff(ka, ia, kb, ib)
        out.append(K.PolyResult(parts, status, ka, ia, kb, ib, H.integer_grid_scale(A[i], B[i])))
    return out


@pytest.mark.parametrize("figure,form,lanes", HARD_CASES, ids=[f"{f}-{form}-G{g}" for f, form, g in HARD_CASES])
@pytest.mark.parametrize("gen", K.GENS)
def test_hard_orientation_rows(gpk, gen, figure, form, lanes):
    """the figures of tests/hard_clip.py — the stage-A orientation filter gives up on a planted triple whose exact sign is not zero —
    through gpk_polygon_symdiff in both operand orders, against the reference: a site that took its sign from a double cross product
    returns the other sign's shape on half of the rows"""
    ts, ka, A, kb, B = K.poly_rows(figure, gen, form)
    sel = hard_selection(figure, gen, form)
    hard = [i for i in sel if ts[i].kind in H.HARD]
    assert len(hard) >= (24 if form == "long" else 96) and {ts[i].sign for i in hard} == {1, -1}
    A, B = [A[i] for i in sel], [B[i] for i in sel]
    if form == "long":
        assert lanes_of(X.column(ka, A)) == 16  # (by itself: no ballast where the long ring is the second operand)
    for swapped in (False, True):
        exp = hard_expected(figure, gen, form, swapped)
        xa, xb = (X.column(kb, B), X.column(ka, A)) if swapped else (X.column(ka, A), X.column(kb, B))
        a, b = GeoSeries(xa), GeoSeries(second_column(xb, lanes))
        rows = np.arange(len(sel), dtype=np.uint32)
        got, status = a.polygon_symmetric_difference(b, other_rows=rows, return_status=True)
        worst, n_x = S.check_rows([r.scaled_back() for r in exp], [r.status for r in exp], xa, xb, got.array, status)
        print(f"{gen} {figure} {form} swapped={swapped} G={lanes}: {len(sel)} rows, {n_x} crossings, worst distance / bound = {worst:.3e}")
