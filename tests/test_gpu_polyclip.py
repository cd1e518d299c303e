"""GPU: polygon x polygon intersection and difference (gpk_polygon_clip, csrc/gpk_polyclip.hip) against the exact rational reference
(tests/polyclip_ref.py; tests/test_polyclip_ref.py pins it) and against the kernels the library already has.

Contract (include/geopolars_hip.h): offsets, validity, status and ring starts exactly; input coordinates bit for bit; a computed
crossing within 1e-9 * d of both carrying edges, d = the diagonal of the pair's joint box.

  1. every fixture row, both modes, both lane-group sizes, both placements; 2. the hand cases by name; 3. exact areas of the returned
  rings; 4. cross-checks against intersection_area, area, is_valid and the relation mask on 20 000 random pairs; 5. row lists, an
  out-of-range index, DROP_EMPTY with out_src; 6. many blocks; 7. arc tables past the LDS slice; 8. the join."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import polygon_clip_pairs, polygon_clip_pairs_device, polygon_relation_pairs, spatial_join_overlay
from tests import clip_abi
from tests import exact_ref as X
from tests import overlay_ref as O
from tests import polyclip_ref as L
from tests.test_gpu_lineclip import N_BALLAST, lanes_of, with_ballast

pytestmark = pytest.mark.gpu

PG, MPG = L.PG, L.MPG
FAMILY_IDS = [f"{L.NAMES[a]}-{L.NAMES[b]}" for a, b in L.FAMILIES]
HOW = {L.INTERSECTION: "intersection", L.DIFFERENCE: "difference"}


@pytest.fixture(scope="module")
def golden():
    return np.load(L.GOLDEN)


def columns(golden, ka, kb, lanes, offset=(0.0, 0.0)):
    """the two fixture columns; for 16 lanes b carries ballast rows that no pair names (they lift its mean coordinate count past 32)"""
    ca, cb = L.load(golden, ka, kb, offset)
    both = cb if lanes == 4 else with_ballast(cb, N_BALLAST)
    assert lanes_of(both) == lanes, (both.n_coords, both.n_geoms)
    return ca, cb, GeoSeries(ca), GeoSeries(both)


def clip_rows(a: GeoSeries, b: GeoSeries, mode, rows):
    call = a.polygon_intersection if mode == L.INTERSECTION else a.polygon_difference
    out, status = call(b, other_rows=rows, return_status=True)
    return out.array, status


# ---- 1. every fixture row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["lattice", "georeferenced"])
@pytest.mark.parametrize("lanes", [4, 16])
@pytest.mark.parametrize("mode", [L.INTERSECTION, L.DIFFERENCE], ids=["intersection", "difference"])
@pytest.mark.parametrize("ka,kb", L.FAMILIES, ids=FAMILY_IDS)
def test_every_fixture_row(golden, ka, kb, mode, lanes, placement):
    """offsets, validity, status and ring starts exactly, input coordinates bit for bit, crossings within the bound — through
    GeoSeries.polygon_intersection / polygon_difference with a row map, and once more, byte for byte, through device buffers"""
    offset = (0.0, 0.0) if placement == "lattice" else L.TRANSLATION
    ca, cb, a, b = columns(golden, ka, kb, lanes, offset)
    rows = np.arange(ca.n_geoms, dtype=np.uint32)
    got, status = clip_rows(a, b, mode, rows)
    worst = L.check_result(golden, ka, kb, mode, ca, cb, got, status, offset)
    print(f"{FAMILY_IDS[L.FAMILIES.index((ka, kb))]} {L.MODES[mode]} G={lanes} {placement}: worst crossing distance / bound = {worst:.3e}")
    r = torch.from_numpy(rows.view(np.int32)).cuda()
    st = torch.full((len(rows),), 255, dtype=torch.uint8, device="cuda")
    dev = polygon_clip_pairs_device(a.device(), b.device(), None, r, HOW[mode], out_status=st).array
    assert dev.xy.tobytes() == got.xy.tobytes() and (dev.ring_offsets == got.ring_offsets).all() and (dev.part_offsets == got.part_offsets).all()
    assert (dev.geom_offsets == got.geom_offsets).all() and (dev.is_valid() == got.is_valid()).all() and (st.cpu().numpy() == status).all()


# ---- 2. the hand cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [4, 16])
def test_hand_cases(lanes):
    """the smallest shapes that can go wrong, by name, with their (parts, rings) stated by hand (they are rows of the fixture too)"""
    ka, kb = MPG, MPG
    A, B, av, bv, names = L.rows(ka, kb)
    want = L.hand_expectations(ka, kb)
    assert len(want) == len(L.HAND_CASES)
    idx = list(want) + [names.index(s) for s in ("a null a", "a null b", "an empty a", "an empty b", "an invalid ring in a", "an invalid ring in b")]
    ca = X.column(ka, [A[i] for i in idx], [av[i] for i in idx])
    cb = X.column(kb, [B[i] for i in idx], [bv[i] for i in idx])
    if lanes == 16:
        cb = with_ballast(cb, N_BALLAST)
    assert lanes_of(cb) == lanes
    rows = np.arange(len(idx), dtype=np.uint32)
    (inter, st_i), (diff, st_d) = clip_rows(GeoSeries(ca), GeoSeries(cb), L.INTERSECTION, rows), clip_rows(GeoSeries(ca), GeoSeries(cb), L.DIFFERENCE, rows)

    def counts(col, k):
        p0, p1 = col.geom_offsets[k], col.geom_offsets[k + 1]
        return int(p1 - p0), int(col.part_offsets[p1] - col.part_offsets[p0])

    for k, i in enumerate(idx[: len(want)]):
        got = (counts(inter, k), counts(diff, k))
        assert got == want[i], (names[i], got, want[i])
    n = len(want)
    assert not inter.is_valid()[n:].any() and not diff.is_valid()[n:].any() and (st_i[n:] == L.ST_NULL).all() and (st_d[n:] == L.ST_NULL).all()
    assert inter.is_valid()[:n].all() and diff.is_valid()[:n].all()
    by_name = {names[i]: k for k, i in enumerate(idx)}
    k = by_name["b inside a touching from within at a point: the hole fuses into the shell"]
    assert st_d[k] == L.ST_TOUCH and st_i[k] == L.ST_OK
    assert set(np.concatenate([st_i[:n], st_d[:n]]).tolist()) <= {L.ST_OK, L.ST_TOUCH, L.ST_EMPTY}
    # equal polygons intersect to a itself, a's own coordinates from a's own start
    k = by_name["equal polygons"]
    r0 = inter.part_offsets[inter.geom_offsets[k]]
    assert (inter.xy[inter.ring_offsets[r0]:inter.ring_offsets[r0 + 1]] == np.array(L.S10, dtype=np.float64)).all() and st_d[k] == L.ST_EMPTY


# ---- 3. exact areas of the returned rings ---------------------------------------------------------------------------------------------
def _exact_ring_area2(xy):
    f = [(Fraction(float(x)), Fraction(float(y))) for x, y in xy]
    return sum(f[i][0] * f[i + 1][1] - f[i + 1][0] * f[i][1] for i in range(len(f) - 1))


def _perimeter(col, i, starts):
    c0, c1 = starts[i], starts[i + 1]
    r = col.ring_offsets
    rings = [(a, b) for a, b in zip(r[:-1], r[1:]) if c0 <= a and b <= c1 and b - a > 1]
    return float(sum(np.hypot(*np.diff(col.xy[a:b], axis=0).T).sum() for a, b in rings))


@pytest.mark.parametrize("mode", [L.INTERSECTION, L.DIFFERENCE], ids=["intersection", "difference"])
@pytest.mark.parametrize("ka,kb", L.FAMILIES, ids=FAMILY_IDS)
def test_exact_area_of_the_returned_rings(golden, ka, kb, mode):
    """For every OK row the exact (Fraction) area of the RETURNED rings differs from the exact result — overlay_ref.exact_area, which
    shares no code with the clip or its reference — by at most 1e-9 * d * (perimeter(a) + perimeter(b)): every moved vertex moves by at
    most 1e-9 * d (the fixture holds the correctly rounded exact crossing), and the output's perimeter is at most the operands' sum."""
    ca, cb, a, b = columns(golden, ka, kb, 4)
    A, B, av, bv, _names = L.rows(ka, kb)
    got, status = clip_rows(a, b, mode, np.arange(ca.n_geoms, dtype=np.uint32))
    key = L.fixture_key(ka, kb) + L.MODES[mode] + "_"
    exact_xy, tag = golden[key + "xy"], golden[key + "tag"]
    assert len(exact_xy) == len(got.xy)
    d = L.pair_diagonals(ca, cb)
    sa, sb = np.append(L._row_starts(ca), len(ca.xy)), np.append(L._row_starts(cb), len(cb.xy))
    so = np.append(got.ring_offsets[got.part_offsets[got.geom_offsets[:-1]]], len(got.xy))
    worst_area, worst_move, n_ok = 0.0, 0.0, 0
    for i in range(ca.n_geoms):
        if status[i] not in (L.ST_OK, L.ST_TOUCH):
            continue
        n_ok += 1
        c0, c1 = so[i], so[i + 1]
        moved = np.hypot(*(got.xy[c0:c1] - exact_xy[c0:c1]).T)
        assert (moved[tag[c0:c1] == L.TAG_IN] == 0).all()
        worst_move = max(worst_move, float(moved.max()) / (L.REL_TOL * d[i]))
        r0, r1 = got.part_offsets[got.geom_offsets[i]], got.part_offsets[got.geom_offsets[i + 1]]
        area = sum((_exact_ring_area2(got.xy[got.ring_offsets[r]:got.ring_offsets[r + 1]]) for r in range(r0, r1)), Fraction(0)) / 2
        shared = O.exact_area(ka, A[i], kb, B[i])
        want = shared if mode == L.INTERSECTION else L.row_area(ka, A[i]) - shared
        pa, pb = _perimeter(ca, i, sa), _perimeter(cb, i, sb)
        worst_area = max(worst_area, float(abs(area - want)) / (L.REL_TOL * d[i] * (pa + pb)))
        assert _perimeter(got, i, so) <= (pa + pb) * (1 + 1e-12)
    print(f"{FAMILY_IDS[L.FAMILIES.index((ka, kb))]} {L.MODES[mode]}: {n_ok} rows, worst |area - exact| / bound = {worst_area:.3e}, worst move / bound = {worst_move:.3e}")
    assert n_ok > 50 and worst_area <= 1.0 and worst_move <= 1.0


# ---- 4. cross-checks against the kernels the library already has ------------------------------------------------------------------------
def lattice_triangles(n, rng, size=16):
    """n non-degenerate triangles on a size x size lattice, stored in either order.  The gap condition holds by construction: a
    transition parameter on a segment is a ratio of two cross products of lattice differences, each at most 2 * size^2 = 512 in size, so
    two distinct ones differ by at least 1 / 512^2 = 3.8e-6 > 1e-6 (asserted below on the integers)."""
    out = []
    while len(out) < n:
        p = rng.integers(0, size + 1, (3, 2))
        cr = int((p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[1, 1] - p[0, 1]) * (p[2, 0] - p[0, 0]))
        if cr != 0:
            t = [tuple(int(c) for c in v) for v in p]
            out.append([t + [t[0]]])
    return out


def test_cross_checks_on_random_pairs():
    """20 000 lattice triangle pairs (coincident vertices, vertices on edges and shared edge pieces are frequent).  area(intersection)
    is intersection_area within that kernel's documented 1e-9 * (d_a^2 + d_b^2) plus the clip's own 1e-9 * d * perimeter; the areas of
    the intersection and of the difference sum to area(a); every status-0 row is valid; the relation mask of (result, a) has no point of
    the result's interior outside a; no row has status 4."""
    rng = np.random.default_rng(41)
    n, size = 20000, 16
    assert 1.0 / (2 * size * size) ** 2 > 1e-6  # the gap, by construction
    ta, tb = lattice_triangles(n, rng, size), lattice_triangles(n, rng, size)
    a, b = GeoSeries(X.column(PG, ta)), GeoSeries(X.column(PG, tb))
    (inter, st_i), (diff, st_d) = a.polygon_intersection(b, return_status=True), a.polygon_difference(b, return_status=True)
    print("status counts, intersection:", np.bincount(st_i, minlength=5).tolist(), "difference:", np.bincount(st_d, minlength=5).tolist())
    assert (st_i != L.ST_UNRESOLVED).all() and (st_d != L.ST_UNRESOLVED).all() and (st_i != L.ST_NULL).all()
    area_a, shared = a.area(), a.intersection_area(b)
    ai, ad = inter.area(), diff.area()
    # d^2 <= 2 size^2 for a row and for the joint box, a perimeter <= 3 d: the measure's 1e-9 (d_a^2 + d_b^2), the clip's 1e-9 d * 6 d
    d2 = 2.0 * size * size
    tol_measure, tol_clip = 2e-9 * d2, 6e-9 * d2
    print(f"worst |area(intersection) - intersection_area| = {float(np.abs(ai - shared).max()):.3e} (bound {tol_measure + tol_clip:.3e}), "
          f"worst |area(intersection) + area(difference) - area(a)| = {float(np.abs(ai + ad - area_a).max()):.3e} (bound {2 * tol_clip:.3e})")
    assert (np.abs(ai - shared) <= tol_measure + tol_clip).all()
    assert (np.abs(ai + ad - area_a) <= 2 * tol_clip).all()
    assert ((st_i == L.ST_EMPTY) == (ai == 0)).all()
    ok = st_i == L.ST_OK
    assert ok.sum() > 5000 and inter.is_valid()[ok].all() and diff.is_valid()[st_d == L.ST_OK].all()
    some = np.nonzero(ok)[0]
    mask = GeoSeries(inter.array.take(some.astype(np.int64))).polygon_relation(a, other_rows=some.astype(np.uint32))
    outside = (mask & 4) != 0
    print(f"rows whose intersection has a point outside a by the exact relation on the rounded coordinates: {int(outside.sum())} of {len(some)}")
    assert not outside.any()


# ---- 5. row lists --------------------------------------------------------------------------------------------------------------------
def _rows_of(col: GeoArrowArray, sel):
    """the selected rows of a MULTIPOLYGON column, row by row: validity, ring counts per part, coordinate counts per ring, bytes"""
    g, p, r = col.geom_offsets, col.part_offsets, col.ring_offsets
    out = []
    for i in sel:
        p0, p1 = g[i], g[i + 1]
        out.append((bool(col.is_valid()[i]), np.diff(p[p0:p1 + 1]).tolist(), np.diff(r[p[p0]:p[p1] + 1]).tolist(), col.xy[r[p[p0]]:r[p[p1]]].tobytes()))
    return out


@pytest.mark.parametrize("mode", [L.INTERSECTION, L.DIFFERENCE], ids=["intersection", "difference"])
def test_row_lists_and_drop_empty(golden, mode):
    """permuted row lists give the rows of the identity call; an index past the end of either column gives a null row of status 3; with
    DROP_EMPTY the column is the undropped one with its empty and null rows removed, byte for byte, and out_src names them"""
    ka, kb = MPG, MPG
    ca, cb = L.load(golden, ka, kb)
    a, b = GeoSeries(ca), GeoSeries(cb)
    base = (a.polygon_intersection if mode == L.INTERSECTION else a.polygon_difference)(b).array
    n = ca.n_geoms
    perm = np.random.default_rng(3).permutation(n).astype(np.uint32)
    got = polygon_clip_pairs(a, b, perm, perm, HOW[mode]).array
    assert _rows_of(got, range(n)) == _rows_of(base, perm)
    li, ri = np.concatenate([perm, [n, 0, 2**32 - 1]]).astype(np.uint32), np.concatenate([perm, [0, cb.n_geoms, 1]]).astype(np.uint32)
    got, status = polygon_clip_pairs(a, b, li, ri, HOW[mode], return_status=True)
    got = got.array
    assert _rows_of(got, range(n)) == _rows_of(base, perm)
    assert not got.is_valid()[n:].any() and (np.diff(got.geom_offsets)[n:] == 0).all() and (status[n:] == L.ST_NULL).all()
    dropped, src, status2 = polygon_clip_pairs(a, b, li, ri, HOW[mode], drop_empty=True, return_status=True)
    keep = np.nonzero(got.is_valid() & (np.diff(got.geom_offsets) > 0))[0]
    assert 0 < len(keep) < n and (src == keep).all() and src.dtype == np.int32 and (status2 == status).all()
    d = dropped.array
    assert d.is_valid().all() and _rows_of(d, range(len(keep))) == _rows_of(got, keep)
    assert d.xy.tobytes() == got.xy.tobytes() and (d.ring_offsets == got.ring_offsets).all() and (d.part_offsets == got.part_offsets).all()
    src_dev = torch.full((len(li),), -1, dtype=torch.int32, device="cuda")
    dd = polygon_clip_pairs_device(a.device(), b.device(), torch.from_numpy(li.view(np.int32)).cuda(), torch.from_numpy(ri.view(np.int32)).cuda(),
                                   HOW[mode], drop_empty=True, out_src=src_dev)
    torch.cuda.synchronize()
    assert (src_dev.cpu().numpy()[: len(dd)] == keep).all() and dd.array.xy.tobytes() == d.xy.tobytes()
    assert (dd.array.geom_offsets == d.geom_offsets).all()


def test_refusals_with_real_handles(golden):
    """the family and count refusals of the library itself, and a result that is empty"""
    import ctypes as C

    ca, cb = L.load(golden, PG, PG)
    a, b = GeoSeries(ca), GeoSeries(cb)
    lines = GeoSeries(X.column(L.R.LS, [[(0, 0), (1, 1)]] * len(a)))
    lib, out = _abi.lib(), C.c_void_p()
    call = lambda x, y, n, mode=0, flags=0: lib.gpk_polygon_clip(x.device().handle, y.device().handle, None, None, n, _abi.MEM_HOST, mode, flags, None,  # noqa: E731
                                                                _abi.MEM_HOST, None, _abi.MEM_HOST, None, C.byref(out))
    assert call(lines, b, len(a)) == _abi.GPK_ERR_MISMATCHED_GEOMETRY and call(a, lines, len(a)) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    assert call(a, b, len(a) - 1) == _abi.GPK_ERR_INVALID_ARGUMENT and not out.value
    far = GeoSeries(X.column(PG, [[L.S10]])).polygon_intersection(GeoSeries(X.column(PG, [[L.sq(40, 40, 50, 50)]])))
    assert len(far) == 1 and far.array.is_valid().all() and len(far.array.xy) == 0 and far.array.ring_offsets.tolist() == [0]
    assert far.array.part_offsets.tolist() == [0] and far.array.geom_offsets.tolist() == [0, 0]


def test_zero_pairs_through_the_abi():
    """n_rows = 0 with host and with device row lists, with and without DROP_EMPTY (the Python layer never makes this call)"""
    clip_abi.check_zero_pairs("gpk_polygon_clip", _abi.PCLIP_INTERSECTION)


def test_every_pair_dropped_through_the_abi():
    clip_abi.check_every_pair_dropped("gpk_polygon_clip", _abi.PCLIP_INTERSECTION)


def test_a_partial_last_byte_of_the_bitmap():
    clip_abi.check_bitmap_edge("gpk_polygon_clip", _abi.PCLIP_INTERSECTION)


# ---- 6. many blocks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes,n_pairs", [(4, 4099), (16, 4099), (4, 70001)])
def test_many_blocks(golden, lanes, n_pairs):
    """The fixture rows tiled to 4 099 and to 70 001 pairs (no multiple of 256 / G): ragged last blocks, offsets far past one scan
    tile, empty and null rows in between.  Every tile's rows must be the base rows, byte for byte."""
    ka, kb = MPG, MPG
    ca, cb, a, b = columns(golden, ka, kb, lanes)
    n = ca.n_geoms
    base = a.polygon_intersection(b, other_rows=np.arange(n, dtype=np.uint32)).array
    idx = (np.arange(n_pairs) % n).astype(np.uint32)
    got, status = polygon_clip_pairs(a, b, idx, idx, "intersection", return_status=True)
    got = got.array
    full, rem = divmod(n_pairs, n)
    tile = lambda off, upto: np.concatenate([np.tile(np.diff(off), full), np.diff(off)[:upto]])  # noqa: E731
    bg, bp, br = base.geom_offsets, base.part_offsets, base.ring_offsets
    assert (np.diff(got.geom_offsets) == tile(bg, rem)).all() and got.geom_offsets[0] == 0
    assert (np.diff(got.part_offsets) == tile(bp, bg[rem])).all() and (np.diff(got.ring_offsets) == tile(br, bp[bg[rem]])).all()
    xy = np.concatenate([np.tile(base.xy, (full, 1)), base.xy[: br[bp[bg[rem]]]]])
    assert got.xy.tobytes() == xy.tobytes()
    assert (got.is_valid() == np.concatenate([np.tile(base.is_valid(), full), base.is_valid()[:rem]])).all()
    assert (status[:n] == golden[L.fixture_key(ka, kb) + "intersection_status"]).all() and (status[n:2 * n] == status[:n]).all()


# ---- 7. arc tables past the LDS slice ----------------------------------------------------------------------------------------------------
def comb(teeth):
    """a comb of `teeth` teeth of width 2 and height 10 on a base of height 4"""
    ring = [(0, 0), (4 * teeth - 2, 0)]
    for k in range(teeth - 1, -1, -1):
        ring += [(4 * k + 2, 10), (4 * k, 10)] + ([(4 * k, 4), (4 * k - 2, 4)] if k else [])
    return ring + [(0, 0)]


@pytest.mark.parametrize("lanes,teeth", [(4, 4), (4, 5), (16, 16), (16, 17)])
def test_arc_tables_around_the_lds_slice(lanes, teeth):
    """A bar across a comb of T teeth: the intersection has 2 T arcs.  The stitch reads a pair's arcs from its LDS slice up to 2 arcs a
    lane — 8 at 4 lanes, 32 at 16 — and from global scratch beyond: the largest comb that fits and the smallest that does not, both
    modes, against the reference."""
    a_row, b_row = [comb(teeth)], [L.sq(-1, 6, 4 * teeth + 1, 8)]
    cb = X.column(PG, [b_row])
    if lanes == 16:
        cb = with_ballast(cb, N_BALLAST)
    assert lanes_of(cb) == lanes
    a, b = GeoSeries(X.column(PG, [a_row])), GeoSeries(cb)
    for mode in (L.INTERSECTION, L.DIFFERENCE):
        parts, st, _gap = L.clip(PG, a_row, PG, b_row, mode)
        got, status = clip_rows(a, b, mode, np.zeros(1, dtype=np.uint32))
        assert status[0] == st == L.ST_OK and len(parts) == (teeth if mode == L.INTERSECTION else teeth + 1)
        want = np.array([(float(x), float(y)) for p in parts for r in p for x, y in r])
        assert got.xy.tobytes() == want.tobytes() and np.diff(got.ring_offsets).tolist() == [len(r) for p in parts for r in p]
        assert np.diff(got.part_offsets).tolist() == [len(p) for p in parts]


# ---- 8. the join ---------------------------------------------------------------------------------------------------------------------
def test_spatial_join_overlay():
    """on the join fixture of overlay_ref.join_rows.  Intersection: the pairs are exactly the reference's pairs with positive area, a
    subset of the intersects join, and the geometry is, byte for byte, the row-wise call on the same pairs.  Difference: one row per pair
    of the intersects join whose left row the reference does not find covered."""
    z = np.load(O.GOLDEN)
    left, right = GeoSeries(O.unpack(z, "join_left_", PG)), GeoSeries(O.unpack(z, "join_right_", PG))
    table = z["join_area"]
    table = table[table[:, 2] > 0]
    table = table[np.lexsort((table[:, 1], table[:, 0]))]
    want = table[:, :2].astype(np.int64)
    l, r, geom = spatial_join_overlay(left, right, "intersection")
    assert (np.stack([l, r], axis=1) == want).all() and len(want) > 50
    joined, _, _ = polygon_relation_pairs(left, right, "intersects")
    assert len(joined) > len(want)
    rowwise = polygon_clip_pairs(left, right, l, r, "intersection").array
    g = geom.array
    assert g.xy.tobytes() == rowwise.xy.tobytes() and (g.ring_offsets == rowwise.ring_offsets).all() and (g.part_offsets == rowwise.part_offsets).all()
    assert g.is_valid().all() and (np.diff(g.geom_offsets) > 0).all()
    assert (np.abs(geom.area() - table[:, 2]) <= 1e-9 * 450.0 * 4 * 450.0).all()
    rows_l, rows_r, _lines = O.join_rows()
    l2, r2, geom2 = spatial_join_overlay(left, right, "difference")
    want2 = [(int(i), int(j)) for i, j in joined.astype(np.int64) if L.clip(PG, rows_l[i], PG, rows_r[j], L.DIFFERENCE)[1] != L.ST_EMPTY]
    assert list(zip(l2.tolist(), r2.tolist())) == want2 and 0 < len(want2) <= len(joined)
    with pytest.raises(_abi.GeopolarsHipError):
        spatial_join_overlay(left, right, "union")
