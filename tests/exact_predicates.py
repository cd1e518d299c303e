"""Exact answers for the polygon predicates (row-wise contains / within / intersects and the polygon joins), and seeded fixtures
that select every compiled path of their kernels.

Every f64 is an integer times a power of two, so the coordinates a predicate looks at are integers at one common exponent and
every orientation is an exact integer: int64 when the coordinates span at most 29 bits (the dyadic lattices below), Python
integers in numpy object arrays otherwise (points one ulp off a vertex or an edge).  No floating-point step decides anything.

Three statements:
- point position (geo 0.27's coordinate_position restated: winding number with its edge rules, holes, multipolygon members);
- intersects(polygon, polygon): geo 0.27's algorithm restated (exterior boxes, every segment of B's rings against every segment
  of A's rings, the endpoints of B's segments against A, the endpoints of A's exterior segments against B).  On valid polygons
  this is the closed-set statement of test_oracle_rational.intersects_bruteforce (checked on a sample); on invalid inputs (rings
  of 1 to 3 coordinates, open rings, an empty exterior with a hole, a hole poking out) it is what the oracle computes;
- contains(polygon, polygon): the set statement "B is not empty and B is a subset of A" of
  test_oracle_rational.contains_bruteforce, by the same edge splitting with exact integer boxes pruning the edge pairs first."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from geopolars_amd import _abi

OUTSIDE, BOUNDARY, INSIDE = -1, 0, 1


# ---- exact integers ------------------------------------------------------------------------------------------------------------


def scaled_ints(*arrays):
    """float arrays -> integer arrays (same shapes) with array == ints * 2^E for one common E; int64 when every value has at most
    29 significant bits at that exponent (differences and orientations then fit int64), else Python ints (object dtype)"""
    flat = np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in arrays]) if arrays else np.zeros(0)
    assert np.isfinite(flat).all(), "exact predicates take finite coordinates"
    m, e = np.frexp(flat)
    mi = (m * 2.0**53).astype(np.int64)
    ex = e.astype(np.int64) - 53
    nz = mi != 0
    if not nz.any():
        return [np.zeros(np.shape(a), dtype=np.int64) for a in arrays]
    tz = np.zeros_like(mi)
    low = np.abs(mi[nz]) & -np.abs(mi[nz])
    tz[nz] = np.round(np.log2(low.astype(np.float64))).astype(np.int64)
    E = int(np.min((ex + tz)[nz]))
    core = np.where(nz, mi >> np.where(nz, tz, 0), 0)
    sh = np.where(nz, ex + tz - E, 0)
    bits = np.where(nz, np.ceil(np.log2(np.abs(core).astype(np.float64) + 1)).astype(np.int64) + sh, 0)
    if int(bits.max()) <= 29:
        out = core << sh
    else:
        out = np.array([int(c) << int(s) for c, s in zip(core.tolist(), sh.tolist())], dtype=object)
    res, k = [], 0
    for a in arrays:
        n = int(np.size(a))
        res.append(out[k : k + n].reshape(np.shape(a)))
        k += n
    return res


def _sign(v):
    return np.sign(v).astype(np.int64) if v.dtype != object else np.array([(x > 0) - (x < 0) for x in v.ravel()], dtype=np.int64).reshape(v.shape)


def orient(ax, ay, bx, by, cx, cy):
    """exact sign of the orientation of (a, b, c), element-wise over broadcast integer arrays"""
    return _sign((bx - ax) * (cy - ay) - (by - ay) * (cx - ax))


# ---- point position ------------------------------------------------------------------------------------------------------------


def ring_pos(px, py, ring):
    """geo's coord_pos_relative_to_ring for integer points (px, py: 1-d) against an integer ring ((n, 2)): upward edges count
    their start, downward edges their end, horizontal edges never; a point on an edge is on the boundary"""
    n = len(ring)
    px, py = np.asarray(px)[:, None], np.asarray(py)[:, None]
    if n == 0:
        return np.full(px.shape[0], OUTSIDE)
    if n == 1:
        return np.where((px[:, 0] == ring[0, 0]) & (py[:, 0] == ring[0, 1]), BOUNDARY, OUTSIDE)
    sx, sy, ex, ey = ring[:-1, 0][None], ring[:-1, 1][None], ring[1:, 0][None], ring[1:, 1][None]
    o = orient(sx, sy, ex, ey, px, py)
    up = (sy <= py) & (ey >= py)
    dn = (sy > py) & (ey <= py)
    between = ((px >= sx) & (px <= ex)) | ((px >= ex) & (px <= sx))
    on = ((up | dn) & (o == 0) & between).any(axis=1)
    wn = ((up & (o > 0) & (ey != py)).astype(np.int64) - (dn & (o < 0)).astype(np.int64)).sum(axis=1)
    return np.where(on, BOUNDARY, np.where(wn != 0, INSIDE, OUTSIDE))


def polygon_pos(px, py, rings):
    """geo's Polygon::coordinate_position: no rings or an empty exterior -> outside; exterior not inside -> its answer; then a
    hole's boundary is the boundary and a hole's inside is outside"""
    m = len(np.atleast_1d(px))
    if not rings or len(rings[0]) == 0:
        return np.full(m, OUTSIDE)
    pos = ring_pos(px, py, rings[0])
    for h in rings[1:]:
        ph = ring_pos(px, py, h)
        pos = np.where(pos == INSIDE, np.where(ph == BOUNDARY, BOUNDARY, np.where(ph == INSIDE, OUTSIDE, INSIDE)), pos)
    return pos


def _int_polys(polys, *points):
    """(list of polygons of integer rings, integer points...) at one exponent"""
    rings = [np.asarray(r, dtype=np.float64).reshape(-1, 2) for p in polys for r in p]
    conv = scaled_ints(*rings, *[np.asarray(q, dtype=np.float64) for q in points])
    it = iter(conv[: len(rings)])
    return [[next(it) for _ in p] for p in polys], conv[len(rings) :]


def point_positions(P, polys):
    """positions (per member: (n_points, n_members)) of the points P ((n, 2) floats) in a (multi)polygon given as a list of
    polygons of float rings"""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    ip, (iP,) = _int_polys(polys, P)
    if not ip:
        return np.full((len(P), 0), OUTSIDE)
    return np.stack([polygon_pos(iP[:, 0], iP[:, 1], rings) for rings in ip], axis=1)


def point_predicate(p, polys, predicate):
    """contains(polys, p) / within(p, polys) = some member has p inside; intersects = some member has p not outside.  A NaN
    point or an empty geometry: false."""
    if p is None or np.isnan(p).any() or not polys:
        return False
    pos = point_positions(np.asarray(p)[None], polys)[0]
    return bool((pos != OUTSIDE).any() if predicate == "intersects" else (pos == INSIDE).any())


# ---- intersects(polygon, polygon): geo 0.27's algorithm --------------------------------------------------------------------------


def _segments(rings):
    s = [(r[:-1], r[1:]) for r in rings if len(r) >= 2]
    if not s:
        return None
    return np.concatenate([a for a, _ in s]), np.concatenate([b for _, b in s])


def segments_meet(A, B):
    """any pair of closed segments (A: (a0, a1) arrays, B likewise) meets: geo's line_intersects_line, exactly, with an exact
    box prune first"""
    (a0, a1), (b0, b1) = A, B
    alo, ahi = np.minimum(a0, a1), np.maximum(a0, a1)
    blo, bhi = np.minimum(b0, b1), np.maximum(b0, b1)
    boxes = (alo[:, None, 0] <= bhi[None, :, 0]) & (blo[None, :, 0] <= ahi[:, None, 0]) & (alo[:, None, 1] <= bhi[None, :, 1]) & (blo[None, :, 1] <= ahi[:, None, 1])
    ia, ib = np.nonzero(boxes)
    if len(ia) == 0:
        return False
    p0, p1, q0, q1 = a0[ia], a1[ia], b0[ib], b1[ib]
    c11 = orient(p0[:, 0], p0[:, 1], p1[:, 0], p1[:, 1], q0[:, 0], q0[:, 1])
    c12 = orient(p0[:, 0], p0[:, 1], p1[:, 0], p1[:, 1], q1[:, 0], q1[:, 1])
    c21 = orient(q0[:, 0], q0[:, 1], q1[:, 0], q1[:, 1], p0[:, 0], p0[:, 1])
    c22 = orient(q0[:, 0], q0[:, 1], q1[:, 0], q1[:, 1], p1[:, 0], p1[:, 1])
    degen = (p0[:, 0] == p1[:, 0]) & (p0[:, 1] == p1[:, 1])
    # a degenerate first segment: the point on the second; collinear: (the boxes already overlap) they meet; else proper test
    hit = np.where(degen, c21 == 0, np.where(c11 != c12, c21 != c22, c11 == 0))
    return bool(hit.any())


def _box(ring):
    return ring.min(axis=0), ring.max(axis=0)


def polygon_intersects_int(A, B):
    """geo's Intersects<Polygon> for Polygon on integer rings ([exterior, hole...])"""
    if not A or not B or len(A[0]) == 0 or len(B[0]) == 0:
        return False
    (alo, ahi), (blo, bhi) = _box(A[0]), _box(B[0])
    if (ahi < blo).any() or (bhi < alo).any():
        return False
    sa, sb = _segments(A), _segments(B)
    if sa is not None and sb is not None and segments_meet(sa, sb):
        return True
    vb = [r for r in B if len(r) >= 2]
    if vb:
        V = np.concatenate(vb)
        if (polygon_pos(V[:, 0], V[:, 1], A) != OUTSIDE).any():
            return True
    if len(A[0]) >= 2 and (polygon_pos(A[0][:, 0], A[0][:, 1], B) != OUTSIDE).any():
        return True
    return False


def intersects(pa, pb) -> bool:
    """intersects of two geometries, each a list of polygons of float rings: some pair of members intersects"""
    ip, _ = _int_polys(list(pa) + list(pb))
    A, B = ip[: len(pa)], ip[len(pa) :]
    return any(polygon_intersects_int(a, b) for a in A for b in B)


# ---- contains(polygon, polygon): the set statement -------------------------------------------------------------------------------


def _edges(rings):
    """non-degenerate edges of closed integer rings, as (p, q) int pairs"""
    out = []
    for r in rings:
        for i in range(len(r) - 1):
            p, q = (int(r[i, 0]), int(r[i, 1])), (int(r[i + 1, 0]), int(r[i + 1, 1]))
            if p != q:
                out.append((p, q))
    return out


def _pieces(ring, others):
    """midpoints (Fractions) of the pieces into which the edges of `others` cut the edges of `ring` (only edge pairs whose exact
    boxes meet are split)"""
    oe = _edges(others)
    if oe:
        olo = np.array([[min(p[0], q[0]), min(p[1], q[1])] for p, q in oe], dtype=object)
        ohi = np.array([[max(p[0], q[0]), max(p[1], q[1])] for p, q in oe], dtype=object)
    out = []
    for p, q in _edges([ring]):
        d = (q[0] - p[0], q[1] - p[1])
        ts = {Fraction(0), Fraction(1)}
        if oe:
            lo, hi = (min(p[0], q[0]), min(p[1], q[1])), (max(p[0], q[0]), max(p[1], q[1]))
            near = np.nonzero((olo[:, 0] <= hi[0]) & (ohi[:, 0] >= lo[0]) & (olo[:, 1] <= hi[1]) & (ohi[:, 1] >= lo[1]))[0]
            for k in near:
                a, b = oe[k]
                e = (b[0] - a[0], b[1] - a[1])
                ap = (a[0] - p[0], a[1] - p[1])
                den = d[0] * e[1] - d[1] * e[0]
                if den != 0:
                    t, u = Fraction(ap[0] * e[1] - ap[1] * e[0], den), Fraction(ap[0] * d[1] - ap[1] * d[0], den)
                    if 0 <= t <= 1 and 0 <= u <= 1:
                        ts.add(t)
                elif ap[0] * d[1] - ap[1] * d[0] == 0:
                    dd = d[0] * d[0] + d[1] * d[1]
                    for c in (a, b):
                        t = Fraction((c[0] - p[0]) * d[0] + (c[1] - p[1]) * d[1], dd)
                        if 0 <= t <= 1:
                            ts.add(t)
        ts = sorted(ts)
        for t0, t1 in zip(ts, ts[1:]):
            t = (t0 + t1) / 2
            out.append((p[0] + t * d[0], p[1] + t * d[1]))
    return out


def _rational_pos(mids, rings):
    """polygon positions of rational points: every point and the rings are brought to one integer grid"""
    if not mids:
        return np.zeros(0, dtype=np.int64)
    den = math.lcm(*[Fraction(v).denominator for m in mids for v in m])
    X = np.array([int(Fraction(x) * den) for x, _ in mids], dtype=object)
    Y = np.array([int(Fraction(y) * den) for _, y in mids], dtype=object)
    R = [np.asarray(r, dtype=object) * den for r in rings]
    return polygon_pos(X, Y, R)


def polygon_contains_int(A, B):
    """B (non-empty, closed rings) is a subset of A (both closed sets), on integer rings"""
    if not A or not B or len(A[0]) == 0 or len(B[0]) == 0:
        return False
    for ring in B:
        if (polygon_pos(ring[:, 0], ring[:, 1], A) == OUTSIDE).any():
            return False
        if (_rational_pos(_pieces(ring, A), A) == OUTSIDE).any():
            return False
    for hole in A[1:]:
        mids = _pieces(hole, B)
        pos = _rational_pos(mids, B)
        if (pos == INSIDE).any():
            return False  # a piece of the hole's boundary in B's interior: B covers points of the hole
        if len(mids) and (pos == BOUNDARY).all() and (_rational_pos(mids, B[:1]) == BOUNDARY).all():
            return False  # the hole is B's exterior: B fills it
    return True


def contains(pa, pb) -> bool:
    """contains(A, B) of two geometries (lists of polygons of float rings, valid): B not empty and every member of B held by
    one member of A (the members of a valid multipolygon meet in points at most, so no polygon of B spans two of them)"""
    if not pb or not pa:
        return False
    ip, _ = _int_polys(list(pa) + list(pb))
    A, B = ip[: len(pa)], ip[len(pa) :]
    return all(any(polygon_contains_int(a, b) for a in A) for b in B)


# ---- the kernels' choices, restated -----------------------------------------------------------------------------------------------

PP_SMALL = 66  # gpk_polypoly.h: single-ring POLYGON pairs of 1 .. PP_SMALL coordinates take polygon_pair_small
PP_LIST = 32  # gpk_polypoly.h: in-window segment list of the general routine
JOIN_GS = 16  # lanes per candidate pair of the refine
CAND_STAGE = 16  # gpk_bboxjoin.hip: rows of at most this many candidates keep a staged slice
CAND_INLINE_SORT = 48  # gpk_bboxjoin.hip: beyond it the join takes bbox_cand_kernel<true> and the segmented sort


def pick_group_rows(n_coords: int, n_geoms: int) -> int:
    """lanes per row of point_poly_predicate_kernel<G> (gpk_distance.h pick_group_rows, not rounded): the first G of 1, 2, ..,
    64 with 32 G > mean coordinates a row (empty and null rows count)"""
    mean = n_coords / n_geoms if n_geoms > 0 else 1.0
    G = 1
    while G < 64 and G * 2 * 8 <= mean:
        G <<= 1
    return G


def small_form(na_rings: int, na: int, nb_rings: int, nb: int) -> bool:
    """pair_refine_kernel's choice of polygon_pair_small for a POLYGON x POLYGON candidate"""
    return na_rings == 1 and nb_rings == 1 and 1 <= na <= PP_SMALL and 1 <= nb <= PP_SMALL


def refine_per(n_cand: int, cu_count: int) -> int:
    """candidates per 16-lane group of pair_refine_kernel: blocks = ceil(n_cand / 16) capped at cu_count * 64"""
    blocks = min((n_cand + 256 // JOIN_GS - 1) // (256 // JOIN_GS), cu_count * 64)
    groups = blocks * (256 // JOIN_GS)
    return (n_cand + groups - 1) // groups


def cand_regime(max_count: int) -> str:
    return "staged" if max_count <= CAND_STAGE else ("compact" if max_count <= CAND_INLINE_SORT else "sorted")


def box_candidates(left_boxes, right_boxes):
    """per left row the right rows whose closed boxes meet its box ((n, 4) xmin, ymin, xmax, ymax; NaN rows never meet)"""
    L, R = np.asarray(left_boxes), np.asarray(right_boxes)
    with np.errstate(invalid="ignore"):
        m = (L[:, None, 0] <= R[None, :, 2]) & (R[None, :, 0] <= L[:, None, 2]) & (L[:, None, 1] <= R[None, :, 3]) & (R[None, :, 1] <= L[:, None, 3])
    return [np.flatnonzero(row) for row in m]


def geom_box(polys):
    """box of a geometry's exterior rings (NaN for an empty one)"""
    ext = [np.asarray(p[0], dtype=np.float64).reshape(-1, 2) for p in polys if p and len(p[0])]
    if not ext:
        return np.full(4, np.nan)
    c = np.concatenate(ext)
    return np.array([c[:, 0].min(), c[:, 1].min(), c[:, 0].max(), c[:, 1].max()])


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
# Every fixture lies on a dyadic lattice (multiples of 1/16, at most 24 significant bits), so the exact tests run in int64; the
# points one ulp off a vertex or an edge take the Python-integer path.

S = 1.0 / 16


def lat(v):
    return np.round(np.asarray(v, dtype=np.float64) / S) * S


def star_ring(cx, cy, R, n, rng, cw=False, dup=False):
    """closed lattice ring of n coordinates (n - 1 edges) around (cx, cy), radii alternating R and 0.55 R: rounding to the
    lattice may repeat a vertex; `dup` repeats one more on purpose (a zero-length edge).  n = 1: the centre alone; n = 2: an
    open two-coordinate ring; n = 3: a closed degenerate ring (p, q, p)."""
    if n == 1:
        return lat([[cx, cy]])
    if n == 2:
        return lat([[cx - R, cy - 0.3 * R], [cx + 0.7 * R, cy + R]])
    if n == 3:
        r = lat([[cx - R, cy], [cx + R, cy + 0.5 * R]])
        return np.concatenate([r, r[:1]])
    k = n - 1 - (1 if dup else 0)
    t = 2 * np.pi * (np.arange(k) + rng.uniform(0.0, 0.3, k)) / k
    if cw:
        t = -t
    r = R * np.where(np.arange(k) % 2 == 0, 1.0, 0.55 if k > 3 else 1.0)
    xy = lat(np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], axis=1))
    if dup:
        j = k // 2
        xy = np.concatenate([xy[: j + 1], xy[j : j + 1], xy[j + 1 :]])
    return np.concatenate([xy, xy[:1]])


def _sizes_for(G, k, rng):
    """a coordinate count n near k whose n - 1 edges are 0, 1 or G - 1 modulo G"""
    base = max(G, (k // G) * G)
    return [base + 1 + r for r in ((0, 1, G - 1) if G > 1 else (0,))][int(rng.integers(0, 3 if G > 1 else 1))]


def point_poly_rows(kind: int, G: int, seed: int = 0):
    """(rows, validity) of a polygonal column whose mean coordinates a row select G (pick_group_rows): a few long rows (ring
    edge counts 0, 1 and G - 1 modulo G, holes, repeated vertices) among rows of 4 coordinates, two empty rows, two null rows
    (coordinates kept).  MULTIPOLYGON long rows have two or three members, the first one short."""
    rng = np.random.default_rng(100 * G + kind + seed)
    n_rows = 48
    n_long = 8 if G >= 2 else 24
    target = 12 * G if G >= 2 else 9  # mean coordinates a row: well inside [8 G, 16 G), the band of G
    per_long = max(6, (target * n_rows - 4 * (n_rows - n_long)) // n_long)
    rows = []
    for i in range(n_rows):
        cx, cy = 256.0 * (i % 8) + 128.0, 256.0 * (i // 8) + 128.0
        if i in (5, 29):
            rows.append([])
            continue
        if i % (n_rows // n_long) == 0:
            members = 1 if kind == _abi.GEOM_POLYGON else 2 + (i % 3 == 0)
            budget = per_long
            polys = []
            for m in range(members):
                ox = cx + 70.0 * m - (35.0 if members > 1 else 0.0)
                R = 60.0 if members == 1 else 30.0
                share = budget if m == members - 1 else (4 if m == 0 else budget // 2)
                budget -= share
                n_h = _sizes_for(G, max(4, share // 5), rng) if share >= 24 else 0
                n_e = _sizes_for(G, max(4, share - n_h), rng) if G > 1 else max(4, share - n_h)
                rings = [star_ring(ox, cy, R, n_e, rng, dup=(i % 3 == 1))]
                if n_h:
                    rings.append(star_ring(ox, cy, 0.25 * R, n_h, rng, cw=True))
                polys.append(rings)
        else:
            polys = [[star_ring(cx, cy, 20.0, 4, rng)]]
        rows.append(polys[0] if kind == _abi.GEOM_POLYGON else polys)
    validity = [i not in (11, 40) for i in range(n_rows)]
    return rows, validity


def row_members(kind: int, row):
    """a polygonal row as a list of polygons"""
    if kind == _abi.GEOM_POLYGON:
        return [row] if len(row) else []
    return row


def _ulps(p):
    x, y = p
    return [(np.nextafter(x, np.inf), y), (np.nextafter(x, -np.inf), y), (x, np.nextafter(y, np.inf)), (x, np.nextafter(y, -np.inf))]


def probes(kind: int, row, rng):
    """query points for one row: a vertex, an edge's midpoint (an exact lattice point), a hole's vertex and edge midpoint, a point
    inside a hole, one inside the polygon, one far outside, and one ulp off the vertex and the midpoints in x and y"""
    polys = row_members(kind, row)
    if not polys:
        return [(64.0, 64.0)]
    out = []
    for rings in polys:
        ext = rings[0]
        j = int(rng.integers(0, len(ext) - 1)) if len(ext) > 1 else 0
        v = tuple(ext[j])
        m = tuple((ext[j] + ext[min(j + 1, len(ext) - 1)]) / 2)
        out += [v, m] + _ulps(v) + _ulps(m)
        c = ext[:-1].mean(axis=0) if len(ext) > 1 else ext[0]
        out += [tuple(lat(c + [0.4 * (ext[0][0] - c[0]), 0.0])), tuple(c + [1000.5, 3.0])]
        for h in rings[1:]:
            k = int(rng.integers(0, len(h) - 1))
            hv, hm = tuple(h[k]), tuple((h[k] + h[k + 1]) / 2)
            out += [hv, hm, tuple(lat(h[:-1].mean(axis=0)))] + _ulps(hv)[:2] + _ulps(hm)[2:]
    return [(float(x), float(y)) for x, y in out]


_CACHE = {}


def point_poly_fixture(kind: int, G: int):
    """dict: rows, validity, array, points ((n, 2): the probes of every row and a few NaN points), rows_of (the row each point is
    asked about), inside / not_outside (the exact answers: some member has the point inside / not outside; False for null and
    empty rows and NaN points); cached per process"""
    from tests.exact_ref import column

    key = ("pp", kind, G)
    if key in _CACHE:
        return _CACHE[key]
    rows, validity = point_poly_rows(kind, G)
    rng = np.random.default_rng(7 * G + kind)
    pts, rows_of, inside, touch = [], [], [], []
    for i, row in enumerate(rows):
        P = probes(kind, row, rng)
        if i % 9 == 4:
            P = P + [(np.nan, np.nan)]
        polys = row_members(kind, row)
        good = [p for p in P if not np.isnan(p[0])]
        pos = point_positions(good, polys) if polys and good else np.full((len(good), 0), OUTSIDE)
        k = 0
        for p in P:
            ok = validity[i] and not np.isnan(p[0]) and len(polys) > 0
            r = None
            if not np.isnan(p[0]):
                r = pos[k]
                k += 1
            pts.append(p)
            rows_of.append(i)
            inside.append(bool(ok and (r == INSIDE).any()))
            touch.append(bool(ok and (r != OUTSIDE).any()))
    fx = {"kind": kind, "rows": rows, "validity": validity, "array": column(kind, rows, validity), "points": np.array(pts, dtype=np.float64),
          "rows_of": np.array(rows_of, dtype=np.uint32), "inside": np.array(inside), "not_outside": np.array(touch)}
    _CACHE[key] = fx
    return fx


POINT_POLY_INSTANCES = [(k, g) for k in (_abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON) for g in (1, 2, 4, 8, 16, 32, 64)]


# ---- polygon x polygon intersects ---------------------------------------------------------------------------------------------------

RING_SIZES = (1, 2, 4, 65, 66, 67)
# rings of 1 - 3 coordinates and open rings are not valid polygons: their pairs are held to geo's algorithm (`intersects`), which
# on valid pairs is the closed-set statement (test_exact_predicate_ref.py checks both on the valid ones)
INVALID_SIZES = (1, 2)


def _comb(n, k_cross, lift, left_leg=True):
    """(A, B): two rings of about n coordinates whose boundaries run side by side (A's bottom at y = 1/2, B's top at y = 1/4, one
    vertex every unit) inside each other's box, so that every one of those segments is in the other's window; B's top vertex
    k_cross (None: none) is lifted to y = 1/4 + lift (3/4: it crosses A's bottom; 1/4: it touches it; 1/4 - 1 ulp: it does not)"""
    xs = np.arange(n, dtype=np.float64)
    a = [(-1.0, 10.0), (-1.0, -10.0), (-0.5, -10.0), (-0.5, 0.5)] + [(x, 0.5) for x in xs] + [(n - 1.0, 10.0), (-1.0, 10.0)]
    top = [[x, 0.25] for x in xs]
    if k_cross is not None:
        top[k_cross][1] = 0.25 + lift
    b = [tuple(t) for t in top] + [(n - 0.5, 0.25), (n - 0.5, 20.0), (n, 20.0), (n, -5.0), (0.0, -5.0), (0.0, 0.25)]
    return [np.array(a)], [np.array(b)]


def intersects_pairs(seed=11):
    """list of (name, A, B) POLYGON pairs ([exterior, hole...] float rings)"""
    rng = np.random.default_rng(seed)
    out = []
    for na in RING_SIZES:
        for nb in RING_SIZES:
            A = [star_ring(0.0, 0.0, 20.0, na, rng)]
            va = A[0][min(3, len(A[0]) - 1)]
            for name, (ox, oy, R) in {"nested": (0.0, 0.0, 6.0), "crossing": (18.0, 2.0, 10.0), "apart": (30.0, 30.0, 8.0),
                                      "box_only": (19.0, 19.0, 6.0)}.items():
                out.append((f"{na}x{nb}:{name}", A, [star_ring(ox, oy, R, nb, rng)]))
            # B's third vertex (or only one) on A's fourth vertex
            B = [star_ring(va[0] + 4.0, va[1] + 4.0, 6.0, nb, rng)]
            B[0] = B[0] + (va - B[0][min(2, len(B[0]) - 1)])
            out.append((f"{na}x{nb}:vertex_on_vertex", A, B))
            if na >= 4:  # B's only / first vertex on the middle of an edge of A (geo: a one-coordinate ring there is disjoint)
                m = (A[0][1] + A[0][2]) / 2
                out.append((f"{na}x{nb}:on_edge", A, [star_ring(m[0], m[1], 4.0, nb, rng) - (star_ring(m[0], m[1], 4.0, nb, rng)[0] - m) if nb > 1 else lat([m])]))
    n = 120
    for kc, where in ((None, "none"), (40, "second_chunk"), (n - 3, "last_chunk")):
        for lift, how in ((0.5, "cross"), (0.25, "touch"), (0.25 - 2.0**-54, "ulp_below")):
            if kc is None and how != "cross":
                continue
            A, B = _comb(n, kc, lift)
            out.append((f"comb:{where}:{how}", A, B))
            out.append((f"comb:{where}:{how}:swapped", B, A))
    big = [star_ring(0.0, 0.0, 40.0, 81, rng), star_ring(0.0, 0.0, 12.0, 41, rng, cw=True)]
    out += [("in_polygon", big, [star_ring(25.0, 0.0, 3.0, 9, rng)]), ("in_hole", big, [star_ring(0.0, 0.0, 3.0, 9, rng)]),
            ("around", [star_ring(0.0, 0.0, 3.0, 9, rng)], big), ("hole_around", [star_ring(0.0, 0.0, 3.0, 70, rng)], big)]
    sq = np.array([(0.0, 0.0), (8.0, 0.0), (8.0, 8.0), (0.0, 8.0), (0.0, 0.0)])
    dia = np.array([(12.0, 4.0), (10.0, 6.0), (8.0, 8.0), (10.0, 10.0), (12.0, 4.0)])  # a vertex on the square's corner
    out += [("corner", [sq], [dia]), ("box_edge_outside", [sq], [dia + [0.0, 1.0]]), ("empty_ext_with_hole", [np.zeros((0, 2)), sq * 0.5], [sq]),
            ("hole_poking_out", [sq, np.array([(6.0, 6.0), (6.0, 12.0), (7.0, 12.0), (7.0, 6.0), (6.0, 6.0)])], [sq + [0.0, 10.0]])]
    return out


def polygon_multi_pairs(seed=12):
    """list of (name, A POLYGON, B MULTIPOLYGON): members with holes, one member inside A's hole, one crossing A, ..."""
    rng = np.random.default_rng(seed)
    A = [star_ring(0.0, 0.0, 40.0, 70, rng), star_ring(0.0, 0.0, 12.0, 20, rng, cw=True)]
    far = [star_ring(200.0, 0.0, 10.0, 30, rng), star_ring(200.0, 0.0, 3.0, 9, rng, cw=True)]
    return [("in_hole_and_far", A, [[star_ring(0.0, 0.0, 4.0, 12, rng)], far]),
            ("crossing_member", A, [far, [star_ring(40.0, 0.0, 8.0, 40, rng), star_ring(40.0, 0.0, 2.0, 5, rng, cw=True)]]),
            ("member_inside", A, [far, [star_ring(25.0, 5.0, 3.0, 67, rng)]]),
            ("all_far", A, [far, [star_ring(0.0, 200.0, 10.0, 66, rng)]]),
            ("member_around", [star_ring(0.0, 0.0, 3.0, 9, rng)], [[star_ring(0.0, 0.0, 40.0, 90, rng)], far]),
            ("member_hole_around", [star_ring(0.0, 0.0, 3.0, 9, rng)], [far, [star_ring(0.0, 0.0, 40.0, 90, rng), star_ring(0.0, 0.0, 10.0, 30, rng, cw=True)]])]


# ---- the polygon join at scale: tiled template blocks ------------------------------------------------------------------------------

BLOCK = 256.0  # tile pitch: a block's polygons fit in [0, 96)^2, so no box meets a box of another tile


def join_template(seed: int):
    """(left rows, right rows) of one block: single-ring POLYGONs on the lattice.  Left rows of 20 - 60 coordinates; right rows
    alternate small-form (9 - 60 coordinates) and general-form (67 - 90) by id, so one left row's run of candidates switches
    forms and back.  Two nested pairs per block (no boundary contact: containment decides, on rings longer than two 16-lane
    strides)."""
    rng = np.random.default_rng(seed)
    left, right = [], []
    for i in range(10):
        c = rng.uniform(16.0, 80.0, 2)
        left.append([star_ring(c[0], c[1], float(rng.uniform(6.0, 14.0)), int(rng.integers(20, 61)), rng)])
    for j in range(12):
        c = rng.uniform(16.0, 80.0, 2)
        n = int(rng.integers(9, 61)) if j % 2 == 0 else int(rng.integers(67, 91))
        right.append([star_ring(c[0], c[1], float(rng.uniform(5.0, 12.0)), n, rng)])
    for k in range(2):  # nested: a 40-coordinate ring well inside a bigger one's inner radius, both orders
        c = rng.uniform(30.0, 66.0, 2)
        big, small = star_ring(c[0], c[1], 14.0, 70, rng), star_ring(c[0], c[1], 4.0, 40, rng)
        left.append([small] if k == 0 else [big])
        right.append([big] if k == 0 else [small])
    return left, right


def template_answers(left, right):
    """(candidates per left row: right ids whose closed boxes meet, exact intersects per candidate)"""
    cands = box_candidates([geom_box([l]) for l in left], [geom_box([r]) for r in right])
    return cands, [np.array([intersects([left[i]], [right[j]]) for j in c], dtype=bool) for i, c in enumerate(cands)]


def join_templates(k=4, max_count=CAND_STAGE):
    """k template blocks whose left rows have at most max_count candidates each (seeds taken in order until k qualify)"""
    out, seed = [], 0
    while len(out) < k:
        left, right = join_template(seed)
        cands, hits = template_answers(left, right)
        if max(len(c) for c in cands) <= max_count and sum(len(c) for c in cands) >= 40:
            out.append((left, right, cands, hits))
        seed += 1
    return out


def _flat(rows):
    """POLYGON rows -> (xy, geom_offsets, ring_offsets)"""
    rings = [r for row in rows for r in row]
    goff = np.concatenate([[0], np.cumsum([len(row) for row in rows])]).astype(np.int32)
    roff = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
    return np.concatenate(rings), goff, roff


def tiled_join(templates, n_tiles: int, hole_row: bool = False):
    """(left GeoArrowArray, right GeoArrowArray, expected pairs (P, 2) sorted by (l, r), expected counts, candidate counts): the
    templates tiled n_tiles times (tile t takes template t % k) at exact translations by multiples of BLOCK.  hole_row: left row
    3 and right row 5 of tile 0 get a small hole at their first vertex's side (single-ring columns no longer)."""
    from geopolars_amd.geoarrow import GeoArrowArray

    k = len(templates)
    side = int(np.ceil(np.sqrt(n_tiles)))
    cols = {}
    for s, which in ((0, "left"), (1, "right")):
        per = [t[s] for t in templates]
        if hole_row:
            per = [list(p) for p in per]
            i = 3 if s == 0 else 5
            ring = per[0][i][0]
            c = lat(ring[:-1].mean(axis=0))
            per[0][i] = [ring, np.array([c, c + [0.0, 0.5], c + [0.5, 0.5], c + [0.5, 0.0], c])]
        flats = [_flat(p) for p in per]
        xys, goffs, roffs, cnt = [], [], [], []
        g_base, r_base, c_base = 0, 0, 0
        for t in range(n_tiles):
            xy, goff, roff = flats[t % k] if t == 0 or t % k else _flat(templates[0][s])
            off = np.array([BLOCK * (t % side), BLOCK * (t // side)])
            xys.append(xy + off)
            goffs.append(goff[1:] + r_base)
            roffs.append(roff[1:] + c_base)
            r_base += len(roff) - 1
            c_base += len(xy)
        xy = np.concatenate(xys)
        goff = np.concatenate([[0], np.concatenate(goffs)]).astype(np.int32)
        roff = np.concatenate([[0], np.concatenate(roffs)]).astype(np.int32)
        cols[which] = GeoArrowArray(_abi.GEOM_POLYGON, xy, geom_offsets=goff, ring_offsets=roff)
    # expected answers: per tile the template's (tile 0 recomputed when it carries the holes)
    base = list(templates)
    if hole_row:  # tile 0 as it was built, read back from the columns
        from tests.exact_ref import polygon_geoms

        l0 = [g[0] for g in polygon_geoms(cols["left"])[: len(templates[0][0])]]
        r0 = [g[0] for g in polygon_geoms(cols["right"])[: len(templates[0][1])]]
        base[0] = (l0, r0) + template_answers(l0, r0)
    pairs, counts, ccounts = [], [], []
    nl = [len(t[0]) for t in templates]
    nr = [len(t[1]) for t in templates]
    l_base = r_base = 0
    for t in range(n_tiles):
        tpl = base[0] if (hole_row and t == 0) else templates[t % k]
        for i, (c, h) in enumerate(zip(tpl[2], tpl[3])):
            js = c[h] + r_base
            pairs.append(np.stack([np.full(len(js), l_base + i), js], axis=1))
            counts.append(len(js))
            ccounts.append(len(c))
        l_base += nl[t % k]
        r_base += nr[t % k]
    return cols["left"], cols["right"], np.concatenate(pairs).astype(np.uint32), np.array(counts, dtype=np.uint32), np.array(ccounts)


def regime_join(counts=(16, 17, 48, 49)):
    """(left rows, right rows): right rows are 1 x 1 squares at x = 2 j; left row r is a thin rectangle whose box meets exactly
    counts[r] of them (its top edge runs through every second square: half the candidates intersect)"""
    n_right = max(counts) + 2
    right = [[np.array([(2.0 * j, 0.0), (2.0 * j + 1, 0.0), (2.0 * j + 1, 1.0), (2.0 * j, 1.0), (2.0 * j, 0.0)]) + [0.0, 4.0 * (j % 2)]] for j in range(n_right)]
    left = []
    for c in counts:
        x1 = 2.0 * (c - 1) + 0.5
        left.append([np.array([(0.25, 0.5), (x1, 0.5), (x1, 4.5), (0.25, 4.5), (0.25, 0.5)])])
    return left, right


# ---- contains / within ------------------------------------------------------------------------------------------------------------


def rect_ring(x0, y0, x1, y1, m, cw=False):
    """closed axis-parallel rectangle with m vertices per side (4 m + 1 coordinates, collinear vertices along every side)"""
    xs, ys = np.linspace(x0, x1, m + 1), np.linspace(y0, y1, m + 1)
    r = [(x, y0) for x in xs[:-1]] + [(x1, y) for y in ys[:-1]] + [(x, y1) for x in xs[::-1][:-1]] + [(x0, y) for y in ys[::-1][:-1]]
    r = lat(np.array(r + r[:1]))
    return r[::-1] if cw else r


def contains_pairs():
    """list of (name, A geometry, B geometry) — geometries as lists of polygons — with rings of 33 to 200 coordinates: B equal to A,
    B equal to A's hole, B touching A's exterior from inside, B touching A's hole from outside, B around A's hole, B crossing the
    hole, multipolygon members"""
    A = [rect_ring(0, 0, 64, 64, 50), rect_ring(24, 24, 40, 40, 8, cw=True)]  # 201 and 33 coordinates
    hole = A[1][::-1]
    cases = [
        ("equal", [A], [A]),
        ("equal_exterior", [A], [[A[0]]]),
        ("is_the_hole", [A], [[hole]]),
        ("touch_exterior_inside", [A], [[rect_ring(0, 0, 16, 20, 10)]]),
        ("touch_hole_outside", [A], [[rect_ring(8, 24, 24, 40, 12)]]),
        ("across_hole", [A], [[rect_ring(20, 20, 30, 30, 9)]]),
        ("around_hole", [A], [[rect_ring(16, 16, 48, 48, 12)]]),
        ("around_hole_with_it", [A], [[rect_ring(16, 16, 48, 48, 12), hole]]),
        ("around_hole_bigger_hole", [A], [[rect_ring(16, 16, 48, 48, 12), rect_ring(20, 20, 44, 44, 9, cw=True)]]),
        ("pokes_out", [A], [[rect_ring(48, 48, 72, 60, 10)]]),
        ("outside_shares_edge", [A], [[rect_ring(64, 0, 80, 64, 10)]]),
        ("inside_member_2", [A, [rect_ring(100, 0, 160, 60, 40)]], [[rect_ring(110, 10, 160, 30, 20)]]),
        ("spans_members", [A, [rect_ring(72, 0, 128, 64, 40)]], [[rect_ring(48, 8, 80, 16, 12)]]),
        ("member_hole", [[rect_ring(-80, 0, -16, 64, 30)], A], [[rect_ring(26, 26, 38, 38, 9)]]),
    ]
    return cases
