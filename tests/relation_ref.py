"""Exact reference of the line x polygon relation mask (gpk_line_polygon_relation, csrc/gpk_linearea.h) and its fixtures.

The mask of a line L (the closed set of its segments and coordinates) against a polygonal geometry P: bit 1 — L has a point in P's
interior, 2 — on a ring of P, 4 — outside every part or strictly inside a hole.  Brute force over rationals: every segment of L is
cut at every exact intersection parameter with every ring edge (the end points of collinear overlaps are cuts); every coordinate,
every cut point and every midpoint between two consecutive cuts is classified by its even-odd position against every ring
(tests/exact_predicates.py: polygon_pos on one integer grid).  Between two consecutive cuts a segment meets no ring, so its midpoint
speaks for the whole piece.  All fixtures live on small integer lattices: the arithmetic is exact and fast.

Rows are what tests/exact_ref.column takes: a LINESTRING row is a list of (x, y), a MULTILINESTRING row a list of such lists, a POLYGON
row a list of rings, a MULTIPOLYGON row a list of polygons."""
from __future__ import annotations

from fractions import Fraction
from functools import lru_cache

import numpy as np

from geopolars_amd import _abi
from tests import exact_predicates as E

LS, MLS, PG, MPG = _abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON
INTERIOR, BOUNDARY, EXTERIOR = 1, 2, 4
FAMILIES = [(LS, PG), (LS, MPG), (MLS, PG), (MLS, MPG)]
NAMES = {LS: "ls", MLS: "mls", PG: "pg", MPG: "mpg"}

# the predicates over the mask, as include/geopolars_hip.h states them (ids: GPK_LP_PRED_*)
PREDICATES = {
    "intersects": lambda m: (m & 3) != 0,
    "within": lambda m: bool(m & 1) and not (m & 4),
    "covered_by": lambda m: m != 0 and not (m & 4),
    "crosses": lambda m: bool(m & 1) and bool(m & 4),
    "touches": lambda m: bool(m & 2) and not (m & 1),
    "disjoint": lambda m: m == 4,
}
PRED_IDS = {"intersects": 0, "within": 1, "covered_by": 2, "crosses": 3, "touches": 4}


def line_seqs(kind, row):
    return [list(row)] if kind == LS else [list(s) for s in row]


def row_polys(kind, row):
    """the non-empty members of a polygonal row (a member without rings or with an empty shell adds nothing)"""
    polys = [row] if kind == PG else list(row)
    return [[r for k, r in enumerate(p) if k == 0 or len(r)] for p in polys if len(p) and len(p[0])]


def _ring_usable(r) -> bool:
    """cont::ring_init: closed, at least 4 coordinates, no NaN, a turning extreme vertex"""
    a = np.asarray(r, dtype=np.float64).reshape(-1, 2)
    if len(a) < 4 or np.isnan(a).any() or not (a[0] == a[-1]).all():
        return False
    v = a[:-1]
    k = int(np.lexsort((v[:, 1], v[:, 0]))[0])
    m = len(v)
    p = next((v[(k - j) % m] for j in range(1, m) if (v[(k - j) % m] != v[k]).any()), None)
    q = next((v[(k + j) % m] for j in range(1, m) if (v[(k + j) % m] != v[k]).any()), None)
    if p is None or q is None:
        return False
    if any(abs(c) >= 2.0**26 for c in a.ravel()) and all(isinstance(c, int) for pt in r for c in pt):
        # wide Python ints (rows of arbitrary doubles on one integer grid, tests/hard_orient.on_integer_grid): the doubles above round
        # them, and the kernel's turn is exact — the same rule on the ints themselves
        w = [(int(x), int(y)) for x, y in r][:-1]
        if w[0] != (int(r[-1][0]), int(r[-1][1])):
            return False
        k = min(range(m), key=lambda i: (w[i][0], w[i][1], i))
        p = next((w[(k - j) % m] for j in range(1, m) if w[(k - j) % m] != w[k]), None)
        q = next((w[(k + j) % m] for j in range(1, m) if w[(k + j) % m] != w[k]), None)
        if p is None or q is None:
            return False
        return (p[0] - w[k][0]) * (q[1] - w[k][1]) != (p[1] - w[k][1]) * (q[0] - w[k][0])
    return (p[0] - v[k][0]) * (q[1] - v[k][1]) != (p[1] - v[k][1]) * (q[0] - v[k][0])


def _int_ring(r):
    """integer coordinates as int64; Python ints that a double cannot hold stay Python ints (object dtype): that is how rows of
    arbitrary doubles arrive, brought to one integer grid by an exact power of two (tests/hard_orient.on_integer_grid)"""
    flat = [v for p in r for v in p]
    if flat and all(isinstance(v, int) for v in flat) and max(abs(v) for v in flat) >= 2**53:
        return np.array([[int(x), int(y)] for x, y in r], dtype=object).reshape(-1, 2)
    a = np.asarray(r, dtype=np.float64).reshape(-1, 2)
    assert (a == np.round(a)).all(), "the reference works on integer coordinates"
    return a.astype(np.int64)


def _cuts(p, q, edges, elo, ehi):
    """the cut parameters (Fractions, sorted, 0 and 1 included) of segment pq (p != q, int pairs) with the ring edges"""
    d = (q[0] - p[0], q[1] - p[1])
    ts = {Fraction(0), Fraction(1)}
    if len(edges):
        lo, hi = (min(p[0], q[0]), min(p[1], q[1])), (max(p[0], q[0]), max(p[1], q[1]))
        near = np.nonzero((elo[:, 0] <= hi[0]) & (ehi[:, 0] >= lo[0]) & (elo[:, 1] <= hi[1]) & (ehi[:, 1] >= lo[1]))[0]
        for k in near:
            a, b = edges[k]
            e = (b[0] - a[0], b[1] - a[1])
            ap = (a[0] - p[0], a[1] - p[1])
            den = d[0] * e[1] - d[1] * e[0]
            if den != 0:
                t, u = Fraction(ap[0] * e[1] - ap[1] * e[0], den), Fraction(ap[0] * d[1] - ap[1] * d[0], den)
                if 0 <= t <= 1 and 0 <= u <= 1:
                    ts.add(t)
            elif ap[0] * d[1] - ap[1] * d[0] == 0:  # collinear: the ends of the overlap
                dd = d[0] * d[0] + d[1] * d[1]
                for c in (a, b):
                    t = Fraction((c[0] - p[0]) * d[0] + (c[1] - p[1]) * d[1], dd)
                    if 0 <= t <= 1:
                        ts.add(t)
    return sorted(ts)


def _positions(points, polys):
    """mask bits of rational points against integer polygons: on a ring of any member -> BOUNDARY, inside one -> INTERIOR"""
    pos = np.stack([E._rational_pos(points, rings) for rings in polys], axis=1)
    return np.where((pos == E.BOUNDARY).any(axis=1), BOUNDARY, np.where((pos == E.INSIDE).any(axis=1), INTERIOR, EXTERIOR))


def sample_points(seqs, polys):
    """every coordinate, cut point and piece midpoint of the line's sequences (integer) against the polygons' rings"""
    edges = E._edges([r for p in polys for r in p])
    dt = object if any(abs(v) >= 2**62 for e in edges for p in e for v in p) else np.int64
    elo = np.array([[min(a[0], b[0]), min(a[1], b[1])] for a, b in edges], dtype=dt).reshape(-1, 2)
    ehi = np.array([[max(a[0], b[0]), max(a[1], b[1])] for a, b in edges], dtype=dt).reshape(-1, 2)
    pts = []
    for s in seqs:
        c = [(int(x), int(y)) for x, y in s]
        pts.extend((Fraction(x), Fraction(y)) for x, y in c)
        for p, q in zip(c, c[1:]):
            if p == q:
                continue
            ts = _cuts(p, q, edges, elo, ehi)
            at = lambda t: (p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1]))  # noqa: E731
            pts.extend(at(t) for t in ts[1:-1])
            pts.extend(at((t0 + t1) / 2) for t0, t1 in zip(ts, ts[1:]))
    return pts


def mask(kl, line_row, kp, poly_row, line_valid=True, poly_valid=True) -> int:
    """the exact mask of one pair of rows, with the row rules of the header: 0 for an unusable row or an invalid ring"""
    if not line_valid or not poly_valid or line_row is None or poly_row is None:
        return 0
    seqs = [s for s in line_seqs(kl, line_row) if len(s)]
    if not seqs or any(np.isnan(np.asarray(s, dtype=np.float64)).any() for s in seqs):
        return 0
    polys = row_polys(kp, poly_row)
    if not polys or not all(_ring_usable(r) for p in polys for r in p):
        return 0
    ipolys = [[_int_ring(r) for r in p] for p in polys]
    iseqs = [_int_ring(s) for s in seqs]
    # (exact shortcut: a line whose box misses the box of the shells lies outside)
    lo = np.min([s.min(axis=0) for s in iseqs], axis=0)
    hi = np.max([s.max(axis=0) for s in iseqs], axis=0)
    plo = np.min([p[0].min(axis=0) for p in ipolys], axis=0)
    phi = np.max([p[0].max(axis=0) for p in ipolys], axis=0)
    if (hi < plo).any() or (phi < lo).any():
        return EXTERIOR
    return int(np.bitwise_or.reduce(_positions(sample_points(iseqs, ipolys), ipolys)))


def masks(kl, lines, kp, polys, rows=None, lv=None, pv=None):
    """row-wise masks; `rows`: the polygon row of every line row (out of range: 0)"""
    out = np.zeros(len(lines), dtype=np.uint8)
    for i, line in enumerate(lines):
        j = i if rows is None else int(rows[i])
        if j >= len(polys):
            continue
        out[i] = mask(kl, line, kp, polys[j], lv is None or bool(lv[i]), pv is None or bool(pv[j]))
    return out


# ---- validity of the fixture polygons, by the reference's own means ----------------------------------------------------------------


def _ring_simple(r) -> bool:
    """no two edges of the closed integer ring meet except neighbours at their shared vertex (zero-length edges dropped)"""
    v = [tuple(int(c) for c in x) for x in r[:-1]]
    v = [x for k, x in enumerate(v) if x != v[k - 1]]
    n = len(v)
    if n < 3 or len(set(v)) != n:
        return False
    a0 = np.array(v, dtype=np.int64)
    a1 = np.roll(a0, -1, axis=0)
    lo, hi = np.minimum(a0, a1), np.maximum(a0, a1)
    for i in range(n):
        p, q = a0[i], a1[i]
        o1 = E.orient(p[0], p[1], q[0], q[1], a0[:, 0], a0[:, 1])
        o2 = E.orient(p[0], p[1], q[0], q[1], a1[:, 0], a1[:, 1])
        o3 = E.orient(a0[:, 0], a0[:, 1], a1[:, 0], a1[:, 1], p[0], p[1])
        o4 = E.orient(a0[:, 0], a0[:, 1], a1[:, 0], a1[:, 1], q[0], q[1])
        box = (lo <= hi[i]).all(axis=1) & (hi >= lo[i]).all(axis=1)
        meet = box & (((o1 != o2) & (o3 != o4)) | ((o1 == 0) & (o2 == 0)))
        for j in np.nonzero(meet)[0]:
            if j == i:
                continue
            if j != (i + 1) % n and i != (j + 1) % n:
                return False
            # neighbours share a vertex: they may not fold back onto each other
            s, e, f = (a1[i], a0[i], a1[j]) if j == (i + 1) % n else (a0[i], a1[i], a0[j])
            if o1[j] == 0 and o2[j] == 0 and (e - s) @ (f - s) > 0:
                return False
    return True


def polygon_valid(kp, poly_row) -> bool:
    """OGC validity as far as the mask's contract needs it: simple rings; no piece of a ring on, inside a hole of, or outside the
    shell of its own polygon, or on or inside another member — so rings meet each other in single points at most, holes lie inside
    their shell and members do not overlap"""
    polys = [[_int_ring(r) for r in p] for p in row_polys(kp, poly_row)]
    if not polys:
        return False
    if not all(_ring_usable(r) and _ring_simple(r) for p in polys for r in p):
        return False
    for a, pa in enumerate(polys):
        for k, ring in enumerate(pa):
            others = [r for b, pb in enumerate(polys) for j, r in enumerate(pb) if (b, j) != (a, k)]
            mids = E._pieces(ring, others)
            for b, pb in enumerate(polys):
                if b != a:
                    if (E._rational_pos(mids, pb) != E.OUTSIDE).any():
                        return False
                    continue
                for j, r in enumerate(pb):
                    if j == k:
                        continue
                    want = E.INSIDE if j == 0 else E.OUTSIDE  # a hole inside the shell; the shell and the other holes outside a hole
                    if (E._rational_pos(mids, [r]) != want).any():
                        return False
    return True


# ---- known answers -------------------------------------------------------------------------------------------------------------------


def sq(x0, y0, x1, y1, cw=False):
    r = [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]
    return r[::-1] if cw else r


DONUT = [sq(0, 0, 12, 12), sq(4, 4, 8, 8, cw=True)]  # one polygon: shell and a hole
# (name, line as one sequence, mask)
KNOWN = [
    ("inside", [(1, 1), (3, 2)], 1),
    ("crossing", [(-2, 2), (2, 2)], 7),
    ("touching at an end point", [(-3, 5), (0, 5)], 6),
    ("along an edge", [(2, 0), (9, 0)], 2),
    ("through a shell vertex tangentially", [(-2, 2), (2, -2)], 6),
    ("through a shell vertex transversally", [(-2, -2), (3, 3)], 7),
    ("inside the hole", [(5, 5), (7, 6)], 4),
    ("along a hole edge", [(5, 4), (7, 4)], 2),
    ("one coordinate on a vertex", [(0, 0)], 2),
    ("from the interior to an edge", [(2, 2), (2, 0)], 3),
    ("across the hole", [(2, 6), (10, 6)], 7),
    ("from the hole onto its edge", [(6, 6), (6, 8)], 6),
    ("outside", [(20, 20), (30, 25), (20, 30)], 4),
    ("repeated coordinates inside", [(2, 2), (2, 2), (3, 2), (3, 2)], 1),
    ("one coordinate inside", [(1, 1)], 1),
    ("along the shell and round a corner", [(3, 0), (12, 0), (12, 7)], 2),
    ("in the interior and along an edge", [(2, 2), (0, 2), (0, 9)], 3),
]
KNOWN_MULTI = ("one member inside, one outside", [[(1, 1), (3, 2)], [(20, 20), (21, 25)]], 5)  # (a MULTILINESTRING only)


def known_columns(kl, kp):
    """(line rows, polygon rows, masks): the known answers in the four family combinations; a MULTIPOLYGON row adds a far second
    member and an empty one, a MULTILINESTRING row an empty member"""
    poly = DONUT if kp == PG else [[], DONUT, [sq(40, 40, 44, 44)]]
    lines, want = [], []
    for _, seq, m in KNOWN:
        lines.append(seq if kl == LS else [[], seq])
        want.append(m)
    if kl == MLS:
        lines.append(KNOWN_MULTI[1])
        want.append(KNOWN_MULTI[2])
    return lines, [poly] * len(lines), np.array(want, dtype=np.uint8)


# ---- ring-touch configurations ---------------------------------------------------------------------------------------------------------

# a hole vertex on a shell mid-edge: the hole's corner (6, 0) lies inside the shell edge (0, 0) - (12, 0)
HOLE_ON_SHELL = [[(0, 0), (12, 0), (12, 12), (0, 12), (0, 0)], [(6, 0), (3, 4), (9, 4), (6, 0)]]
# two holes sharing the vertex (8, 8)
TWO_HOLES = [sq(0, 0, 16, 16), [(8, 8), (3, 5), (3, 11), (8, 8)], [(8, 8), (13, 11), (13, 5), (8, 8)]]
# two members sharing the vertex (10, 5); a third whose corner (5, 10) lies inside the first member's edge (0, 10) - (10, 10)
PARTS = [[sq(0, 0, 10, 10)], [[(10, 5), (16, 2), (16, 8), (10, 5)]], [[(5, 10), (8, 15), (2, 15), (5, 10)]]]
# (name, polygon kind, polygon row, line, mask)
TIES = [
    ("hole-on-shell: transversally into the hole", PG, HOLE_ON_SHELL, [(6, -3), (6, 3)], 6),
    ("hole-on-shell: transversally into the interior", PG, HOLE_ON_SHELL, [(1, -1), (6, 0), (10, 2)], 7),
    ("hole-on-shell: interior through the contact into the interior", PG, HOLE_ON_SHELL, [(2, 2), (6, 0), (10, 2)], 3),
    ("hole-on-shell: tangentially along the shell", PG, HOLE_ON_SHELL, [(2, 0), (10, 0)], 2),
    ("hole-on-shell: tangentially outside", PG, HOLE_ON_SHELL, [(4, -2), (6, 0), (8, -2)], 6),
    ("hole-on-shell: ending there from outside", PG, HOLE_ON_SHELL, [(6, -4), (6, 0)], 6),
    ("hole-on-shell: ending there from the hole", PG, HOLE_ON_SHELL, [(6, 3), (6, 0)], 6),
    ("hole-on-shell: ending there from the interior", PG, HOLE_ON_SHELL, [(2, 1), (6, 0)], 3),
    ("hole-on-shell: one segment crossing the shell edge at the hole vertex into the hole", PG, HOLE_ON_SHELL, [(5, -3), (7, 3)], 6),
    ("hole-on-shell: one segment crossing the shell edge at the hole vertex into the interior", PG, HOLE_ON_SHELL, [(2, -1), (10, 1)], 7),
    ("hole-on-shell: a crossing of the shell edge away from the hole vertex", PG, HOLE_ON_SHELL, [(3, -3), (5, 3)], 7),
    ("two holes: hole to hole through the shared vertex", PG, TWO_HOLES, [(4, 8), (12, 8)], 6),
    ("two holes: hole to hole, a vertex at the contact", PG, TWO_HOLES, [(4, 7), (8, 8), (12, 9)], 6),
    ("two holes: interior to interior through the shared vertex", PG, TWO_HOLES, [(8, 3), (8, 13)], 3),
    ("two holes: hole to interior at the shared vertex", PG, TWO_HOLES, [(4, 8), (8, 8), (8, 12)], 7),
    ("two holes: ending there from the interior", PG, TWO_HOLES, [(8, 2), (8, 8)], 3),
    ("two holes: ending there from a hole", PG, TWO_HOLES, [(5, 8), (8, 8)], 6),
    ("two holes: along a hole edge into the shared vertex", PG, TWO_HOLES, [(3, 5), (8, 8), (13, 11)], 2),
    ("parts: part to part through the shared vertex", MPG, PARTS, [(7, 5), (13, 5)], 3),
    ("parts: part to part, a vertex at the contact", MPG, PARTS, [(7, 4), (10, 5), (14, 6)], 3),
    ("parts: tangentially through the shared vertex", MPG, PARTS, [(10, 2), (10, 8)], 2),
    ("parts: outside to outside through the shared vertex", MPG, PARTS, [(11, 1), (10, 5), (11, 9)], 6),
    ("parts: ending at the shared vertex from outside", MPG, PARTS, [(12, 0), (10, 5)], 6),
    ("parts: part to part through the vertex on the mid-edge", MPG, PARTS, [(5, 7), (5, 13)], 3),
    ("parts: one segment crossing the edge at the other part's vertex", MPG, PARTS, [(4, 8), (6, 12)], 3),
    ("parts: along the edge over the other part's vertex", MPG, PARTS, [(2, 10), (8, 10)], 2),
    ("parts: from the part out beside the other part's vertex", MPG, PARTS, [(5, 8), (5, 10), (9, 12)], 7),
]


def tie_columns(kl=LS, pad=0):
    """the tie rows as columns per polygon kind: {kp: (lines, polys, masks)}; `pad` collinear vertices are put into every ring edge
    (the answers do not change, the rows grow past the lane-group threshold)"""
    out = {}
    for kp in (PG, MPG):
        sel = [t for t in TIES if t[1] == kp]
        lines = [t[3] if kl == LS else [t[3], []] for t in sel]
        polys = [padded(kp, t[2], pad) for t in sel]
        out[kp] = (lines, polys, np.array([t[4] for t in sel], dtype=np.uint8))
    return out


def pad_ring(r, k):
    """k more vertices inside every edge of a ring, collinear and on the lattice: the coordinates are scaled by k + 1 first"""
    a = _int_ring(r) * (k + 1)
    out = []
    for p, q in zip(a[:-1], a[1:]):
        out.extend(tuple(int(c) for c in p + (q - p) * j // (k + 1)) for j in range(k + 1))
    out.append(tuple(int(c) for c in a[-1]))
    return out


def padded(kp, poly_row, k):
    if k == 0:
        return poly_row
    if kp == PG:
        return [pad_ring(r, k) if len(r) else r for r in poly_row]
    return [[pad_ring(r, k) if len(r) else r for r in p] for p in poly_row]


def scaled_line(kl, line_row, k):
    f = lambda s: [(x * (k + 1), y * (k + 1)) for x, y in s]  # noqa: E731
    return f(line_row) if kl == LS else [f(s) for s in line_row]


def placed(kind, row, offset, scale):
    """a row translated by an integer offset and then scaled by a power of two (exact in doubles)"""
    f = lambda s: [((x + offset[0]) * scale, (y + offset[1]) * scale) for x, y in s]  # noqa: E731
    if kind == LS:
        return f(row)
    if kind in (MLS, PG):
        return [f(s) for s in row]
    return [[f(s) for s in p] for p in row]


PLACEMENTS = [((500000, 4649776), 1.0), ((-20037508, 15538711), 1.0), ((3, -7), 2.0**-20), ((1 << 40, -(1 << 39)), 2.0**10)]

# ---- random lattice columns ----------------------------------------------------------------------------------------------------------


def star(cx, cy, R, n, rng, cw=False):
    """closed integer ring of n coordinates around (cx, cy), radii alternating R and about R / 2, by increasing angle"""
    k = n - 1
    t = 2 * np.pi * (np.arange(k) + rng.uniform(0.0, 0.4, k)) / k
    rad = R * np.where(np.arange(k) % 2 == 0, 1.0, 0.55 if k > 4 else 1.0)
    xy = np.round(np.stack([cx + rad * np.cos(t), cy + rad * np.sin(t)], axis=1)).astype(np.int64)
    ring = [tuple(int(c) for c in p) for p in xy]
    ring.append(ring[0])
    return ring[::-1] if cw else ring


def _random_polygon(cx, cy, R, n, holes, rng):
    """a valid star polygon of about n coordinates (rejection sampling against polygon_valid); holes need R >= 10, two holes R >= 16"""
    holes = min(holes, 2 if R >= 16 else (1 if R >= 10 else 0))
    for _ in range(200):
        n_h = [int(rng.integers(4, 7)) for _ in range(holes)]
        rings = [star(cx, cy, R, max(4, n - sum(n_h)), rng)]
        if holes == 1:
            rings.append(star(cx, cy, max(3, R // 4), n_h[0], rng, cw=True))
        elif holes == 2:
            rings.append(star(cx - 3 * R // 10, cy, 3, n_h[0], rng, cw=True))
            rings.append(star(cx + 3 * R // 10, cy, 3, n_h[1], rng, cw=True))
        if polygon_valid(PG, rings):
            return rings
    raise AssertionError(f"no valid polygon found (R = {R}, n = {n}, holes = {holes})")


def _random_seq(poly_rows, cx, cy, R, n, style, rng):
    """n lattice coordinates: style 0 — anywhere near the geometry, 1 — hugging its vertices, 2 — close to the centre, 3 — far away,
    4 — a walk in short steps, 5 — along one ring from vertex to vertex, 6 — from far away to a vertex, 7 — from the centre region
    to a vertex"""
    rings = [r for p in poly_rows for r in p]
    verts = [v for r in rings for v in r]
    near_centre = lambda: (int(cx + rng.integers(-1, 2)), int(cy + R // 2 + rng.integers(-1, 2)))  # noqa: E731
    far = lambda: (int(cx + 3 * R + rng.integers(0, R)), int(cy + 2 * R + rng.integers(0, R)))  # noqa: E731
    if style == 5:
        r = rings[int(rng.integers(0, len(rings)))]
        k = int(rng.integers(0, len(r) - 1))
        return [r[(k + j) % (len(r) - 1)] for j in range(min(n, len(r)))]
    if style in (6, 7):
        v = verts[int(rng.integers(0, len(verts)))]
        return ([far() for _ in range(n - 1)] + [v]) if style == 6 else ([near_centre() for _ in range(n - 1)] + [v])
    out = []
    x, y = int(cx + rng.integers(-R, R + 1)), int(cy + rng.integers(-R, R + 1))
    for _ in range(n):
        if style == 1 and rng.random() < 0.6:
            x, y = verts[int(rng.integers(0, len(verts)))]
        elif style == 2:
            x, y = near_centre()
        elif style == 3:
            x, y = far()
        elif style == 4:
            x, y = x + int(rng.integers(-3, 4)), y + int(rng.integers(-3, 4))
        else:
            x, y = int(cx + rng.integers(-R - 3, R + 4)), int(cy + rng.integers(-R - 3, R + 4))
        out.append((x, y))
    return out


@lru_cache(maxsize=None)
def random_columns(kl, kp, n_rows=96):
    """(line rows, polygon rows, masks) of lattice lines (2 - 40 coordinates) against lattice star polygons (4 - 70 coordinates, holes,
    multipolygons with empty members); small integers, so coincidences are frequent"""
    rng = np.random.default_rng(1000 + 10 * kl + kp)
    lines, polys = [], []
    for i in range(n_rows):
        n = int(rng.choice([4, 5, 8, 17, 33, 48, 70]))
        R = max(int(rng.integers(7, 22)), n // 2 + 4)  # (a ring of n distinct lattice vertices needs the room)
        holes = int(rng.integers(0, 3)) if n >= 17 else 0
        members = [_random_polygon(0, 0, R, n, holes, rng)]
        if kp == MPG:
            if i % 2:
                members.append(_random_polygon(3 * R, 0, R, int(rng.integers(4, 12)), 0, rng))
            if i % 3 == 0:
                members.insert(int(rng.integers(0, len(members) + 1)), [])
        style = i % 8
        n_l = int(rng.choice([2, 2, 3, 5, 9, 17, 40])) if style not in (2, 6, 7) else int(rng.integers(2, 4))
        seq = _random_seq(members, 0, 0, R, n_l, style, rng)
        if kl == LS:
            lines.append(seq)
        else:
            row = [seq]
            if i % 2 or style == 2:  # (a member near the centre with one far away: INTERIOR and EXTERIOR without BOUNDARY)
                row.append(_random_seq(members, 0, 0, R, int(rng.integers(1, 6)), 3 if style == 2 else int(rng.integers(0, 8)), rng))
            if i % 4 == 0:
                row.insert(int(rng.integers(0, len(row) + 1)), [])
            lines.append(row)
        polys.append(members[0] if kp == PG else members)
    return lines, polys, masks(kl, lines, kp, polys)


# ---- the join fixture ------------------------------------------------------------------------------------------------------------------


@lru_cache(maxsize=None)
def join_fixture(kl=LS, kp=PG, n=300):
    """about n short lines and n small polygons spread over a 600 x 600 lattice, plus one polygon that covers the whole domain (one
    row with hundreds of candidates whichever side it is on); a null row and an empty row on either side.
    Returns (lines, line validity, polys, polygon validity, table[n_lines, n_polys] of exact masks)."""
    rng = np.random.default_rng(77 + kl + kp)
    polys, lines = [], []
    for j in range(n):
        cx, cy = int(rng.integers(20, 580)), int(rng.integers(20, 580))
        p = _random_polygon(cx, cy, int(rng.integers(5, 25)), int(rng.choice([4, 5, 9, 13])), int(j % 7 == 0 and 1), rng)
        if kp == MPG and j % 3 == 0:
            polys.append([[], p] if j % 2 else [p, _random_polygon(cx, cy + 80, 6, 5, 0, rng)])
        else:
            polys.append(p if kp == PG else [p])
    cover = [sq(-5, -5, 700, 700), sq(300, 300, 320, 320, cw=True)]
    polys[17] = cover if kp == PG else [cover]
    polys[40] = []
    for i in range(n):
        style = i % 3
        if style == 0:  # from a polygon's vertex to another vertex of it or to a lattice point nearby
            p = row_polys(kp, polys[int(rng.integers(0, n))]) or [[sq(0, 0, 3, 3)]]
            v = p[0][0]
            a = v[int(rng.integers(0, len(v)))]
            seq = [a, v[int(rng.integers(0, len(v)))] if rng.random() < 0.5 else (a[0] + int(rng.integers(-9, 10)), a[1] + int(rng.integers(-9, 10)))]
        else:
            x, y = int(rng.integers(0, 600)), int(rng.integers(0, 600))
            seq = [(x, y)]
            for _ in range(int(rng.integers(1, 5))):
                x, y = x + int(rng.integers(-25, 26)), y + int(rng.integers(-25, 26))
                seq.append((x, y))
        lines.append(seq if kl == LS else ([seq, [(seq[0][0] + 40, seq[0][1]), (seq[0][0] + 45, seq[0][1] + 3)]] if i % 2 else [seq]))
    lines[23] = []
    lv = np.ones(n, dtype=bool)
    pv = np.ones(n, dtype=bool)
    lv[31] = False
    pv[52] = False
    # (pairs whose boxes are apart are EXTERIOR when both rows are usable: only the others go through the rational machinery)
    table = np.zeros((n, n), dtype=np.uint8)
    lm = masks(kl, lines, PG, [[sq(10**6, 10**6, 10**6 + 1, 10**6 + 1)]] * n, lv=lv)  # 4 for a usable line, else 0
    pm = masks(LS, [[(-(10**6), 0), (-(10**6), 1)]] * n, kp, polys, pv=pv)
    inf = 10**9
    lbox = np.array([_box_of([s for s in line_seqs(kl, r)]) if lm[i] else (inf, inf, -inf, -inf) for i, r in enumerate(lines)])
    pbox = np.array([_box_of([p[0] for p in row_polys(kp, r)]) if pm[j] else (inf, inf, -inf, -inf) for j, r in enumerate(polys)])
    for j in range(n):
        if not pm[j]:
            continue
        near = (lbox[:, 0] <= pbox[j, 2]) & (lbox[:, 2] >= pbox[j, 0]) & (lbox[:, 1] <= pbox[j, 3]) & (lbox[:, 3] >= pbox[j, 1])
        table[:, j] = np.where(lm != 0, EXTERIOR, 0)
        for i in np.nonzero(near & (lm != 0))[0]:
            table[i, j] = mask(kl, lines[i], kp, polys[j])
    return lines, lv, polys, pv, table


def _box_of(seqs):
    a = np.concatenate([np.asarray(s, dtype=np.int64).reshape(-1, 2) for s in seqs if len(s)])
    return (*a.min(axis=0), *a.max(axis=0))


def expected_pairs(table, pred: str, transpose=False):
    """(pairs sorted by (l, r), counts per left row, masks per pair) of a predicate over a mask table [lines, polys]; `transpose`:
    the polygons are the left side"""
    t = table.T if transpose else table
    hit = np.vectorize(PREDICATES[pred])(t) if t.size else np.zeros(t.shape, dtype=bool)
    ll, rr = np.nonzero(hit)
    return np.stack([ll, rr], axis=1).astype(np.uint32), np.bincount(ll, minlength=t.shape[0]).astype(np.uint32), t[ll, rr]
