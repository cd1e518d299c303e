"""Exact reference of gpk_validity and gpk_is_simple (include/geopolars_hip.h, csrc/gpk_validity.h) and their fixtures.

Brute force over fractions.Fraction, built straight from the float coordinates: any finite float input is exact.  Segment pairs whose
float boxes are apart share nothing (an exact statement), every other pair is intersected exactly: nothing, one rational point, or a
piece.  Ring x ring relations cut every segment of one ring at its intersection points with the other ring and classify the midpoint
of every piece against that ring with tests/exact_predicates.py (ring_pos on one integer grid).  Code 8 is decided twice: by the graph
of rings and distinct touch points, and — for rectilinear integer fixtures — by a flood fill over unit cells.

Rows are what tests/exact_ref.column takes: a POLYGON row is a list of rings, a MULTIPOLYGON row a list of polygons, a LINESTRING row
a list of (x, y), a MULTILINESTRING row a list of such lists."""
from __future__ import annotations

import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

from geopolars_amd import _abi
from tests import exact_predicates as E

LS, MLS, PG, MPG = _abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON
(VALID, COORDINATE, RING_SHAPE, SELF_INTERSECTION, RINGS_CROSS, HOLE_OUTSIDE, NESTED_HOLES, NESTED_MEMBERS, DISCONNECTED, NULL) = range(10)

# csrc/gpk_validity.h, restated
VAL_G_SMALL, VAL_G_LARGE, VAL_G_MEAN, VAL_BLOCK_COORDS, VAL_SEGS_PER_STRIP, VAL_STRIPS_MAX, VAL_ENTRIES = 4, 16, 32.0, 512, 8, 1024, 12288


def lanes_of(n_coords: int, n_rows: int) -> int:
    return VAL_G_LARGE if n_rows and n_coords / n_rows >= VAL_G_MEAN else VAL_G_SMALL


# ---- exact segments ------------------------------------------------------------------------------------------------------------------


def _fr(p):
    return (Fraction(float(p[0])), Fraction(float(p[1])))


def _cross(ux, uy, vx, vy):
    return ux * vy - uy * vx


def meet(a, b, c, d):
    """what the closed segments ab and cd (Fractions, a != b, c != d) share: None, ("point", x) or ("piece", x0, x1)"""
    dx, dy, ex, ey = b[0] - a[0], b[1] - a[1], d[0] - c[0], d[1] - c[1]
    den = _cross(dx, dy, ex, ey)
    wx, wy = c[0] - a[0], c[1] - a[1]
    if den != 0:
        t, u = _cross(wx, wy, ex, ey) / den, _cross(wx, wy, dx, dy) / den
        if 0 <= t <= 1 and 0 <= u <= 1:
            return ("point", (a[0] + t * dx, a[1] + t * dy))
        return None
    if _cross(wx, wy, dx, dy) != 0:
        return None
    dd = dx * dx + dy * dy
    tc, td = (wx * dx + wy * dy) / dd, ((d[0] - a[0]) * dx + (d[1] - a[1]) * dy) / dd
    lo, hi = max(Fraction(0), min(tc, td)), min(Fraction(1), max(tc, td))
    if lo > hi:
        return None
    at = lambda t: (a[0] + t * dx, a[1] + t * dy)  # noqa: E731
    return ("point", at(lo)) if lo == hi else ("piece", at(lo), at(hi))


def on_seg(x, a, b):
    return _cross(b[0] - a[0], b[1] - a[1], x[0] - a[0], x[1] - a[1]) == 0 and min(a[0], b[0]) <= x[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= x[1] <= max(a[1], b[1])


class Seq:
    """a coordinate sequence of a row: the float array, its first coordinate's index in the column, its non-degenerate segments
    (index of the first coordinate within the sequence, ends as Fractions) and their float boxes"""

    def __init__(self, xy, base):
        self.xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        self.base = base
        self.n = len(self.xy)
        idx = [k for k in range(self.n - 1) if (self.xy[k] != self.xy[k + 1]).any()] if np.isfinite(self.xy).all() else []
        self.idx = np.array(idx, dtype=np.int64)
        self.segs = [(_fr(self.xy[k]), _fr(self.xy[k + 1])) for k in idx]
        self.lo = np.minimum(self.xy[idx], self.xy[[k + 1 for k in idx]]) if idx else np.zeros((0, 2))
        self.hi = np.maximum(self.xy[idx], self.xy[[k + 1 for k in idx]]) if idx else np.zeros((0, 2))
        self.closed = self.n >= 2 and bool((self.xy[0] == self.xy[-1]).all())

    def near(self, lo, hi):
        """positions (in segs) of the segments whose boxes meet the box [lo, hi]"""
        if not len(self.idx):
            return []
        return np.nonzero((self.lo[:, 0] <= hi[0]) & (self.hi[:, 0] >= lo[0]) & (self.lo[:, 1] <= hi[1]) & (self.hi[:, 1] >= lo[1]))[0].tolist()


def self_faults(s: Seq, ring: bool):
    """column indices of the segments of one sequence that break the simplicity rule (a ring: always closed)"""
    m = len(s.segs)
    bad = []
    wrap = ring or s.closed
    for p in range(m):
        a, b = s.segs[p]
        for q in s.near(s.lo[p], s.hi[p]):
            if q <= p:
                continue
            got = meet(a, b, *s.segs[q])
            if got is None:
                continue
            consecutive = q == p + 1 or (wrap and p == 0 and q == m - 1)
            if got[0] == "piece" or not consecutive:
                bad += [s.base + int(s.idx[p]), s.base + int(s.idx[q])]
    return bad


def _grid_pos(points, ring_fr):
    """E.ring_pos of rational points against a ring of Fractions: everything brought to one integer grid"""
    if not points:
        return np.zeros(0, dtype=np.int64)
    den = math.lcm(*[v.denominator for p in points for v in p], *[v.denominator for p in ring_fr for v in p])
    X = np.array([int(p[0] * den) for p in points], dtype=object)
    Y = np.array([int(p[1] * den) for p in points], dtype=object)
    R = np.array([[int(p[0] * den), int(p[1] * den)] for p in ring_fr], dtype=object)
    return E.ring_pos(X, Y, R)


def pieces(r: Seq, s: Seq):
    """ring r cut by ring s: [(position in r.segs, midpoint, end point)] in ring order, and the class of every midpoint against s"""
    out = []
    for p, (a, b) in enumerate(r.segs):
        ts = {Fraction(0), Fraction(1)}
        dx, dy = b[0] - a[0], b[1] - a[1]
        par = lambda x: (x[0] - a[0]) / dx if dx != 0 else (x[1] - a[1]) / dy  # noqa: E731
        for q in s.near(r.lo[p], r.hi[p]):
            got = meet(a, b, *s.segs[q])
            if got is not None:
                ts.update(par(x) for x in got[1:])
        ts = sorted(ts)
        for t0, t1 in zip(ts, ts[1:]):
            tm = (t0 + t1) / 2
            out.append((p, (a[0] + tm * dx, a[1] + tm * dy), (a[0] + t1 * dx, a[1] + t1 * dy)))
    ring_fr = [_fr(v) for v in s.xy]
    return out, _grid_pos([o[1] for o in out], ring_fr)


def cross_faults(r: Seq, s: Seq):
    """column indices of the segments of r and s that take part in a code-4 fault, from r's view: the segments of r with a piece on s,
    and every segment of either ring through a point where two consecutive pieces of r are classified differently"""
    pcs, pos = pieces(r, s)
    bad = []
    n = len(pcs)
    for k in range(n):
        if pos[k] == E.BOUNDARY:
            bad.append(r.base + int(r.idx[pcs[k][0]]))
        if n > 1 and pos[k] != pos[(k + 1) % n]:
            x = pcs[k][2]
            bad += [r.base + int(r.idx[p]) for p, (a, b) in enumerate(r.segs) if on_seg(x, a, b)]
            bad += [s.base + int(s.idx[q]) for q, (c, d) in enumerate(s.segs) if on_seg(x, c, d)]
    return bad


def ring_side(r: Seq, s: Seq):
    """the classes (a set of E.INSIDE / E.BOUNDARY / E.OUTSIDE) of the pieces of ring r against ring s"""
    return set(pieces(r, s)[1].tolist())


# ---- validity --------------------------------------------------------------------------------------------------------------------------


def _members(kind, row, base):
    """the non-empty members of a polygonal row as lists of Seq (non-empty rings only), and the coordinate count of the row"""
    polys = [row] if kind == PG else list(row)
    out = []
    for p in polys:
        rings = []
        for r in p:
            rings.append(Seq(r, base))
            base += len(r)
        if rings and rings[0].n:
            out.append([q for q in rings if q.n])
    return out, base


def touch_graph_cut(rings) -> bool:
    """the graph of a member's rings and the distinct points where two or more of them touch has a cycle"""
    pts = set()
    for i, r in enumerate(rings):
        for s in rings[i + 1 :]:
            for p, (a, b) in enumerate(r.segs):
                for q in s.near(r.lo[p], r.hi[p]):
                    got = meet(a, b, *s.segs[q])
                    if got is not None:
                        pts.update(got[1:])
    parent = list(range(len(rings) + len(pts)))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for k, x in enumerate(pts):
        for i, r in enumerate(rings):
            if any(on_seg(x, a, b) for a, b in r.segs):
                ra, rb = find(i), find(len(rings) + k)
                if ra == rb:
                    return True
                parent[ra] = rb
    return False


def flood_fill_cut(rings) -> bool:
    """second opinion for rectilinear integer members: the unit cells inside the shell and outside the holes, two cells connected
    across a unit edge that lies on no ring, fall into more than one component"""
    arrs = [np.asarray(r.xy if isinstance(r, Seq) else r, dtype=np.float64) for r in rings]
    assert all((a == np.round(a)).all() for a in arrs)
    blocked_v, blocked_h = set(), set()  # unit edges on a ring: vertical (x, y)-(x, y+1), horizontal (x, y)-(x+1, y)
    for a in arrs:
        for (x0, y0), (x1, y1) in zip(a[:-1].astype(int).tolist(), a[1:].astype(int).tolist()):
            assert x0 == x1 or y0 == y1, "rectilinear rings only"
            if x0 == x1:
                blocked_v.update((x0, y) for y in range(min(y0, y1), max(y0, y1)))
            else:
                blocked_h.update((x, y0) for x in range(min(x0, x1), max(x0, x1)))
    lo, hi = arrs[0].min(axis=0).astype(int), arrs[0].max(axis=0).astype(int)
    cells = []
    for x in range(lo[0], hi[0]):
        for y in range(lo[1], hi[1]):
            c = (Fraction(2 * x + 1, 2), Fraction(2 * y + 1, 2))
            if _grid_pos([c], [_fr(v) for v in arrs[0]])[0] == E.INSIDE and all(_grid_pos([c], [_fr(v) for v in h])[0] == E.OUTSIDE for h in arrs[1:]):
                cells.append((x, y))
    cells = set(cells)
    if not cells:
        return False
    seen, todo = set(), [next(iter(cells))]
    while todo:
        x, y = todo.pop()
        if (x, y) in seen:
            continue
        seen.add((x, y))
        for nx, ny, blocked in ((x + 1, y, (x + 1, y) in blocked_v), (x - 1, y, (x, y) in blocked_v), (x, y + 1, (x, y + 1) in blocked_h), (x, y - 1, (x, y) in blocked_h)):
            if not blocked and (nx, ny) in cells:
                todo.append((nx, ny))
    return len(seen) != len(cells)


def validity(kind, row, valid=True, base=0):
    """(code, where) of one row whose first coordinate has index `base` in the column"""
    if not valid or row is None:
        return NULL, -1
    members, _ = _members(kind, row, base)
    rings = [r for m in members for r in m]
    for r in rings:
        bad = np.nonzero(~np.isfinite(r.xy).all(axis=1))[0]
        if len(bad):
            return COORDINATE, r.base + int(bad[0])
    for r in rings:
        if r.n < 4 or not r.closed:
            return RING_SHAPE, r.base
    bad = []
    for r in rings:
        bad += self_faults(r, True) if r.segs else [r.base]
    if bad:
        return SELF_INTERSECTION, min(bad)
    for r in rings:
        for s in rings:
            if s is not r and (r.lo.min(axis=0) <= s.hi.max(axis=0)).all() and (s.lo.min(axis=0) <= r.hi.max(axis=0)).all():
                bad += cross_faults(r, s)
    if bad:
        return RINGS_CROSS, min(bad)
    for m in members:
        for h in m[1:]:
            if E.OUTSIDE in ring_side(h, m[0]):
                return HOLE_OUTSIDE, h.base
    holes = [h.base for m in members for h in m[1:] for k in m[1:] if k is not h and E.INSIDE in ring_side(h, k)]
    if holes:
        return NESTED_HOLES, min(holes)
    for b, mb in enumerate(members):
        for ma in members[:b]:
            for inner, outer in ((mb, ma), (ma, mb)):
                # a piece of a ring of one member in the interior of the other: inside its shell, outside all its holes
                for r in inner:
                    pcs, pos = pieces(r, outer[0])
                    mids = [pc[1] for pc, p in zip(pcs, pos) if p == E.INSIDE]
                    for h in outer[1:]:
                        if mids:
                            ph = _grid_pos(mids, [_fr(v) for v in h.xy])
                            mids = [x for x, p in zip(mids, ph) if p == E.OUTSIDE]
                    if mids:
                        return NESTED_MEMBERS, mb[0].base
    for m in members:
        if len(m) > 1 and touch_graph_cut(m):
            return DISCONNECTED, m[0].base
    return VALID, -1


def n_coords(kind, row) -> int:
    if row is None:
        return 0
    if kind == LS:
        return len(row)
    if kind in (PG, MLS):
        return sum(len(r) for r in row)
    return sum(len(r) for p in row for r in p)


def validity_column(kind, rows, valid=None):
    """(codes uint8, where int32) of a column"""
    codes, where, base = [], [], 0
    for i, row in enumerate(rows):
        c, w = validity(kind, row, valid is None or bool(valid[i]), base)
        codes.append(c)
        where.append(w)
        base += n_coords(kind, row)
    return np.array(codes, dtype=np.uint8), np.array(where, dtype=np.int32)


# ---- simplicity ------------------------------------------------------------------------------------------------------------------------


def is_simple(kind, row, valid=True) -> bool:
    if not valid or row is None:
        return False
    seqs = [Seq(s, 0) for s in ([row] if kind == LS else row) if len(s)]
    if any(not np.isfinite(s.xy).all() for s in seqs):
        return False
    if any(self_faults(s, False) for s in seqs):
        return False
    for i, r in enumerate(seqs):
        ends_r = [] if r.closed else [_fr(r.xy[0]), _fr(r.xy[-1])]
        for s in seqs[i + 1 :]:
            ends_s = [] if s.closed else [_fr(s.xy[0]), _fr(s.xy[-1])]
            for p, (a, b) in enumerate(r.segs):
                for q in s.near(r.lo[p], r.hi[p]):
                    got = meet(a, b, *s.segs[q])
                    if got is None:
                        continue
                    if got[0] == "piece" or got[1] not in ends_r or got[1] not in ends_s:
                        return False
    return True


def is_simple_column(kind, rows, valid=None):
    return np.array([is_simple(kind, r, valid is None or bool(valid[i])) for i, r in enumerate(rows)], dtype=bool)


# ---- known answers -------------------------------------------------------------------------------------------------------------------


def sq(x0, y0, x1, y1, cw=False):
    r = [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]
    return r[::-1] if cw else r


def dia(cx, cy, r):
    return [(cx - r, cy), (cx, cy - r), (cx + r, cy), (cx, cy + r), (cx - r, cy)]


BIG = sq(0, 0, 20, 20)
NAN, INF = float("nan"), float("inf")
# (name, kind, row, code)
KNOWN = [
    ("square", PG, [BIG], VALID),
    ("donut", PG, [BIG, sq(5, 5, 9, 9, cw=True)], VALID),
    ("repeated coordinates", PG, [[(0, 0), (0, 0), (4, 0), (4, 0), (4, 4), (0, 4), (0, 4), (0, 0), (0, 0)]], VALID),
    ("NaN coordinate", PG, [BIG, [(5, 5), (9, 5), (9, NAN), (5, 5)]], COORDINATE),
    ("infinite coordinate", PG, [[(0, 0), (INF, 0), (4, 4), (0, 0)]], COORDINATE),
    ("unclosed ring", PG, [[(0, 0), (4, 0), (4, 4), (0, 4)]], RING_SHAPE),
    ("three coordinates", PG, [[(0, 0), (4, 0), (0, 0)]], RING_SHAPE),
    ("short hole", PG, [BIG, [(5, 5), (6, 6), (5, 5)]], RING_SHAPE),
    ("bow-tie", PG, [[(0, 0), (4, 4), (4, 0), (0, 4), (0, 0)]], SELF_INTERSECTION),
    ("spike A-B-A", PG, [[(0, 0), (4, 0), (4, 4), (7, 7), (4, 4), (0, 4), (0, 0)]], SELF_INTERSECTION),
    ("ring touching itself at a vertex", PG, [[(0, 0), (8, 0), (8, 8), (4, 0), (0, 8), (0, 0)]], SELF_INTERSECTION),
    ("ring touching itself vertex to vertex", PG, [[(0, 0), (4, 4), (8, 0), (8, 8), (4, 4), (0, 8), (0, 0)]], SELF_INTERSECTION),
    ("all collinear", PG, [[(0, 0), (4, 0), (8, 0), (2, 0), (0, 0)]], SELF_INTERSECTION),
    ("two points", PG, [[(0, 0), (4, 0), (0, 0), (0, 0)]], SELF_INTERSECTION),
    ("one point", PG, [[(3, 3), (3, 3), (3, 3), (3, 3)]], SELF_INTERSECTION),
    ("spike at the closing vertex", PG, [[(0, 0), (4, 0), (4, 4), (0, 4), (0, -3), (0, 0)]], SELF_INTERSECTION),
    ("hole sharing an edge with the shell", PG, [BIG, sq(0, 5, 4, 9, cw=True)], RINGS_CROSS),
    ("hole crossing the shell", PG, [BIG, sq(15, 5, 25, 9, cw=True)], RINGS_CROSS),
    ("hole crossing the shell through a vertex", PG, [BIG, dia(20, 20, 3)], RINGS_CROSS),
    ("two identical holes", PG, [BIG, sq(5, 5, 9, 9, cw=True), sq(5, 5, 9, 9, cw=True)], RINGS_CROSS),
    ("two holes crossing", PG, [BIG, sq(5, 5, 9, 9, cw=True), dia(9, 7, 2)], RINGS_CROSS),
    ("hole outside the shell", PG, [BIG, sq(25, 5, 29, 9, cw=True)], HOLE_OUTSIDE),
    ("hole outside the shell, touching it", PG, [BIG, dia(23, 10, 3)], HOLE_OUTSIDE),
    ("hole in a hole", PG, [BIG, sq(4, 4, 12, 12, cw=True), sq(6, 6, 8, 8, cw=True)], NESTED_HOLES),
    ("hole in a hole, touching it", PG, [BIG, sq(6, 6, 8, 8, cw=True), sq(4, 4, 12, 12, cw=True), dia(10, 10, 2)], NESTED_HOLES),
    ("member inside a member", MPG, [[BIG], [sq(5, 5, 9, 9)]], NESTED_MEMBERS),
    ("member around a member", MPG, [[sq(5, 5, 9, 9)], [sq(30, 0, 34, 4)], [BIG]], NESTED_MEMBERS),
    ("member inside another member's hole", MPG, [[BIG, sq(4, 4, 12, 12, cw=True)], [sq(6, 6, 8, 8)]], VALID),
    ("the same, touching the hole ring at one point", MPG, [[BIG, sq(4, 4, 12, 12, cw=True)], [dia(10, 10, 2)]], VALID),
    ("member over another member's hole", MPG, [[BIG, sq(8, 8, 10, 10, cw=True)], [sq(22, 0, 30, 4)], [sq(6, 6, 9, 9)]], RINGS_CROSS),
    ("member around another member's hole", MPG, [[BIG, sq(8, 8, 10, 10, cw=True)], [sq(6, 6, 12, 12)]], NESTED_MEMBERS),
    ("hole touching the shell at one point", PG, [BIG, dia(3, 10, 3)], VALID),
    ("hole touching the shell at its repeated closing coordinate", PG, [[(0, 0), (20, 0), (20, 20), (0, 20), (0, 0), (0, 0)], [(0, 0), (4, 2), (2, 4), (0, 0)]], VALID),
    ("two holes touching where both repeat their closing coordinate", PG, [BIG, [(10, 10), (6, 12), (6, 8), (10, 10), (10, 10), (10, 10)],
                                                                         [(10, 10), (10, 10), (14, 8), (14, 12), (10, 10), (10, 10)]], VALID),
    ("hole touching the shell at two points", PG, [BIG, dia(10, 10, 10)[:2] + [(12, 8), (10, 20), (0, 10)]], DISCONNECTED),
    ("two holes touching at one point", PG, [BIG, dia(5, 10, 2), dia(9, 10, 2)], VALID),
    ("three holes meeting at one common point", PG, [BIG, [(10, 10), (6, 12), (6, 8), (10, 10)], [(10, 10), (14, 8), (14, 12), (10, 10)],
                                                    [(10, 10), (8, 15), (12, 15), (10, 10)]], VALID),
    ("a chain of holes from shell to shell", PG, [BIG, dia(5, 10, 5), dia(15, 10, 5)], DISCONNECTED),
    ("a ring of three holes", PG, [sq(0, 0, 30, 30), sq(5, 5, 15, 10, cw=True), sq(15, 10, 25, 15, cw=True), [(5, 10), (10, 20), (25, 15), (10, 18), (5, 10)]],
     DISCONNECTED),
    ("members touching at a point", MPG, [[sq(0, 0, 4, 4)], [dia(6, 2, 2)]], VALID),
    ("members sharing an edge", MPG, [[sq(0, 0, 4, 4)], [sq(4, 0, 8, 4)]], RINGS_CROSS),
    ("members sharing a part of an edge", MPG, [[sq(0, 0, 4, 4)], [sq(4, 1, 8, 3)]], RINGS_CROSS),
    ("empty row", PG, [], VALID),
    ("only empty members", MPG, [[], [[]]], VALID),
    ("null row", PG, None, NULL),
]


def as_kind(kind_from, row, kind_to):
    """a POLYGON row as a MULTIPOLYGON row with an empty member in front"""
    if row is None or kind_from == kind_to:
        return row
    assert kind_from == PG and kind_to == MPG
    return [[], row]


def known_column(kind):
    """(rows, validity, codes, where) of the known answers that exist in `kind`"""
    sel = [k for k in KNOWN if kind == MPG or k[1] == PG]
    rows = [as_kind(k[1], k[2], kind) for k in sel]
    valid = [r is not None for r in rows]
    rows = [[] if r is None else r for r in rows]
    codes, where = validity_column(kind, rows, valid)
    assert codes.tolist() == [k[3] for k in sel], [(k[0], int(c)) for k, c in zip(sel, codes) if k[3] != c]
    return rows, valid, codes, where


# (name, kind, row, simple)
KNOWN_SIMPLE = [
    ("a segment", LS, [(0, 0), (4, 4)], True),
    ("a closed ring", LS, [(0, 0), (4, 0), (4, 4), (0, 0)], True),
    ("a figure-8", LS, [(0, 0), (4, 4), (4, 0), (0, 4), (0, 0)], False),
    ("a lasso", LS, [(0, 0), (4, 0), (4, 4), (0, 4), (0, 0), (-3, -3)], False),
    ("a spike", LS, [(0, 0), (4, 0), (2, 0)], False),
    ("an end point on its own interior", LS, [(0, 0), (4, 0), (4, 4), (2, 0)], False),
    ("one coordinate", LS, [(1, 1)], True),
    ("equal coordinates", LS, [(1, 1), (1, 1), (1, 1)], True),
    ("repeated coordinates", LS, [(0, 0), (0, 0), (4, 0), (4, 0), (4, 4)], True),
    ("no coordinates", LS, [], True),
    ("NaN", LS, [(0, 0), (NAN, 1)], False),
    ("infinite", LS, [(0, 0), (1, -INF)], False),
    ("a T-junction of two members at a mid-segment point", MLS, [[(0, 0), (8, 0)], [(4, 0), (4, 5)]], False),
    ("an end-to-end chain", MLS, [[(0, 0), (4, 0)], [(4, 0), (4, 4)], [(4, 4), (9, 9)]], True),
    ("an end point on a closed member's start", MLS, [[(0, 0), (4, 0), (4, 4), (0, 0)], [(0, 0), (-3, -3)]], False),
    ("two members crossing", MLS, [[(0, 0), (4, 4)], [(0, 4), (4, 0)]], False),
    ("two members overlapping", MLS, [[(0, 0), (4, 0)], [(2, 0), (6, 0)]], False),
    ("two members apart, one empty", MLS, [[(0, 0), (4, 0)], [], [(0, 2), (4, 2)]], True),
    ("null", LS, None, False),
]


def known_simple_column(kind):
    sel = [k for k in KNOWN_SIMPLE if kind == MLS or k[1] == LS]
    rows = [k[2] if (k[2] is None or k[1] == kind) else [[], k[2]] for k in sel]
    valid = [r is not None for r in rows]
    rows = [[] if r is None else r for r in rows]
    want = is_simple_column(kind, rows, valid)
    assert want.tolist() == [k[3] for k in sel], [(k[0], bool(w)) for k, w in zip(sel, want) if k[3] != w]
    return rows, valid, want


# ---- transformations that keep the answers ------------------------------------------------------------------------------------------


def map_rings(kind, row, f):
    if kind == PG:
        return [f(r) for r in row]
    return [[f(r) for r in p] for p in row]


def placed(kind, rows, scale, shift=(0.0, 0.0)):
    """rows scaled by a power of two and then shifted (exact for the fixtures: small integers)"""
    def f(r):
        out = [(x * scale + shift[0], y * scale + shift[1]) for x, y in r]
        assert all(Fraction(u) == Fraction(x) * Fraction(scale) + Fraction(shift[0]) and Fraction(v) == Fraction(y) * Fraction(scale) + Fraction(shift[1])
                   for (x, y), (u, v) in zip(r, out)), "the placement is not exact"
        return out

    return [map_rings(kind, row, f) for row in rows]


SHIFT = (2.0**30, -(2.0**31))  # after a scale of 2^-20 the sums still fit 53 bits for the fixtures' small integers
PLACEMENTS = [(2.0**-20, (0.0, 0.0)), (2.0**20, (0.0, 0.0)), (2.0**-20, SHIFT), (2.0**20, SHIFT), (1.0, SHIFT)]


def pad_ring(r, k):
    """k more vertices inside every edge of an integer ring (coordinates scaled by k + 1 first): relation_ref.padded's trick"""
    a = np.asarray(r, dtype=np.float64).reshape(-1, 2)
    if not np.isfinite(a).all() or len(a) < 2:
        return [(float(x) * (k + 1), float(y) * (k + 1)) for x, y in a]
    a = a.astype(np.int64) * (k + 1)
    out = []
    for p, q in zip(a[:-1], a[1:]):
        out.extend(tuple(int(c) for c in p + (q - p) * j // (k + 1)) for j in range(k + 1))
    out.append(tuple(int(c) for c in a[-1]))
    return out


def padded(kind, rows, k, every=1, first=0):
    """rows first, first + every, ... padded with k vertices inside every edge; the others stay (all coordinates are scaled by k + 1
    only in the padded rows: rows do not see each other)"""
    return [map_rings(kind, row, lambda r: pad_ring(r, k)) if k and i % every == first % every else row for i, row in enumerate(rows)]


# ---- random lattice columns ------------------------------------------------------------------------------------------------------------


def _rand_ring(rng, x0, y0, w, h, n):
    """a closed lattice ring of n coordinates in the box: points by angle round its centre (often simple, sometimes not)"""
    k = n - 1
    cx, cy = x0 + w / 2, y0 + h / 2
    t = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = rng.uniform(0.5, 1.0, k)
    pts = [(int(np.clip(round(cx + r * w / 2 * np.cos(a)), x0, x0 + w)), int(np.clip(round(cy + r * h / 2 * np.sin(a)), y0, y0 + h))) for a, r in zip(t, rad)]
    return pts + pts[:1]


@lru_cache(maxsize=None)
def random_column(kind, n_rows=96, seed=5):
    """96 rows on a 12 x 12 lattice: rings of 4 - 9 coordinates, 1 - 3 holes, 1 - 3 members (MULTIPOLYGON: each in its own 4 x 12
    box unless the style nests them), a style per row that plants one kind of fault — or none, or whatever random rings give.
    Returns (rows, validity, codes, where)."""
    rng = np.random.default_rng(seed + kind)
    rows = []
    for i in range(n_rows):
        style = i % 12
        n_m = 1 if kind == PG else 1 + (i // 12) % 3
        members = []
        for m in range(n_m):
            w, x0 = (12, 0) if n_m == 1 else (4, 4 * m)
            n_h = 1 + (i // 36 + m) % 3
            box = sq(x0, 0, x0 + w, 12)
            small = lambda: _rand_ring(rng, int(rng.integers(x0, x0 + w - 1)), int(rng.integers(0, 9)), int(rng.integers(2, 4)), int(rng.integers(2, 5)), int(rng.integers(4, 8)))[::-1]  # noqa: E731
            if style == 0:
                rings = [_rand_ring(rng, x0, 0, w, 12, int(rng.integers(4, 10)))]
            elif style in (1, 3):
                rings = [_rand_ring(rng, x0, 0, w, 12, int(rng.integers(5, 10)))] + [small() for _ in range(n_h)]
            elif style in (2, 4):
                rings = [box] + [small() for _ in range(n_h if style == 4 else 1)]
            elif style == 5:  # a hole outside the shell, above it
                rings = [sq(x0, 0, x0 + w, 8), sq(x0 + 1, 1, x0 + 2, 2, cw=True), sq(x0 + 1, 9, x0 + 3, 11, cw=True)][: 1 + max(2, n_h)]
            elif style == 6 or (style == 7 and kind == PG):  # a hole in a hole, touching it or not
                inner = [(x0 + 2, 3), (x0 + 3, 6), (x0 + 2, 9), (x0 + 1, 6), (x0 + 2, 3)] if i % 24 < 12 else [(x0 + 2, 3), (x0 + 1, 5), (x0 + 2, 9), (x0 + 2, 3)]
                rings = [box, sq(x0 + 1, 1, x0 + 3, 11, cw=True), inner]
            elif style == 7:  # members inside each other
                rings = [sq(2 * m, 2 * m, 12 - 2 * m, 12 - 2 * m)]
            elif style == 8:  # diamonds in a row: a chain from shell to shell, or short of it
                r = 2 if rng.random() < 0.7 else 1
                rings = [box] + ([dia(x0 + 2, 2 + 4 * h, r) for h in range(n_h)] if w == 4 else [dia(x0 + 2 + 4 * h, 6, r) for h in range(n_h)])
            elif style == 9:  # holes that touch the shell once or twice
                rings = [box] + [dia(x0 + 2, 2 + 4 * h, 2) if (i // 12 + h) % 2 else [(x0, 4 * h + 1), (x0 + w, 4 * h + 2), (x0 + 2, 4 * h + 3), (x0, 4 * h + 1)]
                                 for h in range(n_h)]
            elif style == 10:  # an unclosed ring, a ring of three coordinates
                rings = [box[:-1] if i % 24 < 12 else box[:2] + box[:1]] if m == n_m - 1 else [box]
            else:  # a NaN or infinite coordinate in the last ring of the row, every other time
                rings = [box, sq(x0 + 1, 1, x0 + 3, 3, cw=True)]
                if m == n_m - 1 and i % 24 < 12:
                    rings[-1] = [(x, (NAN if i % 48 < 24 else INF) if j == 1 else y) for j, (x, y) in enumerate(rings[-1])]
            members.append(rings)
        if kind == MPG and i % 5 == 0:
            members.insert(int(rng.integers(0, len(members) + 1)), [])
        rows.append(members[0] if kind == PG else members)
    valid = [i % 31 != 30 for i in range(n_rows)]
    codes, where = validity_column(kind, rows, valid)
    return rows, valid, codes, where


# ---- the work-group path: 4096-coordinate zigzag rings -----------------------------------------------------------------------------


def zigzag(n=4096, hole=None, fault=None):
    """a closed ring of n coordinates: teeth along the top (x = 0 .. n - 4, y alternating 4 and 8), back along y = 0.  fault:
    'first' / 'last' — the first or the last tooth is pulled below the base line (its segments cross the base: the first and the
    last segment pairs of the ring); 'strip' — a tooth in the middle is drawn far to the right, across many strips"""
    m = n - 3
    top = [(float(x), 8.0 if x % 2 else 4.0) for x in range(m)]
    if fault == "first":
        top[1] = (1.0, -3.0)
    elif fault == "last":
        top[m - 2] = (float(m - 2), -3.0)
    elif fault == "strip":
        top[m // 2] = (float(m // 2 + 700), 6.0 if (m // 2) % 2 else 6.5)
    ring = [(0.0, 0.0)] + [(float(m - 1), 0.0)] + top[::-1] + [(0.0, 0.0)]
    assert len(ring) == n
    rings = [ring]
    if hole is not None:
        rings.append(hole)
    return rings


@lru_cache(maxsize=None)
def large_column():
    """six rows of the work-group path: (rows, codes, where)"""
    n = 4096
    m = n - 3
    inside = [(m - 3.0, 1.0), (m - 3.0, 3.0), (m - 2.0, 3.0), (m - 2.0, 1.0), (m - 3.0, 1.0)]  # in the last strip, inside
    poking = [(m - 3.0, 1.0), (m - 3.0, 5.0), (m - 2.0, 3.0), (m - 2.0, 1.0), (m - 3.0, 1.0)]  # leaves through the shell vertex (m - 3, 4)
    rows = [zigzag(n), zigzag(n, fault="first"), zigzag(n, fault="last"), zigzag(n, fault="strip"), zigzag(n, hole=inside), zigzag(n, hole=poking)]
    codes, where = validity_column(PG, rows)
    return rows, codes, where
