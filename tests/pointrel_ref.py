"""The exact reference of the point relation mask (gpk_point_relation, include/geopolars_hip.h), built differently from the kernel:
every point of A is classified on its own by brute force — exact_ref.on_segment over every segment and a count of the member ends for a
line, exact_ref.geom_position (shell and holes, part by part, by winding numbers) for a polygon, set membership for points — and bit 8
is a set difference.  The kernel's even-odd pass over all edges of a row appears nowhere here.

    mask(ka, row_a, kb, row_b)      the reference;  masks(...) over columns
    KNOWN, TIES                     hand-derived cases: (name, points of A, dimension of B, members of B, mask)
    case_columns, padded, placed, random_columns, join_fixture, mask_table, expected_pairs   fixtures, as tests/linerel_ref.py has them

Rows are those of exact_ref.column: a POINT row is (x, y) or None, a MULTIPOINT row a list of points, a LINESTRING row a list of
coordinates, a MULTILINESTRING row a list of those, a POLYGON row a list of rings, a MULTIPOLYGON row a list of polygons.  Coordinates
are exact in doubles."""
from __future__ import annotations

import math
from collections import Counter
from functools import lru_cache

import numpy as np

from geopolars_amd import _abi
from tests import exact_ref as E
from tests import linerel_ref as L
from tests import relation_ref as R

PT, MPT, LS, MLS, PG, MPG = (_abi.GEOM_POINT, _abi.GEOM_MULTIPOINT, _abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON,
                             _abi.GEOM_MULTIPOLYGON)
DIM = {PT: 0, MPT: 0, LS: 1, MLS: 1, PG: 2, MPG: 2}
FAMILIES = [(a, b) for a in (PT, MPT) for b in (PT, MPT, LS, MLS, PG, MPG)]
NAMES = {PT: "pt", MPT: "mpt", LS: "ls", MLS: "mls", PG: "pg", MPG: "mpg"}
INTERIOR, BOUNDARY, EXTERIOR, B_OUTSIDE = 1, 2, 4, 8
PLACEMENTS = L.PLACEMENTS

# DE-9IM with dim(A) = 0 over (mask, the dimension of B's family)
PREDICATES = {
    "intersects": lambda m, d: bool(m & 3),
    "disjoint": lambda m, d: m != 0 and not (m & 3),
    "within": lambda m, d: bool(m & 1) and not (m & 4),
    "covered_by": lambda m, d: bool(m & 3) and not (m & 4),
    "contains": lambda m, d: bool(m & 1) and not (m & 8),
    "covers": lambda m, d: bool(m & 3) and not (m & 8),
    "touches": lambda m, d: bool(m & 2) and not (m & 1),
    "equals": lambda m, d: bool(m & 1) and not (m & 12),
    "crosses": lambda m, d: d >= 1 and bool(m & 1) and bool(m & 4),
    "overlaps": lambda m, d: d == 0 and (m & 13) == 13,
}
PRED_IDS = {"intersects": 0, "within": 1, "contains": 2, "covered_by": 3, "covers": 4, "crosses": 5, "touches": 6, "overlaps": 7, "equals": 8}  # GPK_PT_PRED_*
TRANSPOSED = {"within": "contains", "contains": "within", "covered_by": "covers", "covers": "covered_by"}

# the masks that can occur, by the family of B (test_pointrel_ref.py confirms them by brute force), and by the pair of kinds: a POINT
# column on the A side has one point, so exactly one of the bits 1, 2, 4
REACHABLE = {0: (1, 5, 9, 12, 13), 1: (1, 5, 9, 10, 11, 12, 13, 14, 15), 2: (9, 10, 11, 12, 13, 14, 15)}


def reachable(ka, kb):
    if ka == MPT:
        return (1, 5, 12) if kb == PT else REACHABLE[DIM[kb]]
    if kb == PT:
        return (1, 12)
    return {0: (1, 9, 12), 1: (1, 9, 10, 12), 2: (9, 10, 12)}[DIM[kb]]


def swapped(m):
    """mask(B, A) from mask(A, B) for two punctual rows: 4 <-> 8"""
    m = np.asarray(m, dtype=np.uint8)
    return ((m & 3) | ((m & 4) << 1) | ((m & 8) >> 1)).astype(np.uint8)


def _finite(p):
    return math.isfinite(p[0]) and math.isfinite(p[1])


def points_of(kind, row, valid=True):
    """the points of a usable punctual row, else None (null, no point, a NaN or infinite coordinate)"""
    if not valid or row is None:
        return None
    pts = [tuple(row)] if kind == PT else [tuple(p) for p in row]
    if not pts or not all(_finite(p) for p in pts):
        return None
    return pts


def _line_members(kind, row, valid):
    if not valid:
        return None
    ms = [m for m in L.members(kind, row) if len(m)]
    if not ms or not all(_finite(p) for m in ms for p in m):
        return None
    return [[tuple(p) for p in m] for m in ms]


def _polys(kind, row, valid):
    """the non-empty members of a usable polygonal row, else None: the conditions of gpk_polygon_relation and finite coordinates"""
    if not valid:
        return None
    polys = R.row_polys(kind, row)
    if not polys or not all(_finite(p) for g in polys for r in g for p in r) or not all(R._ring_usable(r) for g in polys for r in g):
        return None
    return [[[tuple(p) for p in r] for r in g] for g in polys]


def usable(kind, row, valid=True) -> bool:
    d = DIM[kind]
    return (points_of(kind, row, valid) if d == 0 else _line_members(kind, row, valid) if d == 1 else _polys(kind, row, valid)) is not None


def classify(p, kb, row_b, b_valid=True):
    """the bit of one point against a usable row B (None: B unusable)"""
    d = DIM[kb]
    if d == 0:
        pb = points_of(kb, row_b, b_valid)
        return None if pb is None else (INTERIOR if p in set(pb) else EXTERIOR)
    if d == 1:
        ms = _line_members(kb, row_b, b_valid)
        if ms is None:
            return None
        on = any(p == c for m in ms for c in m) or any(a != b and E.on_segment(p, a, b) for m in ms for a, b in zip(m[:-1], m[1:]))
        if not on:
            return EXTERIOR
        ends = sum((m[0] == p) + (m[-1] == p) for m in ms)
        return BOUNDARY if ends % 2 else INTERIOR
    polys = _polys(kb, row_b, b_valid)
    if polys is None:
        return None
    return {1: INTERIOR, 0: BOUNDARY, -1: EXTERIOR}[E.geom_position(p, polys)]


def mask(ka, row_a, kb, row_b, a_valid=True, b_valid=True) -> int:
    pa = points_of(ka, row_a, a_valid)
    if pa is None:
        return 0
    m = 0
    for p in set(pa):
        c = classify(p, kb, row_b, b_valid)
        if c is None:
            return 0
        m |= c
    d = DIM[kb]
    if d == 2:
        return m | B_OUTSIDE
    if d == 1:
        ms = _line_members(kb, row_b, b_valid)
        if any(a != b for mm in ms for a, b in zip(mm[:-1], mm[1:])):
            return m | B_OUTSIDE
        pb = {c for mm in ms for c in mm}
    else:
        pb = set(points_of(kb, row_b, b_valid))
    return m | (B_OUTSIDE if pb - set(pa) else 0)


def masks(ka, rows_a, kb, rows_b, rows=None, av=None, bv=None):
    out = np.zeros(len(rows_a), dtype=np.uint8)
    for i, ra in enumerate(rows_a):
        j = i if rows is None else int(rows[i])
        if j >= len(rows_b):
            continue
        out[i] = mask(ka, ra, kb, rows_b[j], av is None or av[i], bv is None or bv[j])
    return out


# ---- hand-derived cases: (name, points of A, dimension of B, members of B, mask) --------------------------------------------------------
# members of B: points (dimension 0), coordinate lists (1), polygons as lists of rings (2)

sq = R.sq
SQ4 = [sq(0, 0, 4, 4)]
DONUT = R.DONUT  # shell (0, 0) - (12, 12), hole (4, 4) - (8, 8)
HOLE_ON_SHELL = R.HOLE_ON_SHELL  # shell (0, 0) - (12, 12), a triangular hole with its apex (6, 0) on the shell
DIAMOND = [[(0, 2), (2, 0), (4, 2), (2, 4), (0, 2)]]
PARTS = R.PARTS  # a square and two triangles that touch it at (10, 5) and (5, 10)
RING, BOW = L.RING, L.BOW
SEG = [(0, 0), (4, 0)]

KNOWN = [
    ("a point in a square", [(2, 2)], 2, [SQ4], 9),
    ("a point outside a square", [(9, 9)], 2, [SQ4], 12),
    ("points inside and outside a square", [(2, 2), (9, 9)], 2, [SQ4], 13),
    ("a point inside a segment", [(2, 0)], 1, [SEG], 9),
    ("a point off a line", [(2, 1)], 1, [SEG], 12),
    ("the same point", [(1, 1)], 0, [(1, 1)], 1),
    ("two different points", [(1, 1)], 0, [(2, 2)], 12),
]

TIES = [
    # ---- polygons
    ("on a vertex", [(0, 0)], 2, [SQ4], 10),
    ("inside an edge", [(2, 0)], 2, [SQ4], 10),
    ("inside, on the boundary and outside", [(2, 2), (4, 3), (9, 9)], 2, [SQ4], 15),
    ("on a hole ring", [(4, 6)], 2, [DONUT], 10),
    ("on a vertex of a hole", [(8, 8)], 2, [DONUT], 10),
    ("strictly in a hole", [(6, 6)], 2, [DONUT], 12),
    ("between shell and hole", [(2, 6)], 2, [DONUT], 9),
    ("where a hole touches its shell", [(6, 0)], 2, [HOLE_ON_SHELL], 10),
    ("inside a hole that touches its shell", [(6, 2)], 2, [HOLE_ON_SHELL], 12),
    ("beside a hole that touches its shell", [(2, 1), (10, 1)], 2, [HOLE_ON_SHELL], 9),
    ("level with two vertices, inside", [(1, 2)], 2, [DIAMOND], 9),
    ("level with two vertices, outside", [(-1, 2)], 2, [DIAMOND], 12),
    ("on the line of a horizontal edge, outside", [(-2, 0), (6, 4)], 2, [SQ4], 12),
    ("where two members touch", [(10, 5)], 2, PARTS, 10),
    ("inside the second member", [(14, 5)], 2, PARTS, 9),
    ("inside one member, outside all", [(1, 1), (14, 12)], 2, PARTS, 13),
    # ---- lines
    ("at a line's end", [(0, 0)], 1, [SEG], 10),
    ("at both ends and inside", [(0, 0), (4, 0), (1, 0)], 1, [SEG], 11),
    ("a node where two members end: interior", [(0, 0)], 1, [[(-2, 0), (0, 0)], [(0, 0), (2, 1)]], 9),
    ("a node where three members end: boundary", [(0, 0)], 1, [[(-2, 0), (0, 0)], [(0, 0), (2, 1)], [(0, 0), (1, -2)]], 10),
    ("a member ends inside another's segment", [(2, 0)], 1, [SEG, [(2, 0), (2, 3)]], 10),
    ("the start of a closed ring line", [(0, 0)], 1, [RING], 9),
    ("inside a segment of a closed ring line", [(4, 2)], 1, [RING], 9),
    ("inside a ring line is off it", [(2, 2)], 1, [RING], 12),
    ("a self-crossing that is no coordinate", [(2, 2)], 1, [BOW], 9),
    ("the ends of a self-crossing line", [(0, 0), (0, 4)], 1, [BOW], 10),
    ("a member of equal coordinates, matched", [(1, 1)], 1, [[(1, 1), (1, 1)]], 1),
    ("a member of one coordinate, matched and more", [(1, 1), (3, 3)], 1, [[(1, 1)]], 5),
    ("two degenerate members, one matched", [(1, 1)], 1, [[(1, 1)], [(2, 2), (2, 2)]], 9),
    ("two degenerate members, both matched", [(2, 2), (1, 1)], 1, [[(1, 1)], [(2, 2), (2, 2)]], 1),
    ("a degenerate member beside a segment", [(7, 7)], 1, [SEG, [(7, 7)]], 9),
    ("a repeated coordinate inside a line", [(2, 2)], 1, [[(0, 0), (2, 2), (2, 2), (4, 0)]], 9),
    # ---- points
    ("equal as sets, duplicates and another order", [(1, 1), (2, 2), (1, 1)], 0, [(2, 2), (1, 1)], 1),
    ("a proper subset", [(1, 1)], 0, [(1, 1), (2, 2)], 9),
    ("a proper superset", [(1, 1), (2, 2)], 0, [(1, 1)], 5),
    ("a proper superset with duplicates in B", [(1, 1), (2, 2)], 0, [(1, 1), (1, 1)], 5),
    ("sets that overlap", [(1, 1), (2, 2)], 0, [(2, 2), (3, 3)], 13),
    ("sets apart, boxes that meet", [(1, 1), (3, 3)], 0, [(2, 2), (1, 3)], 12),
]


def as_a(kind, pts):
    if kind == PT:
        assert len(pts) == 1
        return pts[0]
    return list(pts)


def as_b(kind, ms):
    """members as a row of `kind`; MULTILINESTRING and MULTIPOLYGON rows get an empty member in front"""
    if kind in (PT, LS, PG):
        assert len(ms) == 1
        return ms[0] if kind == PT else list(ms[0])
    if kind == MPT:
        return list(ms)
    return [[]] + [list(m) for m in ms]


KINDS_OF_DIM = {0: (PT, MPT), 1: (LS, MLS), 2: (PG, MPG)}


def padded(kind, row, k):
    """the row scaled by k + 1 with k collinear vertices put into every segment or edge; a MULTIPOINT row repeats every point k + 1
    times instead (all sides scale alike: the answers stay)"""
    if k == 0:
        return row
    if kind == PT:
        return None if row is None else (row[0] * (k + 1), row[1] * (k + 1))
    if kind == MPT:
        return [(x * (k + 1), y * (k + 1)) for x, y in row for _ in range(k + 1)]
    if kind in (LS, MLS):
        return L.padded(kind, row, k)
    return R.padded(kind, row, k)


def placed(kind, row, offset, scale):
    """a row translated by an integer offset and then scaled by a power of two (exact in doubles)"""
    if kind == PT:
        return None if row is None else ((row[0] + offset[0]) * scale, (row[1] + offset[1]) * scale)
    if kind == MPT:
        return R.placed(LS, row, offset, scale)
    return R.placed(kind, row, offset, scale)


def case_columns(cases, ka, kb, pad=0):
    """(rows of A, rows of B, masks, names) of the cases that the two kinds can hold"""
    sel = [c for c in cases if kb in KINDS_OF_DIM[c[2]] and (ka == MPT or len(c[1]) == 1) and (kb in (MPT, MLS, MPG) or len(c[3]) == 1)]
    a = [padded(ka, as_a(ka, c[1]), pad) for c in sel]
    b = [padded(kb, as_b(kb, c[3]), pad) for c in sel]
    return a, b, np.array([c[4] for c in sel], dtype=np.uint8), [c[0] for c in sel]


# ---- random lattice columns ----------------------------------------------------------------------------------------------------------

LATTICE = [(x, y) for x in range(10) for y in range(10)]


def _pick(rng, pool, k):
    idx = rng.choice(len(pool), size=min(k, len(pool)), replace=False)
    return [pool[int(i)] for i in idx]


def _rewrite_ring(r, rng):
    """the same ring from another start, the other way round now and then"""
    v = r[:-1]
    s = int(rng.integers(0, len(v)))
    v = v[s:] + v[:s]
    if rng.random() < 0.5:
        v = v[::-1]
    return v + [v[0]]


def _random_polygon(rng):
    """a valid lattice polygon inside 0..9: a rectangle (now and then with a hole, or with a triangular hole whose apex sits on the
    shell) or a diamond"""
    style = int(rng.integers(0, 4))
    if style == 0:
        r = int(rng.integers(1, 4))
        cx, cy = int(rng.integers(r, 10 - r)), int(rng.integers(r, 10 - r))
        return [_rewrite_ring([(cx - r, cy), (cx, cy - r), (cx + r, cy), (cx, cy + r), (cx - r, cy)], rng)]
    if style == 1:
        x0, y0 = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        x1, y1 = x0 + int(rng.integers(5, 8)), y0 + int(rng.integers(5, 8))
        return [_rewrite_ring(sq(x0, y0, x1, y1), rng), _rewrite_ring(sq(x0 + 2, y0 + 2, x1 - 2, y1 - 2, cw=True), rng)]
    if style == 2:
        x0, y0 = int(rng.integers(0, 2)), int(rng.integers(0, 3))
        return [_rewrite_ring(sq(x0, y0, x0 + 8, y0 + 6), rng), _rewrite_ring([(x0 + 4, y0), (x0 + 2, y0 + 3), (x0 + 6, y0 + 3), (x0 + 4, y0)], rng)]
    x0, y0 = int(rng.integers(0, 7)), int(rng.integers(0, 7))
    return [_rewrite_ring(sq(x0, y0, int(rng.integers(x0 + 2, 10)), int(rng.integers(y0 + 2, 10))), rng)]


def _random_b(rng, kb, degenerate=False):
    d = DIM[kb]
    if d == 0:
        return _pick(rng, LATTICE, 1)[0] if kb == PT else [p for p in _pick(rng, LATTICE, int(rng.integers(1, 5))) for _ in range(int(rng.integers(1, 3)))]
    if d == 1:
        if degenerate:
            ms = [[p] * int(rng.integers(1, 3)) for p in _pick(rng, LATTICE, 1 if kb == LS else int(rng.integers(1, 3)))]
        else:
            a = L._walk(rng, int(rng.integers(2, 6)))
            ms = [a]
            if kb == MLS:
                style = int(rng.integers(0, 5))
                if style == 1:
                    ms.append(L._walk(rng, 3, start=a[-1]))  # two ends at one node: an interior point
                elif style == 2:
                    ms += [L._walk(rng, 2, start=a[-1]), L._walk(rng, 2, start=a[-1])]  # three: a boundary point
                elif style == 3:
                    ms.append(_pick(rng, LATTICE, 1) * 2)  # a degenerate member
                elif style == 4:
                    ms.append(L._walk(rng, 3, start=a[len(a) // 2]))
            elif rng.random() < 0.25 and len(a) > 2:
                ms = [a + [a[0]]]  # closed: no boundary
        if kb == LS:
            return ms[0]
        if rng.random() < 0.3:
            ms.insert(int(rng.integers(0, len(ms) + 1)), [])
        return ms
    if kb == PG:
        return _random_polygon(rng)
    first = _random_polygon(rng)
    xs = [p[0] for p in first[0]]
    row = [first]
    if max(xs) <= 6:  # a second member to the right of the first, now and then touching it at a vertex
        x0 = max(xs) + int(rng.integers(0, 2))
        ys = [p[1] for p in first[0] if p[0] == max(xs)]
        y = ys[0]
        row.append([[(x0, y), (9, max(0, y - 2)), (9, min(9, y + 2)), (x0, y)]])
    if rng.random() < 0.3:
        row.insert(int(rng.integers(0, len(row) + 1)), [])
    return row


def _pair_for(rng, ka, kb, target):
    """rows A, B built towards the mask `target` (the reference, not this construction, says what they are)"""
    d = DIM[kb]
    for _ in range(200):
        b = _random_b(rng, kb, degenerate=(d == 1 and target in (1, 5)))
        if d == 0 or (d == 1 and target in (1, 5)):
            pb = [b] if kb == PT else (sorted({p for m in L.members(kb, b) for p in m}) if d == 1 else sorted(set(b)))
            off = [p for p in LATTICE if p not in pb]
            if target == 1:
                if ka == PT and len(pb) > 1:
                    continue
                pa = list(pb)
            elif target == 5:
                pa = list(pb) + _pick(rng, off, int(rng.integers(1, 3)))
            elif target == 9:
                if len(pb) < 2:
                    continue
                pa = _pick(rng, pb, 1 if ka == PT else int(rng.integers(1, len(pb))))
            elif target == 12:
                pa = _pick(rng, off, 1 if ka == PT else int(rng.integers(1, 4)))
            else:
                if len(pb) < 2:
                    continue
                pa = _pick(rng, pb, int(rng.integers(1, len(pb)))) + _pick(rng, off, int(rng.integers(1, 3)))
        else:
            cls = {INTERIOR: [], BOUNDARY: [], EXTERIOR: []}
            for p in LATTICE:
                cls[classify(p, kb, b)].append(p)
            need = [bit for bit in (INTERIOR, BOUNDARY, EXTERIOR) if target & bit]
            if any(not cls[bit] for bit in need):
                continue
            pa = [p for bit in need for p in _pick(rng, cls[bit], 1 if ka == PT else int(rng.integers(1, 3)))]
        if ka == PT:
            if len(pa) != 1:
                continue
            return pa[0], b
        pa = [p for p in pa for _ in range(int(rng.integers(1, 3)))]  # duplicates
        rng.shuffle(pa)
        return [tuple(int(c) for c in p) for p in pa], b
    raise AssertionError(f"no pair built for {NAMES[ka]} x {NAMES[kb]} towards mask {target}")


@lru_cache(maxsize=None)
def random_columns(ka, kb, n_rows=96):
    """(rows of A, rows of B, masks): geometries on the 10 x 10 lattice and points picked from the lattice points inside, on and
    outside them, row i built towards the i-th of the masks the pair of kinds can have, in turn"""
    rng = np.random.default_rng(5000 + 10 * ka + kb)
    targets = reachable(ka, kb)
    A, B = [], []
    for i in range(n_rows):
        a, b = _pair_for(rng, ka, kb, targets[i % len(targets)])
        A.append(a)
        B.append(b)
    return A, B, masks(ka, A, kb, B)


def honest(ka, kb, want) -> bool:
    """the condition that keeps the random tests honest: every mask the pair of kinds can have occurs in at least 3 rows, and none
    fills more than half of them"""
    count = Counter(int(m) for m in want)
    return set(count) == set(reachable(ka, kb)) and min(count.values()) >= 3 and max(count.values()) <= len(want) // 2


# ---- the join fixture ------------------------------------------------------------------------------------------------------------------


def _coords(kind, row):
    if row is None:
        return []
    if kind == PT:
        return [row]
    if kind in (MPT, LS):
        return list(row)
    if kind in (MLS, PG):
        return [p for s in row for p in s]
    return [p for g in row for s in g for p in s]


def _moved(kind, row, o):
    return placed(kind, row, o, 1)


def mask_table(ka, rows_a, av, kb, rows_b, bv):
    """the exact masks of every row of A against every row of B (two usable rows whose boxes are apart: 12)"""
    big = 10**9
    ua = np.array([usable(ka, r, av[i]) for i, r in enumerate(rows_a)])
    ub = np.array([usable(kb, r, bv[j]) for j, r in enumerate(rows_b)])

    def boxes(kind, rows, ok):
        out = []
        for i, r in enumerate(rows):
            c = _coords(kind, r) if ok[i] else []
            out.append((min(x for x, _ in c), min(y for _, y in c), max(x for x, _ in c), max(y for _, y in c)) if c else (big, big, -big, -big))
        return np.array(out, dtype=np.float64)

    ba, bb = boxes(ka, rows_a, ua), boxes(kb, rows_b, ub)
    table = np.where(ua[:, None] & ub[None, :], EXTERIOR | B_OUTSIDE, 0).astype(np.uint8)
    for j in np.nonzero(ub)[0]:
        near = (ba[:, 0] <= bb[j, 2]) & (ba[:, 2] >= bb[j, 0]) & (ba[:, 1] <= bb[j, 3]) & (ba[:, 3] >= bb[j, 1])
        for i in np.nonzero(near & ua)[0]:
            table[i, j] = mask(ka, rows_a[i], kb, rows_b[j])
    return table


@lru_cache(maxsize=None)
def join_fixture(ka=PT, kb=PG, n=300):
    """a column of about n punctual rows and one of about n rows of kind `kb` over a 60 x 60 domain: every B row is a lattice geometry
    moved somewhere, two thirds of the A rows are points picked inside, on and outside one of them, the rest anywhere; some A rows
    appear twice (duplicates for the self-join) and some B rows repeat an A row's points (punctual B: equals); a null row and an empty
    row on either side.  Returns (A rows, A validity, B rows, B validity, table[n, n] of exact masks (A, B), table of A against A)."""
    rng = np.random.default_rng(991 + 10 * ka + kb)
    B, A = [], []
    for j in range(n):
        o = (int(rng.integers(0, 50)), int(rng.integers(0, 50)))
        B.append(_moved(kb, _random_b(rng, kb, degenerate=(DIM[kb] == 1 and j % 11 == 0)), o))
    for i in range(n):
        if i % 3 < 2:
            j = int(rng.integers(0, n))
            c = _coords(kb, B[j])
            x0, y0 = min(x for x, _ in c), min(y for _, y in c)
            near = [(x0 + dx, y0 + dy) for dx in range(-1, 9) for dy in range(-1, 9)]
            pts = _pick(rng, near, 1 if ka == PT else int(rng.integers(1, 5)))
            if i % 6 == 0:
                pts = _pick(rng, sorted(set(c)), len(pts))  # on coordinates of B
        else:
            pts = [(int(rng.integers(0, 60)), int(rng.integers(0, 60))) for _ in range(1 if ka == PT else int(rng.integers(1, 4)))]
        A.append(pts[0] if ka == PT else pts)
    for i in range(40, 60):
        A[i] = A[i - 20] if i % 2 else (A[i - 20] if ka == PT else A[i - 20][::-1] + A[i - 20][:1])  # duplicates, written differently
    if DIM[kb] == 0:
        for j in range(100, 130):
            pts = _coords(ka, A[j])
            B[j] = pts[0] if kb == PT else (pts + pts[:1] if j % 2 else pts + [(pts[0][0] + 1, pts[0][1])])
    av, bv = np.ones(n, dtype=bool), np.ones(n, dtype=bool)
    av[31] = bv[52] = False
    A[23] = None if ka == PT else []
    B[40] = None if kb == PT else []
    return A, av, B, bv, mask_table(ka, A, av, kb, B, bv), mask_table(ka, A, av, ka, A, av)


def expected_pairs(table, pred: str, dim_b: int, transpose=False):
    """(pairs sorted by (l, r), counts per left row, masks per pair) of a predicate over a mask table [A, B]; transpose: B is the left
    column, so the table is turned and `pred` is what the left rows are asked against the right ones"""
    name = TRANSPOSED.get(pred, pred) if transpose else pred
    hit = np.vectorize(lambda m: PREDICATES[name](int(m), dim_b), otypes=[bool])(table)
    if transpose:
        hit, table = hit.T, table.T
    ll, rr = np.nonzero(hit)
    return np.stack([ll, rr], axis=1).astype(np.uint32), np.bincount(ll, minlength=table.shape[0]).astype(np.uint32), table[ll, rr]


def zigzag(n=400):
    """a zigzag line of n coordinates"""
    return [(2 * i, (i % 2) * 3 + (i % 4 == 3)) for i in range(n)]


def big_donut(n=300):
    """a polygon of about n coordinates with a hole: a rectangle whose lower side is a saw of teeth one unit deep, a square hole"""
    m = n - 10
    w = 2 * m
    shell = [(2 * i, -(i % 2)) for i in range(m + 1)] + [(w, 300), (0, 300), (0, 0)]
    return [shell, sq(100, 100, 200, 200, cw=True)]
