"""Exact reference of the polygon x polygon relation mask (gpk_polygon_relation, csrc/gpk_polyrel.h) and its fixtures.

The mask of two polygonal geometries A and B (closed regular sets): bit 1 — the interiors share a point, 2 — a ring of A and a ring of B
share a point, 4 — A's interior has a point in B's exterior, 8 — B's interior has a point in A's exterior.

The three area bits are decided from rational SAMPLE POINTS OF AREAS, never from the side of a shared boundary piece (which is what
the kernel uses).  S = the x coordinates of all vertices and of all exact edge x edge intersection points of A with B.  Inside an open
slab between two consecutive values of S no edge starts, ends or meets another, so the edges that span the slab are ordered from
bottom to top and cut it into trapezoids; every face of the arrangement of all edges meets some slab in such trapezoids.  On the
slab's middle line x = xm the edges are evaluated exactly (Fractions) and sorted; a sample point between two consecutive edges lies in
A's interior when the number of A's edges below it is odd (even-odd over all rings of all members: holes lie in their shells and
members do not overlap), the same for B.  tests/test_polyrel_ref.py checks the very same sample points with
exact_predicates._rational_pos.  BOUNDARIES: some edge of A meets some edge of B (closed segments, exact integers).
All fixtures live on small integer lattices.

Rows are what tests/exact_ref.column takes: a POLYGON row is a list of rings, a MULTIPOLYGON row a list of polygons."""
from __future__ import annotations

from fractions import Fraction
from functools import lru_cache

import numpy as np

from tests import exact_predicates as E
from tests import relation_ref as R

PG, MPG = R.PG, R.MPG
INTERIORS, BOUNDARIES, A_OUTSIDE, B_OUTSIDE = 1, 2, 4, 8
FAMILIES = [(PG, PG), (PG, MPG), (MPG, PG), (MPG, MPG)]
NAMES = R.NAMES
REACHABLE = (3, 5, 7, 9, 11, 12, 13, 14, 15)

# the predicates over the mask, as include/geopolars_hip.h states them
PREDICATES = {
    "intersects": lambda m: (m & 3) != 0,
    "disjoint": lambda m: m != 0 and not (m & 3),
    "touches": lambda m: bool(m & 2) and not (m & 1),
    "overlaps": lambda m: (m & 13) == 13,
    "within": lambda m: bool(m & 1) and not (m & 4),
    "contains": lambda m: bool(m & 1) and not (m & 8),
    "equals": lambda m: bool(m & 1) and not (m & 12),
    "contains_properly": lambda m: (m & 11) == 1,
    "crosses": lambda m: False,
}
PREDICATES["covered_by"] = PREDICATES["within"]
PREDICATES["covers"] = PREDICATES["contains"]
PRED_IDS = {"intersects": 0, "within": 1, "contains": 2, "touches": 3, "overlaps": 4, "equals": 5, "contains_properly": 6}  # GPK_PP_PRED_*


def swapped(m):
    """mask(B, A) from mask(A, B): bits 4 and 8 change places"""
    m = np.asarray(m)
    return (m & 3) | ((m & 4) << 1) | ((m & 8) >> 1)


def usable(kind, row, valid=True):
    """the integer polygons of a usable row, else None (the row rules of the header)"""
    if not valid or row is None:
        return None
    polys = R.row_polys(kind, row)
    if not polys or not all(R._ring_usable(r) for p in polys for r in p):
        return None
    return [[R._int_ring(r) for r in p] for p in polys]


def _meet(p, q, a, b):
    """the x coordinate (Fraction) of the single point where the closed segments pq and ab meet, True when they are collinear and
    share at least a point (the ends of the shared piece are vertices), None when they do not meet"""
    d, e, ap = (q[0] - p[0], q[1] - p[1]), (b[0] - a[0], b[1] - a[1]), (a[0] - p[0], a[1] - p[1])
    den = d[0] * e[1] - d[1] * e[0]
    if den != 0:
        t, u = Fraction(ap[0] * e[1] - ap[1] * e[0], den), Fraction(ap[0] * d[1] - ap[1] * d[0], den)
        return p[0] + t * d[0] if 0 <= t <= 1 and 0 <= u <= 1 else None
    if ap[0] * d[1] - ap[1] * d[0] != 0:
        return None
    k = 0 if d[0] != 0 else 1
    return True if max(min(p[k], q[k]), min(a[k], b[k])) <= min(max(p[k], q[k]), max(a[k], b[k])) else None


def area_samples(ea, eb):
    """(boundaries, samples): whether an edge of `ea` meets an edge of `eb`, and one rational point (x, y, in A, in B) in every
    trapezoid of every slab that lies between two edges"""
    xs = {Fraction(p[0]) for e in ea + eb for p in e}
    boundaries = False
    for p, q in ea:
        lo, hi = (min(p[0], q[0]), min(p[1], q[1])), (max(p[0], q[0]), max(p[1], q[1]))
        for a, b in eb:
            if max(a[0], b[0]) < lo[0] or min(a[0], b[0]) > hi[0] or max(a[1], b[1]) < lo[1] or min(a[1], b[1]) > hi[1]:
                continue
            x = _meet(p, q, a, b)
            if x is None:
                continue
            boundaries = True
            if x is not True:
                xs.add(x)
    xs = sorted(xs)
    out = []
    for x0, x1 in zip(xs, xs[1:]):
        xm = (x0 + x1) / 2
        ys = []
        for which, edges in ((0, ea), (1, eb)):
            for p, q in edges:
                if min(p[0], q[0]) < xm < max(p[0], q[0]):
                    ys.append((p[1] + (q[1] - p[1]) * (xm - p[0]) / (q[0] - p[0]), which))
        ys.sort()
        below = [0, 0]
        for k, (y, which) in enumerate(ys):
            below[which] ^= 1
            if k + 1 < len(ys) and ys[k + 1][0] != y and (below[0] or below[1]):
                out.append((xm, (y + ys[k + 1][0]) / 2, bool(below[0]), bool(below[1])))
    return boundaries, out


def mask(ka, row_a, kb, row_b, a_valid=True, b_valid=True) -> int:
    """the exact mask of one pair of rows; 0 for an unusable row or an invalid ring on either side"""
    pa, pb = usable(ka, row_a, a_valid), usable(kb, row_b, b_valid)
    if pa is None or pb is None:
        return 0
    boundaries, samples = area_samples(E._edges([r for p in pa for r in p]), E._edges([r for p in pb for r in p]))
    m = BOUNDARIES if boundaries else 0
    for _, _, ia, ib in samples:
        m |= INTERIORS if ia and ib else (A_OUTSIDE if ia else B_OUTSIDE)
    return m


def masks(ka, rows_a, kb, rows_b, rows=None, av=None, bv=None):
    out = np.zeros(len(rows_a), dtype=np.uint8)
    for i, ra in enumerate(rows_a):
        j = i if rows is None else int(rows[i])
        if j < len(rows_b):
            out[i] = mask(ka, ra, kb, rows_b[j], av is None or bool(av[i]), bv is None or bool(bv[j]))
    return out


# ---- the second derivation: the kernel's argument, on rationals ------------------------------------------------------------------------


def _shoelace(r):
    return sum(int(r[i, 0]) * int(r[i + 1, 1]) - int(r[i + 1, 0]) * int(r[i, 1]) for i in range(len(r) - 1))


def _hand_edges(polys):
    """(p, q, interior on the left) for every edge: the left of a counter-clockwise shell or of a clockwise hole"""
    return [(p, q, (_shoelace(r) > 0) != (k > 0)) for poly in polys for k, r in enumerate(poly) for p, q in E._edges([r])]


def side_bits(pa, pb):
    """INTERIORS for an overlap piece of positive length with both interiors on one hand, A_OUTSIDE | B_OUTSIDE for opposite hands"""
    bits = 0
    for p, q, la in _hand_edges(pa):
        d = (q[0] - p[0], q[1] - p[1])
        for a, b, lb in _hand_edges(pb):
            e = (b[0] - a[0], b[1] - a[1])
            if d[0] * e[1] - d[1] * e[0] != 0 or (a[0] - p[0]) * d[1] - (a[1] - p[1]) * d[0] != 0:
                continue
            k = 0 if d[0] != 0 else 1
            if max(min(p[k], q[k]), min(a[k], b[k])) >= min(max(p[k], q[k]), max(a[k], b[k])):
                continue
            same_way = d[0] * e[0] + d[1] * e[1] > 0
            bits |= INTERIORS if (la == lb) == same_way else A_OUTSIDE | B_OUTSIDE
    return bits


def mask_by_walks(ka, row_a, kb, row_b) -> int:
    """the combination csrc/gpk_polyrel.h uses: the rings of A as a MULTILINESTRING against B, and back, plus the side rule"""
    pa, pb = usable(ka, row_a), usable(kb, row_b)
    if pa is None or pb is None:
        return 0
    rings = lambda polys: [[tuple(int(c) for c in v) for v in r] for p in polys for r in p]  # noqa: E731
    m_ab, m_ba = R.mask(R.MLS, rings(pa), kb, row_b), R.mask(R.MLS, rings(pb), ka, row_a)
    side = side_bits(pa, pb)
    m = m_ab & 2
    m |= INTERIORS if (m_ab & 1) or (m_ba & 1) or (side & INTERIORS) else 0
    m |= A_OUTSIDE if (m_ab & 4) or (m_ba & 1) or (side & A_OUTSIDE) else 0
    m |= B_OUTSIDE if (m_ba & 4) or (m_ab & 1) or (side & B_OUTSIDE) else 0
    return m


# ---- known answers and ties ------------------------------------------------------------------------------------------------------------

sq = R.sq
S10 = sq(0, 0, 10, 10)
DONUT = R.DONUT  # shell (0, 0) - (12, 12), hole (4, 4) - (8, 8)
# a hole whose vertex (6, 0) is a vertex of the shell too
PINCHED = [[(0, 0), (6, 0), (12, 0), (12, 12), (0, 12), (0, 0)], [(6, 0), (3, 4), (9, 4), (6, 0)]]
# two parts of A and two parts of B meet in (10, 10), in complementary sectors
FAN_A = [[[(10, 10), (4, 13), (4, 7), (10, 10)]], [[(10, 10), (16, 7), (16, 13), (10, 10)]]]
FAN_B = [[[(10, 10), (13, 16), (7, 16), (10, 10)]], [[(10, 10), (7, 4), (13, 4), (10, 10)]]]
B_TWO = [[sq(0, 0, 4, 4)], [sq(10, 0, 22, 12), sq(14, 4, 18, 8, cw=True)]]  # a square, and a donut

# (name, A, B, mask): A and B as lists of polygons; a one-member list is a POLYGON row as well
KNOWN = [
    ("far apart", [[S10]], [[sq(40, 40, 50, 50)]], 12),
    ("apart with boxes that meet", [[[(0, 0), (4, 0), (0, 4), (0, 0)]]], [[[(5, 5), (5, 1), (1, 5), (5, 5)]]], 12),
    ("proper overlap", [[S10]], [[sq(5, 5, 15, 15)]], 15),
    ("A holds B", [[S10]], [[sq(2, 2, 5, 5)]], 5),
    ("B holds A", [[sq(2, 2, 5, 5)]], [[S10]], 9),
    ("B in A's hole", [DONUT], [[sq(5, 5, 7, 7)]], 12),
    ("B covers A's hole, inside A's shell, no ring contact", [DONUT], [[sq(3, 3, 9, 9)]], 13),
    ("A covers B's hole, inside B's shell, no ring contact", [[sq(3, 3, 9, 9)]], [DONUT], 13),
    ("B holds the donut A", [DONUT], [[sq(-2, -2, 14, 14)]], 9),
    ("two members of A, one in B", [[sq(1, 1, 3, 3)], [sq(20, 20, 23, 23)]], [[S10]], 13),
]
TIES = [
    ("equal, same start", [[S10]], [[S10]], 3),
    ("equal, rotated start", [[S10]], [[[(10, 0), (10, 10), (0, 10), (0, 0), (10, 0)]]], 3),
    ("equal, reversed winding", [[S10]], [[sq(0, 0, 10, 10, cw=True)]], 3),
    ("equal, an extra collinear vertex", [[S10]], [[[(0, 0), (5, 0), (10, 0), (10, 10), (0, 10), (0, 0)]]], 3),
    ("equal donuts, hole rotated and reversed", [DONUT], [[sq(0, 0, 12, 12, cw=True), [(8, 8), (8, 4), (4, 4), (4, 8), (8, 8)]]], 3),
    ("equal multipolygons, parts in another order", [[sq(0, 0, 4, 4)], [sq(6, 6, 9, 9)]], [[sq(6, 6, 9, 9)], [sq(0, 0, 4, 4)]], 3),
    ("A fills B's hole exactly", [[sq(4, 4, 8, 8)]], [DONUT], 14),
    ("A in B's hole, free", [[sq(5, 5, 7, 7)]], [DONUT], 12),
    ("A in B's hole, touching it at a vertex", [[[(4, 4), (6, 5), (5, 6), (4, 4)]]], [DONUT], 14),
    ("neighbours sharing a whole edge", [[S10]], [[sq(10, 0, 20, 10)]], 14),
    ("neighbours sharing part of an edge, no shared vertex", [[S10]], [[sq(10, 2, 20, 8)]], 14),
    ("neighbours sharing one vertex", [[S10]], [[sq(10, 10, 20, 20)]], 14),
    ("a vertex of B inside an edge of A", [[S10]], [[[(10, 5), (15, 2), (15, 8), (10, 5)]]], 14),
    ("A strictly inside B", [[sq(2, 2, 5, 5)]], [[S10]], 9),
    ("A inside B, sharing a boundary piece", [[sq(0, 2, 5, 5)]], [[S10]], 11),
    ("B strictly inside A", [[S10]], [[sq(2, 2, 5, 5)]], 5),
    ("B inside A, sharing a boundary piece", [[S10]], [[sq(0, 2, 5, 5)]], 7),
    ("the filled shell A against the donut B", [[sq(0, 0, 12, 12)]], [DONUT], 7),
    ("the donut A against its filled shell B", [DONUT], [[sq(0, 0, 12, 12)]], 11),
    ("overlap by proper crossing", [[S10]], [[sq(5, 5, 15, 15)]], 15),
    ("overlap, rings meet only at vertices", [[S10]], [[[(0, 0), (10, 10), (15, -5), (0, 0)]]], 15),
    ("A1 equals B1, A2 fills B2's hole", [[sq(0, 0, 4, 4)], [sq(14, 4, 18, 8)]], B_TWO, 15),
    ("A1 equals B1, B has a far second part", [[sq(0, 0, 4, 4)]], [[sq(0, 0, 4, 4)], [sq(30, 30, 35, 35)]], 11),
    ("parts of A and parts of B meet in one point, complementary sectors", FAN_A, FAN_B, 14),
    ("pinched hole of B: A outside, at the pinch", [[[(6, 0), (9, -5), (3, -5), (6, 0)]]], [PINCHED], 14),
    ("pinched hole of B: A in the hole, at the pinch", [[[(6, 0), (7, 3), (5, 3), (6, 0)]]], [PINCHED], 14),
    ("pinched hole of B: A in the interior, at the pinch", [[[(6, 0), (2, 1), (1, 3), (6, 0)]]], [PINCHED], 11),
    ("pinched hole of B: A fills the hole", [[[(6, 0), (9, 4), (3, 4), (6, 0)]]], [PINCHED], 14),
    ("pinched hole of B: A through the pinch from outside into the hole", [[[(6, 0), (7, 3), (5, 3), (6, 0)]], [[(6, 0), (9, -5), (3, -5), (6, 0)]]], [PINCHED], 14),
]


def as_row(kind, polys):
    """a list of polygons as a row of `kind`; a MULTIPOLYGON row gets an empty member in front"""
    if kind == PG:
        assert len(polys) == 1
        return polys[0]
    return [[]] + [list(p) for p in polys]


def case_columns(cases, ka, kb, pad=0):
    """(rows of A, rows of B, masks, names) of the cases that the two kinds can hold, every ring padded with `pad` collinear vertices
    an edge (both sides scale alike: the answers stay)"""
    sel = [c for c in cases if (ka == MPG or len(c[1]) == 1) and (kb == MPG or len(c[2]) == 1)]
    a = [R.padded(ka, as_row(ka, c[1]), pad) for c in sel]
    b = [R.padded(kb, as_row(kb, c[2]), pad) for c in sel]
    return a, b, np.array([c[3] for c in sel], dtype=np.uint8), [c[0] for c in sel]


# ---- random lattice columns ----------------------------------------------------------------------------------------------------------


def _moved(poly, dx, dy):
    return [[(x + dx, y + dy) for x, y in r] for r in poly]


def _rewritten(poly, rng):
    """the same polygon written differently: rings started elsewhere, some reversed"""
    out = []
    for r in poly:
        v = list(r[:-1])
        k = int(rng.integers(0, len(v)))
        v = v[k:] + v[:k]
        if rng.random() < 0.5:
            v = v[::-1]
        out.append(v + [v[0]])
    return out


def _partner(a, Rad, style, rng):
    """a valid polygon B for the polygon A (centred at the origin, radius Rad): 0 — another star nearby, 1 — A itself rewritten,
    2 — a small star near the centre, 3 — far away, 4 — the triangle of three of A's shell vertices, 5 — A moved by its own width,
    6 — the filling of A's hole (else style 4), 7 — the box of A's shell"""
    shell = a[0]
    if style == 1:
        return _rewritten(a, rng)
    if style == 3:
        return R._random_polygon(4 * Rad, 3 * Rad, Rad, int(rng.integers(4, 9)), 0, rng)
    if style == 6 and len(a) > 1:
        return [a[1][::-1]]
    if style in (4, 6):
        for _ in range(50):
            i, j, k = sorted(rng.choice(len(shell) - 1, 3, replace=False))
            t = [shell[i], shell[j], shell[k], shell[i]]
            if R.polygon_valid(PG, [t]):
                return [t]
    if style == 5:
        xs = [x for x, _ in shell]
        return _moved(a, max(xs) - min(xs), 0)
    if style == 7:
        xs, ys = [x for x, _ in shell], [y for _, y in shell]
        return [sq(min(xs), min(ys), max(xs), max(ys))]
    if style == 2:
        return R._random_polygon(int(rng.integers(-1, 2)), int(rng.integers(-1, 2)) + (Rad // 2 if len(a) > 1 else 0), 2, 4, 0, rng)
    return R._random_polygon(int(rng.integers(-Rad, Rad + 1)), int(rng.integers(-Rad, Rad + 1)), int(rng.integers(4, 14)), int(rng.integers(4, 10)), 0, rng)


@lru_cache(maxsize=None)
def random_columns(ka, kb, n_rows=64):
    """(rows of A, rows of B, masks): lattice star polygons of at most 8 distinct vertices a ring, some with a hole, against partners
    built to coincide with them in many ways; MULTIPOLYGON rows carry a second member (now and then the same on both sides) and
    empty members"""
    rng = np.random.default_rng(2000 + 10 * ka + kb)
    A, B = [], []
    for i in range(n_rows):
        Rad = int(rng.integers(10, 20))
        a = R._random_polygon(0, 0, Rad, int(rng.choice([4, 5, 7, 9])), int(i % 3 == 0), rng)
        b = _partner(a, Rad, i % 8, rng)
        ra, rb = [a], [b]
        extra = R._random_polygon(5 * Rad, 0, 5, int(rng.integers(4, 8)), 0, rng)
        if ka == MPG and i % 2:
            ra.append(extra)
        if kb == MPG and i % 4 >= 2:
            rb.append(_rewritten(extra, rng) if i % 8 >= 4 else _moved(extra, 3, 2))
        for kind, row in ((ka, ra), (kb, rb)):
            if kind == MPG and i % 3 == 1:
                row.insert(int(rng.integers(0, len(row) + 1)), [])
        A.append(a if ka == PG else ra)
        B.append(b if kb == PG else rb)
    return A, B, masks(ka, A, kb, B)


# ---- the join fixture ------------------------------------------------------------------------------------------------------------------


def _boxes(kind, rows, ok):
    inf = 10**9
    return np.array([R._box_of([p[0] for p in R.row_polys(kind, r)]) if ok[i] else (inf, inf, -inf, -inf) for i, r in enumerate(rows)])


def mask_table(ka, rows_a, av, kb, rows_b, bv):
    """the exact masks of every row of A against every row of B (pairs of usable rows whose boxes are apart: 12)"""
    ua = np.array([usable(ka, r, av[i]) is not None for i, r in enumerate(rows_a)])
    ub = np.array([usable(kb, r, bv[j]) is not None for j, r in enumerate(rows_b)])
    ba, bb = _boxes(ka, rows_a, ua), _boxes(kb, rows_b, ub)
    table = np.where(ua[:, None] & ub[None, :], A_OUTSIDE | B_OUTSIDE, 0).astype(np.uint8)
    for j in np.nonzero(ub)[0]:
        near = (ba[:, 0] <= bb[j, 2]) & (ba[:, 2] >= bb[j, 0]) & (ba[:, 1] <= bb[j, 3]) & (ba[:, 3] >= bb[j, 1])
        for i in np.nonzero(near & ua)[0]:
            table[i, j] = mask(ka, rows_a[i], kb, rows_b[j])
    return table


@lru_cache(maxsize=None)
def join_fixture(ka=PG, kb=PG, n=300):
    """two columns of about n small polygons over a 600 x 600 lattice.  Both hold the same block of 6 x 6 square tiles (adjacency:
    shared edges and shared corners; equal rows across the columns) and a polygon with a hole that covers the whole domain (a row
    with hundreds of candidates on either side); the right column repeats some left rows rewritten; a null row and an empty row on
    either side.  Returns (left, left validity, right, right validity, table[n, n] of exact masks, table of left against left)."""
    rng = np.random.default_rng(99 + ka + kb)
    tiles = [[sq(620 + 10 * i, 10 * j, 630 + 10 * i, 10 + 10 * j)] for i in range(6) for j in range(6)]
    cover = [sq(-5, -5, 700, 700), sq(300, 300, 320, 320, cw=True)]

    def column(kind, seed_rows):
        rows = []
        for j in range(n - len(tiles) - len(seed_rows)):
            cx, cy = int(rng.integers(20, 580)), int(rng.integers(20, 580))
            p = R._random_polygon(cx, cy, int(rng.integers(5, 25)), int(rng.choice([4, 5, 9])), int(j % 7 == 0), rng)
            if kind == MPG and j % 3 == 0:
                rows.append([[], p] if j % 2 else [p, R._random_polygon(cx, cy + 80, 6, 5, 0, rng)])
            else:
                rows.append(p if kind == PG else [p])
        rows += [t if kind == PG else [t] for t in tiles]
        rows += [r if kind == PG else [r] for r in seed_rows]
        return rows

    left = column(ka, [])
    left[5] = cover if ka == PG else [cover]
    copies = [_rewritten(R.row_polys(ka, left[i])[0], rng) for i in range(60, 72)]
    right = column(kb, copies)
    right[17] = cover if kb == PG else [cover]
    left[23], right[40] = [], []
    lv, rv = np.ones(n, dtype=bool), np.ones(n, dtype=bool)
    lv[31] = rv[52] = False
    return left, lv, right, rv, mask_table(ka, left, lv, kb, right, rv), mask_table(ka, left, lv, ka, left, lv)


def expected_pairs(table, pred: str):
    """(pairs sorted by (l, r), counts per left row, masks per pair) of a predicate over a mask table [left, right]"""
    hit = np.vectorize(PREDICATES[pred], otypes=[bool])(table)
    ll, rr = np.nonzero(hit)
    return np.stack([ll, rr], axis=1).astype(np.uint32), np.bincount(ll, minlength=table.shape[0]).astype(np.uint32), table[ll, rr]


def all_fixture_rows():
    """(kind, row) of every polygon row of every fixture: each must pass relation_ref.polygon_valid"""
    for cases in (KNOWN, TIES):
        for _, a, b, _ in cases:
            yield MPG, a
            yield MPG, b
    for ka, kb in FAMILIES:
        A, B, _ = random_columns(ka, kb)
        for r in A:
            yield ka, r
        for r in B:
            yield kb, r
    for ka, kb in ((PG, PG), (MPG, MPG)):
        left, lv, right, rv, _, _ = join_fixture(ka, kb)
        for kind, rows in ((ka, left), (kb, right)):
            for i, r in enumerate(rows):
                if len(r):
                    yield kind, r
