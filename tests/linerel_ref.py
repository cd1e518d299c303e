"""The exact rational reference of the line x line relation mask (gpk_line_relation, include/geopolars_hip.h), built differently from
the kernel: an ARRANGEMENT.  Every segment of both rows is split at every point where it meets a segment of the other row and at every
coordinate of either row that lies on it; every node and the midpoint of every elementary piece is classified as on A, on B or on
both, with `fractions.Fraction` throughout, and the seven bits are read off that classification with the mod-2 boundary sets.

    mask(ka, row_a, kb, row_b)      the arrangement reference
    mask_by_rules(...)              the kernel's formulation (coordinates, proper crossings, shared pieces, the covering walk) in
                                    plain Python — tests/test_linerel_ref.py holds the two against each other
    KNOWN, TIES                     hand-derived cases: (name, members of A, members of B, mask)
    case_columns, random_columns, join_fixture, mask_table, expected_pairs   fixtures, as tests/polyrel_ref.py has them

A row is a list of members (a LINESTRING row: one member), a member a list of (x, y).  Coordinates are exact in doubles."""
from __future__ import annotations

import math
from collections import Counter
from fractions import Fraction
from functools import lru_cache

import numpy as np

from geopolars_amd import _abi
from tests import relation_ref as R

LS, MLS = _abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING
FAMILIES = [(LS, LS), (LS, MLS), (MLS, LS), (MLS, MLS)]
NAMES = {LS: "ls", MLS: "mls"}
INTERIORS, SHARED_PIECE, INT_BND, BND_INT, BND_BND, A_OUTSIDE, B_OUTSIDE = 1, 2, 4, 8, 16, 32, 64
PLACEMENTS, placed = R.PLACEMENTS, R.placed

# the DE-9IM predicates of dimension 1 / 1 over the mask
PREDICATES = {
    "intersects": lambda m: bool(m & 31),
    "disjoint": lambda m: m != 0 and not (m & 31),
    "touches": lambda m: bool(m & 28) and not (m & 1),
    "crosses": lambda m: bool(m & 1) and not (m & 2),
    "overlaps": lambda m: bool(m & 2) and bool(m & 32) and bool(m & 64),
    "within": lambda m: bool(m & 1) and not (m & 32),
    "contains": lambda m: bool(m & 1) and not (m & 64),
    "covered_by": lambda m: bool(m & 31) and not (m & 32),
    "covers": lambda m: bool(m & 31) and not (m & 64),
    "equals": lambda m: bool(m & 1) and not (m & 96),
}
PRED_IDS = {"intersects": 0, "within": 1, "contains": 2, "covered_by": 3, "covers": 4, "crosses": 5, "touches": 6, "overlaps": 7, "equals": 8}  # GPK_LL_PRED_*


def swapped(m):
    """mask(B, A) from mask(A, B): 4 <-> 8 and 32 <-> 64"""
    m = np.asarray(m, dtype=np.uint8)
    return ((m & 19) | ((m & 4) << 1) | ((m & 8) >> 1) | ((m & 32) << 1) | ((m & 64) >> 1)).astype(np.uint8)


def members(kind, row):
    return [list(row)] if kind == LS else [list(s) for s in row]


def usable(kind, row, valid=True):
    """the non-empty members of a usable row as Fraction points, else None (null, no coordinate, a NaN or infinite coordinate)"""
    if not valid:
        return None
    ms = [m for m in members(kind, row) if len(m)]
    if not ms or any(not (math.isfinite(x) and math.isfinite(y)) for m in ms for x, y in m):
        return None
    return [[(Fraction(x), Fraction(y)) for x, y in m] for m in ms]


def _orient(a, b, c):
    d = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    return (d > 0) - (d < 0)


def _in_box(p, s):
    return s[2] <= p[0] <= s[3] and s[4] <= p[1] <= s[5]


class _Row:
    """points, non-degenerate segments (a, b, lx, hx, ly, hy) and the mod-2 boundary set of a usable row"""

    def __init__(self, ms):
        self.pts = {p for m in ms for p in m}
        self.segs = [(a, b, min(a[0], b[0]), max(a[0], b[0]), min(a[1], b[1]), max(a[1], b[1])) for m in ms for a, b in zip(m[:-1], m[1:]) if a != b]
        ends = Counter()
        for m in ms:
            ends[m[0]] += 1
            ends[m[-1]] += 1
        self.bnd = {p for p, k in ends.items() if k % 2}
        self.ends = [p for m in ms for p in (m[0], m[-1])]

    def has(self, p):
        return p in self.pts or any(_in_box(p, s) and _orient(s[0], s[1], p) == 0 for s in self.segs)


def _meet_point(s, t):
    """the single point two non-degenerate segments share, None when they share nothing or a piece (whose ends are coordinates)"""
    if s[3] < t[2] or s[2] > t[3] or s[5] < t[4] or s[4] > t[5]:
        return None
    a, b, c, d = s[0], s[1], t[0], t[1]
    rx, ry, sx, sy = b[0] - a[0], b[1] - a[1], d[0] - c[0], d[1] - c[1]
    den = rx * sy - ry * sx
    qx, qy = c[0] - a[0], c[1] - a[1]
    if den == 0:
        return None  # parallel: nothing, or collinear — one shared end (a coordinate) or a piece
    u, v = (qx * sy - qy * sx) / den, (qx * ry - qy * rx) / den
    if 0 <= u <= 1 and 0 <= v <= 1:
        return (a[0] + u * rx, a[1] + u * ry)
    return None


def _arrangement_bits(A: _Row, B: _Row) -> int:
    nodes = A.pts | B.pts
    for s in A.segs:
        for t in B.segs:
            x = _meet_point(s, t)
            if x is not None:
                nodes.add(x)
    m = 0
    for x in nodes:
        on_a, on_b = A.has(x), B.has(x)
        if on_a and on_b:
            ba, bb = x in A.bnd, x in B.bnd
            m |= (BND_BND if bb else BND_INT) if ba else (INT_BND if bb else INTERIORS)
        elif on_a:
            m |= A_OUTSIDE
        else:
            m |= B_OUTSIDE
    for own, other, outside in ((A, B, A_OUTSIDE), (B, A, B_OUTSIDE)):
        for s in own.segs:
            on = sorted(x for x in nodes if _in_box(x, s) and _orient(s[0], s[1], x) == 0)
            for p, q in zip(on[:-1], on[1:]):
                mid = ((p[0] + q[0]) / 2, (p[1] + q[1]) / 2)  # no node: no coordinate, an interior point of its row
                m |= (INTERIORS | SHARED_PIECE) if other.has(mid) else outside
    return m


def mask(ka, row_a, kb, row_b, a_valid=True, b_valid=True) -> int:
    ma, mb = usable(ka, row_a, a_valid), usable(kb, row_b, b_valid)
    if ma is None or mb is None:
        return 0
    return _arrangement_bits(_Row(ma), _Row(mb))


def masks(ka, rows_a, kb, rows_b, rows=None, av=None, bv=None):
    out = np.zeros(len(rows_a), dtype=np.uint8)
    for i, ra in enumerate(rows_a):
        j = i if rows is None else int(rows[i])
        if j >= len(rows_b):
            continue
        out[i] = mask(ka, ra, kb, rows_b[j], av is None or av[i], bv is None or bv[j])
    return out


# ---- the kernel's formulation ------------------------------------------------------------------------------------------------------


def _shared_bit(ba, bb):
    return (BND_BND if bb else BND_INT) if ba else (INT_BND if bb else INTERIORS)


def _covered(s, other: _Row) -> bool:
    """the frontier walk: do the collinear pieces `other` shares with the segment cover it"""
    a, b = s[0], s[1]
    ax = 0 if a[0] != b[0] else 1
    f, hi = min(a[ax], b[ax]), max(a[ax], b[ax])
    while f < hi:
        nf = f
        for t in other.segs:
            if _orient(a, b, t[0]) != 0 or _orient(a, b, t[1]) != 0:
                continue
            lo, up = min(t[0][ax], t[1][ax]), max(t[0][ax], t[1][ax])
            if lo <= f and up > nf:
                nf = up
        if nf == f:
            return False
        f = nf
    return True


def mask_by_rules(ka, row_a, kb, row_b) -> int:
    ma, mb = usable(ka, row_a), usable(kb, row_b)
    if ma is None or mb is None:
        return 0
    A, B = _Row(ma), _Row(mb)
    m = 0
    for own, other, first, outside in ((A, B, True, A_OUTSIDE), (B, A, False, B_OUTSIDE)):
        for c in own.pts:
            if other.has(c):
                bo, bt = sum(e == c for e in own.ends) % 2 == 1, sum(e == c for e in other.ends) % 2 == 1
                m |= _shared_bit(bo, bt) if first else _shared_bit(bt, bo)
            else:
                m |= outside
    for s in A.segs:
        for t in B.segs:
            a, b, c, d = s[0], s[1], t[0], t[1]
            o1, o2 = _orient(a, b, c), _orient(a, b, d)
            if o1 == 0 and o2 == 0:
                ax = 0 if a[0] != b[0] else 1
                if max(min(a[ax], b[ax]), min(c[ax], d[ax])) < min(max(a[ax], b[ax]), max(c[ax], d[ax])):
                    m |= INTERIORS | SHARED_PIECE
            elif o1 * o2 < 0 and _orient(c, d, a) * _orient(c, d, b) < 0:
                at = lambda v: _in_box(v, s) and _in_box(v, t) and _orient(a, b, v) == 0 and _orient(c, d, v) == 0  # noqa: E731
                m |= _shared_bit(sum(at(v) for v in A.ends) % 2 == 1, sum(at(v) for v in B.ends) % 2 == 1)
    if not m & A_OUTSIDE and not all(_covered(s, B) for s in A.segs):
        m |= A_OUTSIDE
    if not m & B_OUTSIDE and not all(_covered(s, A) for s in B.segs):
        m |= B_OUTSIDE
    return m


# ---- hand-derived cases: (name, members of A, members of B, mask) ----------------------------------------------------------------------

RING = [(0, 0), (4, 0), (4, 4), (0, 4), (0, 0)]
BOW = [(0, 0), (4, 4), (4, 0), (0, 4)]  # crosses itself at (2, 2); ends (0, 0) and (0, 4)

KNOWN = [
    # II = {(2, 2)}, nothing else shared; both have points off the other: 1FF0FF... -> crosses
    ("an X", [[(0, 0), (4, 4)]], [[(0, 4), (4, 0)]], 1 | 96),
    ("apart", [[(0, 0), (1, 1)]], [[(5, 5), (6, 7)]], 96),
    # the only shared point is an end of both: BB -> touches
    ("end on end", [[(0, 0), (2, 2)]], [[(2, 2), (4, 0)]], 16 | 96),
    # an end of A inside B's segment: BI -> touches
    ("T-junction", [[(2, 0), (2, 2)]], [[(0, 2), (4, 2)]], 8 | 96),
    # the same point set: II has dimension 1, the ends coincide (BB), nothing outside -> equals
    ("the same line", [[(0, 0), (2, 2), (4, 0)]], [[(0, 0), (2, 2), (4, 0)]], 1 | 2 | 16),
    # A inside B's segment: II dimension 1, A's ends are interior points of B (BI), B sticks out -> within
    ("a stretch of B", [[(1, 0), (2, 0)]], [[(0, 0), (4, 0)]], 1 | 2 | 8 | 64),
    # [2, 3] shared; A's end (3, 0) inside B (BI), B's end (2, 0) inside A (IB), both stick out -> overlaps
    ("partial overlap", [[(0, 0), (3, 0)]], [[(2, 0), (5, 0)]], 1 | 2 | 4 | 8 | 96),
]

TIES = [
    ("crossing between lattice points", [[(0, 0), (3, 1)]], [[(0, 1), (3, 0)]], 1 | 96),
    # the crossing point (1, 1/3) is no double
    ("crossing at a point that is no double", [[(0, 0), (3, 1)]], [[(1, -1), (1, 2)]], 1 | 96),
    # a second member of A ends at (1, 1), on B's segment next to the crossing: a boundary point of A inside B (BI) besides II
    ("an end of another member near the crossing", [[(0, 0), (3, 1)], [(5, 5), (1, 1)]], [[(1, -1), (1, 2)]], 1 | 8 | 96),
    # a second member of A ends AT the crossing (2, 1): the one shared point is a boundary point of A -> BI only, touches
    ("an end of another member at the crossing", [[(0, 0), (4, 2)], [(5, 5), (2, 1)]], [[(2, -1), (2, 3)]], 8 | 96),
    # ... and a member of B ends there too: BB only
    ("ends of both at the crossing", [[(0, 0), (4, 2)], [(5, 5), (2, 1)]], [[(2, -1), (2, 3)], [(2, 1), (-3, 4)]], 16 | 96),
    ("T-junction, A's end", [[(2, 0), (2, 2)]], [[(0, 2), (4, 2)]], 8 | 96),
    ("T-junction, B's end", [[(0, 2), (4, 2)]], [[(2, 0), (2, 2)]], 4 | 96),
    ("end on end", [[(0, 0), (2, 2)]], [[(2, 2), (4, 0)]], 16 | 96),
    # three members of A end at (0, 0): counted 3 times, a boundary point; B runs through it -> BI
    ("three members meet (odd)", [[(-2, 0), (0, 0)], [(0, 0), (2, 1)], [(0, 0), (1, -2)]], [[(-1, -3), (1, 3)]], 8 | 96),
    # two members: counted twice, an interior point -> II
    ("two members meet (even)", [[(-2, 0), (0, 0)], [(0, 0), (2, 1)]], [[(-1, -3), (1, 3)]], 1 | 96),
    # a closed member has no boundary: its start is an interior point
    ("ring, a line through its start", [RING], [[(-2, -2), (2, 2)]], 1 | 96),
    ("ring, a line that ends at its start", [RING], [[(-2, -2), (0, 0)]], 4 | 96),
    ("reversed, with extra collinear vertices", [[(0, 0), (4, 0), (4, 4)]], [[(4, 4), (4, 2), (4, 0), (2, 0), (0, 0)]], 1 | 2 | 16),
    # B's members abut at (3, 0), counted twice: interior.  A's ends are interior points of B, B sticks out -> within
    ("covered by two members that abut", [[(1, 0), (5, 0)]], [[(0, 0), (3, 0)], [(3, 0), (6, 0)]], 1 | 2 | 8 | 64),
    # the gap (3, 4) is off B; its ends are boundary points of B inside A (IB)
    ("covered except for a gap", [[(1, 0), (5, 0)]], [[(0, 0), (3, 0)], [(4, 0), (6, 0)]], 1 | 2 | 4 | 8 | 96),
    ("partial overlap", [[(0, 0), (3, 0)]], [[(2, 0), (5, 0)]], 1 | 2 | 4 | 8 | 96),
    # a point member has no boundary: it is an interior point of A
    ("point member inside B", [[(2, 0)]], [[(0, 0), (4, 0)]], 1 | 64),  # within
    ("point member (equal coordinates) on B's end", [[(0, 0), (0, 0)]], [[(0, 0), (4, 0)]], 4 | 64),  # covered_by, not within
    ("point member off B", [[(1, 1)]], [[(0, 0), (4, 0)]], 96),
    ("self-crossing A, B through the crossing", [BOW], [[(2, -1), (2, 5)]], 1 | 96),
    # B is A's first segment: shared piece; (0, 0) ends both (BB), (4, 4) ends B inside A (IB); A's third segment crosses B (II)
    ("self-crossing A, B along its first segment", [BOW], [[(0, 0), (4, 4)]], 1 | 2 | 4 | 16 | 32),
    ("zero-length segments", [[(0, 0), (2, 2), (2, 2), (4, 4)]], [[(0, 4), (2, 2), (2, 2), (2, 2), (4, 0)]], 1 | 96),
]


def as_row(kind, ms):
    """members as a row of `kind`; a MULTILINESTRING row gets an empty member in front"""
    if kind == LS:
        assert len(ms) == 1
        return list(ms[0])
    return [[]] + [list(m) for m in ms]


def pad_member(m, k):
    """k more vertices inside every segment, collinear and on the lattice (the coordinates are scaled by k + 1 first)"""
    return R.pad_ring(m, k) if len(m) else m


def padded(kind, row, k):
    if k == 0:
        return row
    return pad_member(row, k) if kind == LS else [pad_member(m, k) for m in row]


def case_columns(cases, ka, kb, pad=0):
    """(rows of A, rows of B, masks, names) of the cases that the two kinds can hold, every segment padded with `pad` collinear
    vertices (both sides scale alike: the answers stay)"""
    sel = [c for c in cases if (ka == MLS or len(c[1]) == 1) and (kb == MLS or len(c[2]) == 1)]
    a = [padded(ka, as_row(ka, c[1]), pad) for c in sel]
    b = [padded(kb, as_row(kb, c[2]), pad) for c in sel]
    return a, b, np.array([c[3] for c in sel], dtype=np.uint8), [c[0] for c in sel]


# ---- random lattice columns ----------------------------------------------------------------------------------------------------------

STEPS = [(dx, dy) for dx in range(-2, 3) for dy in range(-2, 3) if (dx, dy) != (0, 0)]


def _walk(rng, n, lo=0, hi=9, start=None):
    """n lattice coordinates, steps of at most 2 a direction, inside [lo, hi]^2"""
    p = start if start is not None else (int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1)))
    lo, hi = min(lo, p[0], p[1]), max(hi, p[0], p[1])  # (a start outside the square widens it)
    out = [p]
    while len(out) < n:
        dx, dy = STEPS[int(rng.integers(0, len(STEPS)))]
        q = (out[-1][0] + dx, out[-1][1] + dy)
        if lo <= q[0] <= hi and lo <= q[1] <= hi:
            out.append(q)
    return out


def _rewritten(m, rng):
    """the same point set written differently: reversed now and then, lattice midpoints put in"""
    out = []
    for p, q in zip(m[:-1], m[1:]):
        out.append(p)
        if (p[0] + q[0]) % 2 == 0 and (p[1] + q[1]) % 2 == 0 and rng.random() < 0.7:
            out.append(((p[0] + q[0]) // 2, (p[1] + q[1]) // 2))
    out.append(m[-1])
    return out[::-1] if rng.random() < 0.5 else out


def _partner(a, style, rng):
    """a member B for the member A: 0 — another walk, 1 — A rewritten, 2 — a stretch of A, 3 — A's tail and more, 4 — from A's end
    onwards, 5 — a walk that ends on a vertex of A, 6 — far away, 7 — a walk through a vertex of A"""
    if style == 1:
        return _rewritten(a, rng)
    if style == 2:
        i = int(rng.integers(0, len(a) - 2))
        return _rewritten(a[i : i + int(rng.integers(2, len(a) - i + 1))], rng)
    if style == 3:
        k = int(rng.integers(1, len(a) - 1))
        return a[k:] + _walk(rng, 3, start=a[-1])[1:]
    if style == 4:
        return _walk(rng, int(rng.integers(2, 5)), start=a[-1] if rng.random() < 0.7 else a[0])
    if style == 5:
        return _walk(rng, int(rng.integers(2, 4)), start=a[int(rng.integers(1, len(a) - 1))])[::-1]
    if style == 6:
        return [(x + 40, y + 3) for x, y in _walk(rng, 3)]
    if style == 7:
        v = a[int(rng.integers(1, len(a) - 1))]
        dx, dy = STEPS[int(rng.integers(0, len(STEPS)))]
        return [(v[0] - dx, v[1] - dy), v, (v[0] + dx, v[1] + dy)]
    return _walk(rng, int(rng.integers(2, 6)))


@lru_cache(maxsize=None)
def random_columns(ka, kb, n_rows=96):
    """(rows of A, rows of B, masks): walks on a 10 x 10 lattice against partners built to coincide with them in many ways;
    MULTILINESTRING rows carry a second member now and then (a stretch that abuts, a point, a walk) and empty members"""
    rng = np.random.default_rng(3000 + 10 * ka + kb)
    A, B = [], []
    for i in range(n_rows):
        a = _walk(rng, int(rng.integers(4, 7)))
        b = _partner(a, i % 8, rng)
        ra, rb = [a], [b]
        if ka == MLS and i % 16 >= 8:
            ra.append(_walk(rng, 3, start=a[-1]) if i % 3 else [a[0]])
        if ka == MLS and kb == MLS and i % 8 == 1:
            rb += [_rewritten(m, rng) for m in ra[1:]]  # (the same members on both sides: equals)
        elif kb == MLS and i % 32 >= 16:
            rb.append(_walk(rng, 2, start=b[0]) if i % 3 else _walk(rng, 3))
        for kind, row in ((ka, ra), (kb, rb)):
            if kind == MLS and i % 3 == 1:
                row.insert(int(rng.integers(0, len(row) + 1)), [])
        A.append(a if ka == LS else ra)
        B.append(b if kb == LS else rb)
    return A, B, masks(ka, A, kb, B)


# ---- the join fixture ------------------------------------------------------------------------------------------------------------------


def _boxes(kind, rows, ok):
    inf = 10**9
    out = []
    for i, r in enumerate(rows):
        pts = [p for m in members(kind, r) for p in m]
        out.append((min(x for x, _ in pts), min(y for _, y in pts), max(x for x, _ in pts), max(y for _, y in pts)) if ok[i] else (inf, inf, -inf, -inf))
    return np.array(out)


def mask_table(ka, rows_a, av, kb, rows_b, bv):
    """the exact masks of every row of A against every row of B (pairs of usable rows whose boxes are apart: 96)"""
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
def join_fixture(ka=LS, kb=LS, n=300):
    """two columns of about n short lines over a 120 x 120 lattice.  Both hold the same block of street segments of a 5 x 5 grid
    (junctions: shared ends; equal rows across the columns) and a long line across the whole domain (a row with many candidates on
    either side); the right column repeats some left rows rewritten, cut short or run on; a null row and an empty row on either
    side.  Returns (left, left validity, right, right validity, table[n, n] of exact masks, table of left against left)."""
    rng = np.random.default_rng(77 + ka + kb)
    streets = [[(130 + 4 * i, 4 * j), (134 + 4 * i, 4 * j)] for i in range(5) for j in range(4)] + [[(130 + 4 * i, 4 * j), (130 + 4 * i, 4 * j + 4)] for i in range(4) for j in range(4)]
    long_line = [(-3, -2), (60, 61), (125, 124)]

    def column(kind, seed_rows):
        rows = []
        for j in range(n - len(streets) - len(seed_rows)):
            o = (int(rng.integers(0, 110)), int(rng.integers(0, 110)))
            m = [(x + o[0], y + o[1]) for x, y in _walk(rng, int(rng.integers(2, 6)), hi=12)]
            if kind == MLS and j % 3 == 0:
                rows.append([[], m] if j % 2 else [m, _walk(rng, 3, lo=0, hi=119, start=m[-1])])
            else:
                rows.append(m if kind == LS else [m])
        rows += [s if kind == LS else [s] for s in streets]
        rows += [r if kind == LS else [r] for r in seed_rows]
        return rows

    left = column(ka, [])
    left[5] = long_line if ka == LS else [long_line]
    first = lambda i: members(ka, left[i])[-1]  # noqa: E731
    seeds = [_rewritten(first(i), rng) for i in range(60, 68)]
    seeds += [first(i)[:-1] if len(first(i)) > 2 else first(i) for i in range(68, 74)]
    seeds += [first(i) + _walk(rng, 2, lo=-5, hi=125, start=first(i)[-1])[1:] for i in range(74, 80)]
    right = column(kb, seeds)
    right[17] = long_line[::-1] if kb == LS else [long_line[:2], long_line[1:]]
    left[23], right[40] = [], []
    lv, rv = np.ones(n, dtype=bool), np.ones(n, dtype=bool)
    lv[31] = rv[52] = False
    return left, lv, right, rv, mask_table(ka, left, lv, kb, right, rv), mask_table(ka, left, lv, ka, left, lv)


def expected_pairs(table, pred: str):
    """(pairs sorted by (l, r), counts per left row, masks per pair) of a predicate over a mask table [left, right]"""
    hit = np.vectorize(PREDICATES[pred], otypes=[bool])(table)
    ll, rr = np.nonzero(hit)
    return np.stack([ll, rr], axis=1).astype(np.uint32), np.bincount(ll, minlength=table.shape[0]).astype(np.uint32), table[ll, rr]


def zigzag_pair(n=600):
    """a zigzag of n coordinates and the same with every second vertex dropped (the rows of the slow path)"""
    a = [(2 * i, (i % 2) * 3 + (i % 4 == 3)) for i in range(n)]
    return a, a[::2]
