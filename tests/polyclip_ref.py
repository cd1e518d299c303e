"""Exact reference of the polygon clip (gpk_polygon_clip, csrc/gpk_polyclip.h) and its fixture.

Rules 1 - 5 of the header on Fractions, not computed the way the kernel computes them: no depth walk, no identities, no orientation
flags.  Every segment of every ring walk is cut at ALL its exact meets with the other row's edges, the rational midpoint of every piece
is classified against the other row by crossing numbers, a piece along an edge gets its side from the signed area of the carrying ring,
arcs are linked by EXACT POINT EQUALITY, the junction order comes from exact cross and dot products of the true neighbours, ring signs
from exact shoelace areas and nesting from exact crossing numbers.  All fixtures live on small integer lattices; rows are what
tests/exact_ref.column takes.  tests/test_polyclip_ref.py pins this file by identities it shares no code with."""
from __future__ import annotations

import io
import os
from fractions import Fraction
from functools import cmp_to_key, lru_cache

import numpy as np

from tests import exact_ref as X
from tests import overlay_ref as O
from tests import polyrel_ref as P
from tests import relation_ref as R

PG, MPG = R.PG, R.MPG
NAMES = R.NAMES
FAMILIES = O.AREA_FAMILIES
INTERSECTION, DIFFERENCE = 0, 1
MODES = {INTERSECTION: "intersection", DIFFERENCE: "difference"}
WALK_A, WALK_B = 0, 1
INT, SAME, EXT, OPP = 1, 2, 4, 8  # the classes of a piece
ST_OK, ST_TOUCH, ST_EMPTY, ST_NULL, ST_UNRESOLVED = 0, 1, 2, 3, 4
TAG_IN, TAG_X = 0, 1  # an output coordinate: an input coordinate (bit for bit) or a computed crossing
MIN_GAP = Fraction(1, 10**6)
REL_TOL = 1e-9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polyclip_lattice.npz")
TRANSLATION = O.TRANSLATION
sq = R.sq


def kept(cls: int, walk: int, mode: int) -> bool:
    if walk == WALK_B:
        return cls == INT
    return cls in (INT, SAME) if mode == INTERSECTION else cls in (EXT, OPP)


# ---- exact helpers -------------------------------------------------------------------------------------------------------------------


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _shoelace2(ring):
    """twice the signed area of a closed ring of exact points"""
    return sum(ring[i][0] * ring[i + 1][1] - ring[i + 1][0] * ring[i][1] for i in range(len(ring) - 1))


def _on_segment(t, a, b):
    return min(a[0], b[0]) <= t[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= t[1] <= max(a[1], b[1]) and _cross(a, b, t) == 0  # (the cheap test first)


def ring_position(t, ring):
    """+1 inside, 0 on, -1 outside a closed ring (exact points), by the crossing number"""
    inside = False
    for a, b in zip(ring, ring[1:]):
        if a == b:
            continue
        if _on_segment(t, a, b):
            return 0
        if (a[1] > t[1]) != (b[1] > t[1]):
            s = _cross(a, b, t)
            if (b[1] > a[1]) == (s > 0):
                inside = not inside
    return 1 if inside else -1


def row_rings(kind, row):
    """(member, is_hole, first coordinate number in the row, [(x, y) ints]) of every non-empty ring of every non-empty member"""
    members = [row] if kind == PG else list(row)
    out, at = [], 0
    for m, poly in enumerate(members):
        live = len(poly) > 0 and len(poly[0]) > 0
        for k, r in enumerate(poly):
            if live and len(r):
                out.append((m, k > 0, at, [(int(x), int(y)) for x, y in r]))
            at += len(r)
    return out


def row_position(t, rings):
    """INT / EXT, or 0 on a ring, of an exact point against the rings of row_rings"""
    pos = [(m, hole, ring_position(t, c)) for m, hole, _c0, c in rings]
    if any(p == 0 for _m, _h, p in pos):
        return 0
    for m in {m for m, _h, _p in pos}:
        if all((p < 0) if hole else (p > 0) for mm, hole, p in pos if mm == m):
            return INT
    return EXT


def _edges(rings):
    """(first coordinate number, a, b, interior on the left of a -> b) of every non-degenerate edge"""
    out = []
    for _m, hole, c0, c in rings:
        left = (_shoelace2(c) > 0) != hole
        for k in range(len(c) - 1):
            if c[k] != c[k + 1]:
                out.append((c0 + k, c[k], c[k + 1], left))
    return out


def _cuts(p, q, edges):
    """the sorted cut parameters of segment pq with the edges, 0 and 1 included"""
    d = (q[0] - p[0], q[1] - p[1])
    lo, hi = (min(p[0], q[0]), min(p[1], q[1])), (max(p[0], q[0]), max(p[1], q[1]))
    ts = {Fraction(0), Fraction(1)}
    for _k, a, b, _l in edges:
        if max(a[0], b[0]) < lo[0] or min(a[0], b[0]) > hi[0] or max(a[1], b[1]) < lo[1] or min(a[1], b[1]) > hi[1]:
            continue
        e, ap = (b[0] - a[0], b[1] - a[1]), (a[0] - p[0], a[1] - p[1])
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
    return sorted(ts)


def _piece_class(mid, p, q, rings, edges):
    pos = row_position(mid, rings)
    if pos:
        return pos
    for _k, a, b, left in edges:  # the carrying edge: the other row's interior is on our left iff it is on its left and it runs our way
        if _cross(a, b, p) == 0 and _cross(a, b, q) == 0 and _on_segment(mid, a, b):
            same_dir = (b[0] - a[0]) * (q[0] - p[0]) + (b[1] - a[1]) * (q[1] - p[1]) > 0
            return SAME if left == same_dir else OPP
    raise AssertionError("a piece on the boundary that no edge carries")


def _walk_arcs(rings_w, rings_o, walk, mode, gaps):
    """the arcs of one walk: dicts with pts (exact points, both ends included), key, whole"""
    edges_o = _edges(rings_o)
    arcs = []
    for _m, hole, c0, c in rings_w:
        w = c if (_shoelace2(c) > 0) != hole else c[::-1]  # interior on the left
        pieces, ip = [], 0
        for iq in range(1, len(w)):
            p, q = w[ip], w[iq]
            if p == q:
                continue
            ts = _cuts(p, q, edges_o)
            gaps.extend(t1 - t0 for t0, t1 in zip(ts, ts[1:]))
            for t0, t1 in zip(ts, ts[1:]):
                tm = (t0 + t1) / 2
                mid = (p[0] + tm * (q[0] - p[0]), p[1] + tm * (q[1] - p[1]))
                cls = _piece_class(mid, p, q, rings_o, edges_o)
                start = (p[0] + t0 * (q[0] - p[0]), p[1] + t0 * (q[1] - p[1]))
                pieces.append((c0 + iq - 1, t0, start, cls, kept(cls, walk, mode)))
            ip = iq
        n = len(pieces)
        if not any(pc[4] for pc in pieces):
            continue

        def is_break(i):
            prev, cur = pieces[i - 1], pieces[i]
            if prev[4] != cur[4]:
                return True
            return cur[4] and prev[3] in (INT, EXT) and cur[3] in (INT, EXT) and row_position(cur[2], rings_o) == 0

        brk = [is_break(i) for i in range(n)]
        breaks = [i for i in range(n) if brk[i]]
        if not breaks:
            pts = [pc[2] for pc in pieces if pc[1] == 0]
            arcs.append({"pts": pts + [pts[0]], "key": (walk, c0, 0, Fraction(0)), "whole": True})
            continue
        for i in breaks:
            if not pieces[i][4]:
                continue
            pts, j = [pieces[i][2]], (i + 1) % n
            while not brk[j]:
                if pieces[j][1] == 0:
                    pts.append(pieces[j][2])
                j = (j + 1) % n
            pts.append(pieces[j][2])
            seg, t0 = pieces[i][0], pieces[i][1]
            arcs.append({"pts": pts, "key": (walk, seg, 0 if t0 == 0 else 1, t0), "whole": False})
    if walk == WALK_B and mode == DIFFERENCE:
        for a in arcs:
            a["pts"] = a["pts"][::-1]
    return arcs


def _cw_order(E, back):
    """compare two directions from E by the clockwise angle from E -> back, in (0, a full turn]"""

    def rank(d):
        c = _cross(E, back, d)
        if c < 0:
            return 0
        if c > 0:
            return 2
        dot = (back[0] - E[0]) * (d[0] - E[0]) + (back[1] - E[1]) * (d[1] - E[1])
        return 3 if dot > 0 else 1

    def cmp(d1, d2):
        r1, r2 = rank(d1), rank(d2)
        if r1 != r2:
            return r1 - r2
        c = _cross(E, d1, d2)
        return -1 if c < 0 else (1 if c > 0 else 0)

    return cmp


def stitch(arcs):
    """(parts, status): parts = a list of lists of closed rings of exact points, shell first; None when the arcs do not close"""
    arcs = sorted(arcs, key=lambda a: a["key"])
    starts = {}
    for k, a in enumerate(arcs):
        if not a["whole"]:
            starts.setdefault(a["pts"][0], []).append(k)
    used, rings = [False] * len(arcs), []
    for k0 in range(len(arcs)):
        if used[k0]:
            continue
        ring, k = [], k0
        while True:
            if used[k]:
                return None, ST_UNRESOLVED
            used[k] = True
            a = arcs[k]
            ring.extend(a["pts"][:-1])
            if a["whole"]:
                break
            E, back = a["pts"][-1], a["pts"][-2]
            cand = starts.get(E, [])
            if not cand:
                return None, ST_UNRESOLVED
            cmp = _cw_order(E, back)
            k = sorted(cand, key=cmp_to_key(lambda i, j: cmp(arcs[i]["pts"][1], arcs[j]["pts"][1])))[0]
            if k == k0:
                break
        ring.append(ring[0])
        rings.append(ring)
    status = ST_TOUCH if any(len(set(r[:-1])) != len(r) - 1 for r in rings) else ST_OK
    signs = [_shoelace2(r) for r in rings]
    if any(s == 0 for s in signs):
        return None, ST_UNRESOLVED
    shells = [k for k, s in enumerate(signs) if s > 0]
    holes_of = {k: [] for k in shells}
    for k, s in enumerate(signs):
        if s > 0:
            continue
        home = None
        for sh in shells:
            verdict = next((v for v in (ring_position(t, rings[sh]) for t in rings[k][:-1]) if v != 0), 0)
            if verdict > 0:
                home = sh
                break
        if home is None:
            return None, ST_UNRESOLVED
        holes_of[home].append(k)
    parts = [[rings[sh]] + [rings[h] for h in holes_of[sh]] for sh in shells]
    return parts, (ST_EMPTY if not parts else status)


def clip(ka, row_a, kb, row_b, mode, a_valid=True, b_valid=True):
    """(parts, status, min gap) of one pair; parts None for a null result row"""
    if P.usable(ka, row_a, a_valid) is None or P.usable(kb, row_b, b_valid) is None:
        return None, ST_NULL, None
    ra, rb = row_rings(ka, row_a), row_rings(kb, row_b)
    gaps = []
    arcs = _walk_arcs(ra, rb, WALK_A, mode, gaps) + _walk_arcs(rb, ra, WALK_B, mode, gaps)
    parts, status = stitch(arcs)
    return parts, status, (min(gaps) if gaps else None)


def transition_gap(ka, row_a, kb, row_b, mode, kept_fn=None):
    """What Rule 6 of gpk_polyclip.h conditions on, by the headers' own definition: a transition is a touch point, or a vertex of the
    walked ring, where the kept-ness of the piece before differs from that of the piece after (a cut of rule 4, kept on both hands, is
    none).  Returns the least distance between two distinct transition points of one segment of either walk, as a share of the segment
    (a Fraction), None when no segment carries two.  `clip`'s third value is another thing: the least distance between ANY two cuts of a
    segment, its own ends included.  kept_fn: the kept table (default: this module's)."""
    kept_fn = kept if kept_fn is None else kept_fn
    ra, rb = row_rings(ka, row_a), row_rings(kb, row_b)
    best = None
    for rings_w, rings_o, walk in ((ra, rb, WALK_A), (rb, ra, WALK_B)):
        edges_o = _edges(rings_o)
        for _m, hole, _c0, c in rings_w:
            w = c if (_shoelace2(c) > 0) != hole else c[::-1]
            segs, ip = [], 0  # per non-degenerate segment: [(t0, kept)] of its pieces
            for iq in range(1, len(w)):
                p, q = w[ip], w[iq]
                if p == q:
                    continue
                ts = _cuts(p, q, edges_o)
                pcs = []
                for t0, t1 in zip(ts, ts[1:]):
                    tm = (t0 + t1) / 2
                    mid = (p[0] + tm * (q[0] - p[0]), p[1] + tm * (q[1] - p[1]))
                    pcs.append((t0, kept_fn(_piece_class(mid, p, q, rings_o, edges_o), walk, mode)))
                segs.append(pcs)
                ip = iq
            trans = [{pcs[k][0] for k in range(1, len(pcs)) if pcs[k][1] != pcs[k - 1][1]} for pcs in segs]
            for s, pcs in enumerate(segs):  # the ring is closed: segment s - 1 ends where segment s begins
                if segs[s - 1][-1][1] != pcs[0][1]:
                    trans[s].add(Fraction(0))
                    trans[s - 1].add(Fraction(1))
            for here in trans:
                ts = sorted(here)
                for t0, t1 in zip(ts, ts[1:]):
                    best = t1 - t0 if best is None else min(best, t1 - t0)
    return best


def scaled_back(parts, ka, row_a, kb, row_b, scale):
    """A result of `clip` (or polyunion_ref.union) on rows that tests/hard_orient.on_integer_grid brought to an integer grid, in the
    units of the doubles (scale = hard_orient.integer_grid_scale of the same rows, a power of two): parts -> rings -> coordinates
    (TAG_IN, x, y, -1, -1) with x, y the doubles of the input coordinate, exactly — to be compared bit for bit — or
    (TAG_X, x, y, edge of a, edge of b) with Fractions x, y and the two carrying edges as tag_point names them."""
    if parts is None:
        return None
    ra, rb = row_rings(ka, row_a), row_rings(kb, row_b)
    out = []
    for p in parts:
        rings = []
        for r in p:
            pts = []
            for pt in r:
                t, e0, e1 = tag_point((Fraction(pt[0]), Fraction(pt[1])), ra, rb)
                x, y = Fraction(pt[0]) / scale, Fraction(pt[1]) / scale
                if t == TAG_IN:
                    assert Fraction(float(x)) == x and Fraction(float(y)) == y
                    x, y = float(x), float(y)
                pts.append((t, x, y, e0, e1))
            rings.append(pts)
        out.append(rings)
    return out


def shape_of(parts, ka, row_a, kb, row_b):
    """what a wrong orientation sign changes in a result, as a hashable value: per part, per ring, per coordinate the number of the
    input coordinate that stands there ("a" or "b" and its row-relative number), or "x" for a computed crossing"""
    if parts is None:
        return None
    ra, rb = row_rings(ka, row_a), row_rings(kb, row_b)
    where = {}
    for name, rings in (("a", ra), ("b", rb)):
        for _m, _h, c0, c in rings:
            for k, v in enumerate(c[:-1]):
                where.setdefault(v, (name, c0 + k))

    def label(pt):
        if pt[0].denominator == 1 and pt[1].denominator == 1 and (int(pt[0]), int(pt[1])) in where:
            return where[(int(pt[0]), int(pt[1]))]
        return "x"

    return tuple(tuple(tuple(label(pt) for pt in r) for r in p) for p in parts)


def counts_of(parts):
    """(parts, rings, coordinates per ring with the closing one) of a result"""
    return None if parts is None else (len(parts), sum(len(p) for p in parts), tuple(len(r) for p in parts for r in p))


def check_rows(want, status_want, ca, cb, got, status=None):
    """check_result for rows that are in no fixture file: `want[i]` is None (a null row) or the rings of scaled_back for row i of the
    columns ca, cb, `got` the downloaded MULTIPOLYGON column.  Offsets, validity, status and ring starts exactly, input coordinates bit
    for bit, crossings within REL_TOL * d of both carrying edges.  Returns (the worst ratio of a crossing's distance to its bound, the
    number of crossings)."""
    n = len(want)
    assert got.n_geoms == n
    gv = np.ones(n, dtype=bool) if got.validity is None else np.unpackbits(got.validity, bitorder="little")[:n].astype(bool)
    wv = np.array([w is not None for w in want])
    assert (gv == wv).all(), np.nonzero(gv != wv)[0][:10]
    if status is not None:
        assert (np.asarray(status) == np.asarray(status_want)).all(), np.nonzero(np.asarray(status) != np.asarray(status_want))[0][:10]
    live = [w for w in want if w is not None]
    n_parts = np.array([0 if w is None else len(w) for w in want])
    assert (np.diff(got.geom_offsets) == n_parts).all(), np.nonzero(np.diff(got.geom_offsets) != n_parts)[0][:10]
    n_rings = np.array([len(p) for w in live for p in w], dtype=np.int64)
    assert (np.diff(got.part_offsets) == n_rings).all(), np.nonzero(np.diff(got.part_offsets) != n_rings)[0][:10]
    sizes = np.array([len(r) for w in live for p in w for r in p], dtype=np.int64)
    assert (np.diff(got.ring_offsets) == sizes).all(), np.nonzero(np.diff(got.ring_offsets) != sizes)[0][:10]
    sa, sb, diag = _row_starts(ca), _row_starts(cb), pair_diagonals(ca, cb)
    at, worst, n_x = 0, 0.0, 0
    for i, w in enumerate(want):
        for p in w or []:
            for r in p:
                for t, x, y, e0, e1 in r:
                    g = got.xy[at]
                    if t == TAG_IN:
                        assert g.tobytes() == np.array([x, y], dtype=np.float64).tobytes(), (i, "an input coordinate is not returned bit for bit", g, (x, y))
                    else:
                        ia, ib = int(sa[i]) + e0, int(sb[i]) + e1
                        far = max(float(_off_segment(g[None], ca.xy[ia][None], ca.xy[ia + 1][None])[0]), float(_off_segment(g[None], cb.xy[ib][None], cb.xy[ib + 1][None])[0]))
                        worst, n_x = max(worst, far / (REL_TOL * diag[i])), n_x + 1
                        assert far <= REL_TOL * diag[i], (i, far, diag[i])
                    at += 1
    assert at == len(got.xy)
    return worst, n_x


def area_of(parts) -> Fraction:
    return sum((Fraction(_shoelace2(r), 2) for p in parts for r in p), Fraction(0))


def row_area(kind, row) -> Fraction:
    return sum((abs(Fraction(_shoelace2(c), 2)) * (-1 if hole else 1) for _m, hole, _c0, c in row_rings(kind, row)), Fraction(0))


def tag_point(pt, ra, rb):
    """(TAG_IN, -1, -1) for a coordinate of either row, else (TAG_X, edge of a, edge of b) of the two edges that cross at pt properly —
    edges as row-relative numbers of their first coordinate"""
    if pt[0].denominator == 1 and pt[1].denominator == 1:
        ipt = (int(pt[0]), int(pt[1]))
        if any(ipt in c for _m, _h, _c0, c in ra + rb):
            return TAG_IN, -1, -1
    found = []
    for rings in (ra, rb):
        hit = [k for k, a, b, _l in _edges(rings) if _on_segment(pt, a, b) and pt != a and pt != b]
        assert len(hit) == 1, (pt, hit)
        found.append(hit[0])
    return TAG_X, found[0], found[1]


# ---- hand cases: the smallest shapes that can go wrong, (parts, rings) of the intersection and of the difference by hand -------------

S10, DONUT = P.S10, P.DONUT
COMB = [(0, 0), (14, 0), (14, 10), (12, 10), (12, 4), (10, 4), (10, 10), (8, 10), (8, 4), (6, 4), (6, 10), (4, 10), (4, 4), (2, 4), (2, 10), (0, 10), (0, 0)]
THIN_A = [(0, 0), (30, 10), (29, 13), (-1, 3), (0, 0)]
THIN_B = [(10, -5), (13, -6), (23, 24), (20, 25), (10, -5)]
APEX = [(2, -2), (8, -2), (5, 10), (2, -2)]  # its apex on the top edge of S10
HAND_CASES = [
    ("two crossing squares", [[S10]], [[sq(5, 5, 15, 15)]], (1, 1), (1, 1)),
    ("two thin rectangles crossing: all four result vertices computed", [[THIN_A]], [[THIN_B]], (1, 1), (2, 2)),
    ("b inside a", [[S10]], [[sq(2, 2, 5, 5)]], (1, 1), (1, 2)),
    ("b inside a touching from within at a point: the hole fuses into the shell", [[S10]], [[[(5, 0), (8, 4), (2, 4), (5, 0)]]], (1, 1), (1, 1)),
    ("a inside a hole of b", [[sq(5, 5, 7, 7)]], [DONUT], (0, 0), (1, 1)),
    ("b filling a hole of a exactly", [DONUT], [[sq(4, 4, 8, 8)]], (0, 0), (1, 2)),
    ("neighbours sharing an edge", [[S10]], [[sq(10, 0, 20, 10)]], (0, 0), (1, 1)),
    ("partially collinear shared edge, same side", [[S10]], [[sq(0, 2, 5, 5)]], (1, 1), (1, 1)),
    ("partially collinear shared edge, opposite side", [[S10]], [[sq(10, 2, 20, 8)]], (0, 0), (1, 1)),
    ("equal polygons", [[S10]], [[[(10, 0), (10, 10), (0, 10), (0, 0), (10, 0)]]], (1, 1), (0, 0)),
    ("corner-to-corner touch", [[S10]], [[sq(10, 10, 20, 20)]], (0, 0), (1, 1)),
    ("a bow-tie pair of parts: the junction rule keeps two rings", [[S10]], [[APEX]], (1, 1), (2, 2)),
    ("a's hole crossing b's hole", [DONUT], [[sq(2, 2, 14, 14), sq(6, 6, 10, 10, cw=True)]], (1, 2), (2, 2)),
    ("a comb giving many parts", [[COMB]], [[sq(-1, 6, 15, 8)]], (4, 4), (5, 5)),
    ("a vertex of one on an edge of the other", [[[(5, 10), (2, 5), (8, 5), (5, 10)]]], [[S10]], (1, 1), (0, 0)),
    ("a crossing exactly at a vertex", [[S10]], [[[(0, 0), (10, 10), (15, -5), (0, 0)]]], (1, 1), (1, 1)),
    ("a ring stored clockwise", [[sq(0, 0, 10, 10, cw=True)]], [[sq(5, 5, 15, 15)]], (1, 1), (1, 1)),
    ("a crossing at the point where a hole of b touches its shell", [[[(3, -2), (9, 4), (9, -2), (3, -2)]]], [[sq(0, -5, 5, 5), [(5, 0), (2, -1), (2, 1), (5, 0)]]],
     (1, 1), (1, 1)),
    ("a multipolygon of two parts against one polygon", [[sq(1, 1, 3, 3)], [sq(20, 20, 23, 23)]], [[sq(2, 2, 22, 22)]], (2, 2), (2, 2)),
]
UNCLOSED = [(0, 0), (4, 0), (4, 4), (0, 3)]


@lru_cache(maxsize=None)
def rows(ka, kb, n_random=100):
    """(rows of a, rows of b, validity of a, validity of b, names): the hand cases the two kinds can hold, null / empty / invalid-ring
    rows on either side, then the rows of overlay_ref.area_rows (hand cases of the area, stride rows, seeded random lattice stars against
    partners built to coincide with them) — of which a row that misses the 1e-6 gap is drawn again, that is, left out"""
    sel = [c for c in HAND_CASES if (ka == MPG or len(c[1]) == 1) and (kb == MPG or len(c[2]) == 1)]
    A, B = [P.as_row(ka, c[1]) for c in sel], [P.as_row(kb, c[2]) for c in sel]
    names = [c[0] for c in sel]
    av, bv = [1] * len(A), [1] * len(A)
    inner, donut_a, donut_b = P.as_row(ka, [[sq(2, 2, 5, 5)]]), P.as_row(ka, [DONUT]), P.as_row(kb, [DONUT])
    bad_a, bad_b = P.as_row(ka, [[UNCLOSED]]), P.as_row(kb, [[UNCLOSED]])
    for name, a, b, x, y in (("a null a", inner, donut_b, 0, 1), ("a null b", inner, donut_b, 1, 0), ("an empty a", [], donut_b, 1, 1),
                             ("an empty b", inner, [], 1, 1), ("an invalid ring in a", bad_a, donut_b, 1, 1), ("an invalid ring in b", donut_a, bad_b, 1, 1)):
        A.append(a), B.append(b), av.append(x), bv.append(y), names.append(name)
    RA, RB = O.area_rows(ka, kb, n_random)
    for i, (a, b) in enumerate(zip(RA, RB)):
        _parts, status, gap = clip(ka, a, kb, b, INTERSECTION)
        if gap is not None and gap < MIN_GAP:
            continue
        A.append(a), B.append(b), av.append(1), bv.append(1), names.append("area row %d" % i)
    return A, B, av, bv, names


def hand_expectations(ka, kb):
    """{row: ((parts, rings) of the intersection, (parts, rings) of the difference)} of the hand cases in rows(ka, kb)"""
    sel = [c for c in HAND_CASES if (ka == MPG or len(c[1]) == 1) and (kb == MPG or len(c[2]) == 1)]
    return {i: (c[3], c[4]) for i, c in enumerate(sel)}


def _row_starts(col):
    g = col.geom_offsets
    return col.ring_offsets[g[:-1]] if col.geom_type == PG else col.ring_offsets[col.part_offsets[g[:-1]]]


def pair_diagonals(ca, cb):
    """d of the contract for the identity pairs of two columns (NaN for a row without coordinates on either side)"""
    sa, sb = np.append(_row_starts(ca), len(ca.xy)), np.append(_row_starts(cb), len(cb.xy))
    out = np.full(ca.n_geoms, np.nan)
    for i in range(ca.n_geoms):
        a, b = ca.xy[sa[i]:sa[i + 1]], cb.xy[sb[i]:sb[i + 1]]
        if len(a) and len(b):
            both = np.concatenate([a, b])
            out[i] = np.sqrt(((both.max(axis=0) - both.min(axis=0)) ** 2).sum())
    return out


def expected_columns(ka, kb):
    """the fixture arrays of one family: the two input columns, and per mode the expected offsets, coordinates, tags and status"""
    A, B, av, bv, _names = rows(ka, kb)
    ca, cb = X.column(ka, A, av), X.column(kb, B, bv)
    sa, sb = _row_starts(ca), _row_starts(cb)
    out = {}
    O._pack("a_", ca, out)
    O._pack("b_", cb, out)
    out["a_valid"], out["b_valid"] = np.array(av, dtype=np.uint8), np.array(bv, dtype=np.uint8)
    for mode, mname in MODES.items():
        geom, part, ring, xy, tag, ea, eb, valid, status = [0], [0], [0], [], [], [], [], [], []
        for i, (a, b) in enumerate(zip(A, B)):
            parts, st, gap = clip(ka, a, kb, b, mode, bool(av[i]), bool(bv[i]))
            assert st != ST_UNRESOLVED and (gap is None or gap >= MIN_GAP), (NAMES[ka], NAMES[kb], i, st, gap)
            valid.append(0 if parts is None else 1)
            status.append(st)
            if parts is not None:
                ra, rb = row_rings(ka, a), row_rings(kb, b)
                for p in parts:
                    for r in p:
                        for pt in r:
                            t, e0, e1 = tag_point(pt, ra, rb)
                            tag.append(t)
                            ea.append(int(sa[i]) + e0 if t == TAG_X else -1)
                            eb.append(int(sb[i]) + e1 if t == TAG_X else -1)
                            xy.append((float(pt[0]), float(pt[1])))  # (Fraction -> float rounds correctly)
                        ring.append(len(xy))
                    part.append(len(ring) - 1)
            geom.append(len(part) - 1)
        key = mname + "_"
        out[key + "geom_offsets"] = np.array(geom, dtype=np.int32)
        out[key + "part_offsets"] = np.array(part, dtype=np.int32)
        out[key + "ring_offsets"] = np.array(ring, dtype=np.int32)
        out[key + "xy"] = np.array(xy, dtype=np.float64).reshape(-1, 2)
        out[key + "tag"] = np.array(tag, dtype=np.uint8)
        out[key + "ea"] = np.array(ea, dtype=np.int32)
        out[key + "eb"] = np.array(eb, dtype=np.int32)
        out[key + "valid"] = np.array(valid, dtype=np.uint8)
        out[key + "status"] = np.array(status, dtype=np.uint8)
    return out


def fixture_key(ka, kb):
    return f"{NAMES[ka]}_{NAMES[kb]}_"


def build_arrays():
    """every array of tests/golden/polyclip_lattice.npz"""
    out = {}
    for ka, kb in FAMILIES:
        for k, v in expected_columns(ka, kb).items():
            out[fixture_key(ka, kb) + k] = v
    return out


def fixture_bytes() -> bytes:
    buf = io.BytesIO()
    np.savez_compressed(buf, **build_arrays())
    return buf.getvalue()


def regenerate(path=GOLDEN):
    with open(path, "wb") as f:
        f.write(fixture_bytes())


def load(z, ka, kb, offset=(0.0, 0.0)):
    """(column a, column b) of one family of the fixture, translated by `offset`, with their validity"""
    key = fixture_key(ka, kb)
    ca, cb = O.unpack(z, key + "a_", ka, offset), O.unpack(z, key + "b_", kb, offset)
    ca.validity = np.packbits(z[key + "a_valid"].astype(bool), bitorder="little")
    cb.validity = np.packbits(z[key + "b_valid"].astype(bool), bitorder="little")
    return ca, cb


def _off_segment(pt, u, v):
    """distance of the points pt to the closed segments uv, around u"""
    e, w = v - u, pt - u
    s = np.clip((w * e).sum(axis=1) / (e * e).sum(axis=1), 0.0, 1.0)
    return np.sqrt(((w - s[:, None] * e) ** 2).sum(axis=1))


def check_result(z, ka, kb, mode, ca, cb, got, status=None, offset=(0.0, 0.0), rows_sel=None):
    """Compare a downloaded MULTIPOLYGON column `got` with the fixture's expectation for the family and mode: offsets, validity, status
    and ring starts exactly, input coordinates bit for bit, crossings within REL_TOL * d of both carrying edges.  `rows_sel`: the fixture
    row of every row of `got` (default: all, in order).  Returns the worst ratio of a crossing's distance to its bound."""
    key = fixture_key(ka, kb) + MODES[mode] + "_"
    geom, part, ring, xy, tag, ea, eb, valid, want_status = (z[key + n] for n in ("geom_offsets", "part_offsets", "ring_offsets", "xy", "tag", "ea", "eb",
                                                                                  "valid", "status"))
    sel = np.arange(len(valid)) if rows_sel is None else np.asarray(rows_sel)
    assert got.n_geoms == len(sel)
    gv = np.ones(len(sel), dtype=bool) if got.validity is None else np.unpackbits(got.validity, bitorder="little")[: len(sel)].astype(bool)
    assert (gv == valid[sel].astype(bool)).all(), np.nonzero(gv != valid[sel].astype(bool))[0][:10]
    if status is not None:
        assert (np.asarray(status) == want_status[sel]).all(), np.nonzero(np.asarray(status) != want_status[sel])[0][:10]
    n_parts = geom[sel + 1] - geom[sel]
    assert (np.diff(got.geom_offsets) == n_parts).all(), np.nonzero(np.diff(got.geom_offsets) != n_parts)[0][:10]
    empty = np.zeros(0, dtype=np.int64)
    want_parts = np.concatenate([np.arange(geom[r], geom[r + 1]) for r in sel] + [empty]).astype(np.int64)
    assert (np.diff(got.part_offsets) == part[want_parts + 1] - part[want_parts]).all()
    want_rings = np.concatenate([np.arange(part[k], part[k + 1]) for k in want_parts] + [empty]).astype(np.int64)
    sizes = ring[want_rings + 1] - ring[want_rings]
    assert (np.diff(got.ring_offsets) == sizes).all(), np.nonzero(np.diff(got.ring_offsets) != sizes)[0][:10]
    want_c = np.concatenate([np.arange(ring[k], ring[k + 1]) for k in want_rings] + [empty]).astype(np.int64)
    assert len(want_c) == len(got.xy)
    off = np.asarray(offset, dtype=np.float64)
    t = tag[want_c]
    exact = t == TAG_IN
    assert ((xy[want_c][exact] + off).view(np.uint64) == got.xy[exact].view(np.uint64)).all(), "an input coordinate is not returned bit for bit"
    xa = np.nonzero(t == TAG_X)[0]
    worst = 0.0
    if len(xa):
        pt, ia, ib = got.xy[xa], ea[want_c][xa], eb[want_c][xa]
        row = np.searchsorted(_row_starts(ca), ia, side="right") - 1
        d = pair_diagonals(ca, cb)[row]
        ratio = np.maximum(_off_segment(pt, ca.xy[ia], ca.xy[ia + 1]), _off_segment(pt, cb.xy[ib], cb.xy[ib + 1])) / (REL_TOL * d)
        worst = float(ratio.max())
        assert worst <= 1.0, (worst, int(xa[np.argmax(ratio)]))
        # (a crossing also lies where the exact one does: both carriers pin it unless they are nearly parallel)
    return worst


# ---- records of tests/polyclip_host_driver.cpp -------------------------------------------------------------------------------------------


def _edges_full(rings):
    """(first coordinate number, a, b, winding of the ring, hole flag) of every non-degenerate edge"""
    return [(c0 + k, c[k], c[k + 1], 1 if _shoelace2(c) > 0 else -1, int(hole)) for _m, hole, c0, c in rings for k in range(len(c) - 1) if c[k] != c[k + 1]]


def driver_records(ka, kb, mode, ca, cb) -> bytes:
    """the input records of the host driver for every pair of the family, with the coordinates of the (translated) columns ca, cb: per
    non-degenerate segment of every ring walk its exact touch points in REVERSE order, every piece as its exact class and, along an edge
    of the other row, the carrying edge"""
    A, B, av, bv, _names = rows(ka, kb)
    sa, sb = np.append(_row_starts(ca), len(ca.xy)), np.append(_row_starts(cb), len(cb.xy))
    buf = io.BytesIO()
    f8 = lambda *v: np.array(v, dtype=np.float64).tobytes()  # noqa: E731
    i4 = lambda *v: np.array(v, dtype=np.int32).tobytes()  # noqa: E731
    for i, (a, b) in enumerate(zip(A, B)):
        if P.usable(ka, a, bool(av[i])) is None or P.usable(kb, b, bool(bv[i])) is None:
            buf.write(i4(-1))
            continue
        xa, xb = ca.xy[sa[i]:sa[i + 1]], cb.xy[sb[i]:sb[i + 1]]
        o = (0.5 * max(xa[:, 0].min(), xb[:, 0].min()) + 0.5 * min(xa[:, 0].max(), xb[:, 0].max()),
             0.5 * max(xa[:, 1].min(), xb[:, 1].min()) + 0.5 * min(xa[:, 1].max(), xb[:, 1].max()))
        buf.write(i4(mode) + f8(*o))
        ra, rb = row_rings(ka, a), row_rings(kb, b)
        for rings_w, rings_o, xw, xo, start_w, start_o in ((ra, rb, xa, xb, int(sa[i]), int(sb[i])), (rb, ra, xb, xa, int(sb[i]), int(sa[i]))):
            edges_o, full_o = _edges(rings_o), _edges_full(rings_o)
            where = {}
            for _m, _h, c0, c in rings_o:
                for k, v in enumerate(c):
                    where.setdefault(v, c0 + k)

            own_where = {}
            for _m, _h, c0, c in rings_w:
                for k, v in enumerate(c):
                    own_where.setdefault(v, c0 + k)

            def piece(mid, p, q):
                pos = row_position(mid, rings_o)
                if pos:
                    return i4(pos) + f8(0, 0, 0, 0) + i4(0, 0)
                k, _a, _b, ccw, hole = next(e for e in full_o if _cross(e[1], e[2], p) == 0 and _cross(e[1], e[2], q) == 0 and _on_segment(mid, e[1], e[2]))
                return i4(2) + f8(*xo[k], *xo[k + 1]) + i4(ccw, hole)

            buf.write(i4(len(rings_w)))
            for _m, hole, c0, c in rings_w:
                rev = (_shoelace2(c) > 0) == hole
                idx = list(range(len(c)))[::-1] if rev else list(range(len(c)))
                segs, ip = [], 0
                for iq in range(1, len(idx)):
                    p, q = c[idx[ip]], c[idx[iq]]
                    if p == q:
                        continue
                    ts = _cuts(p, q, edges_o)
                    at = lambda t: (p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1]))  # noqa: E731
                    mids = [at((t0 + t1) / 2) for t0, t1 in zip(ts, ts[1:])]
                    edge = c0 + (idx[iq] if rev else idx[iq] - 1)
                    rec = i4(c0 + iq - 1, start_w + edge) + f8(*xw[c0 + idx[ip]], *xw[c0 + idx[iq]], *xw[edge], *xw[edge + 1])
                    rec += i4(int(row_position(p, rings_o) == 0)) + piece(mids[0], p, q) + piece(mids[-1], p, q) + i4(len(ts) - 2)
                    events = []
                    for k in range(1, len(ts) - 1):
                        pt = at(ts[k])
                        ipt = (int(pt[0]), int(pt[1])) if pt[0].denominator == 1 and pt[1].denominator == 1 else None
                        if ipt in where:
                            events.append(i4(0) + f8(*xo[where[ipt]]) + piece(mids[k - 1], p, q) + piece(mids[k], p, q))
                        else:
                            e = next(e for e in full_o if _cross(p, q, e[1]) * _cross(p, q, e[2]) < 0 and _on_segment(pt, e[1], e[2]))
                            own = own_where.get(ipt, -1)
                            events.append(i4(1) + f8(*xo[e[0]], *xo[e[0] + 1]) + i4(start_o + e[0], e[3], e[4], int(own >= 0)) + f8(*xw[max(own, 0)]))
                    segs.append(rec + b"".join(reversed(events)))
                    ip = iq
                buf.write(i4(c0, len(segs)) + b"".join(segs))
    return buf.getvalue()


def parse_driver_output(raw: bytes, n_pairs: int):
    """(MULTIPOLYGON column, status) of the driver's output for n_pairs pairs"""
    from geopolars_amd.geoarrow import GeoArrowArray

    at, geom, part, ring, xy, status, valid = 0, [0], [0], [0], [], [], []
    for _ in range(n_pairs):
        st, n_parts, n_rings, n_coords = (int(v) for v in np.frombuffer(raw, dtype=np.int32, count=4, offset=at))
        at += 16
        per_part = np.frombuffer(raw, dtype=np.int32, count=n_parts, offset=at)
        at += 4 * n_parts
        per_ring = np.frombuffer(raw, dtype=np.int32, count=n_rings, offset=at)
        at += 4 * n_rings
        xy.append(np.frombuffer(raw, dtype=np.float64, count=2 * n_coords, offset=at).reshape(-1, 2))
        at += 16 * n_coords
        assert per_part.sum() == n_rings and per_ring.sum() == n_coords
        for k in per_ring:
            ring.append(ring[-1] + int(k))
        for k in per_part:
            part.append(part[-1] + int(k))
        geom.append(len(part) - 1)
        status.append(st)
        valid.append(st not in (ST_NULL, ST_UNRESOLVED))
    assert at == len(raw)
    col = GeoArrowArray(MPG, np.concatenate(xy + [np.zeros((0, 2))]), geom_offsets=np.array(geom, dtype=np.int32), part_offsets=np.array(part, dtype=np.int32),
                        ring_offsets=np.array(ring, dtype=np.int32), validity=np.packbits(np.array(valid, dtype=bool), bitorder="little"))
    return col, np.array(status, dtype=np.uint8)


if __name__ == "__main__":
    regenerate()
