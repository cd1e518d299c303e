"""Exact reference of the polygon symmetric difference (gpk_polygon_symdiff, csrc/gpk_polysymdiff.h) and its fixture.

On Fractions and by other means than the header: no piece classes, no table, no levels.  Every segment of every ring of either row is
cut at ALL its exact meets with the other row (polyclip_ref._cuts).  A piece is kept iff exactly one of its two SIDES lies in exactly
one of the rows: a rational sample point is put a little to the left and a little to the right of an inner point of the piece — so
little that the way there meets no edge of either row — and each is located in a and in b by crossing numbers.  A kept piece is
directed so that the side in the result is on its left.  Pieces are joined into arcs only to NAME them (the key convention of the
header decides ring starts and part order and nothing else), arcs are linked by EXACT POINT EQUALITY, the junction order comes from
exact cross and dot products of the true neighbours, ring signs from shoelace areas, and a hole goes to the enclosing shell of the
smallest exact area (polyunion_ref.stitch).  tests/test_polysymdiff_ref.py pins this file by identities it shares no code with.  All
fixtures live on small integer lattices; rows are what tests/exact_ref.column takes."""
from __future__ import annotations

import io
import os
from fractions import Fraction
from functools import lru_cache

import numpy as np

from tests import exact_ref as X
from tests import overlay_ref as O
from tests import polyclip_ref as L
from tests import polyrel_ref as P
from tests import polyunion_ref as U

PG, MPG, NAMES, FAMILIES = L.PG, L.MPG, L.NAMES, L.FAMILIES
SYMDIFF = 0
MODES = {SYMDIFF: "symmetric_difference"}
WALK_A, WALK_B = L.WALK_A, L.WALK_B
ST_OK, ST_TOUCH, ST_EMPTY, ST_NULL, ST_UNRESOLVED = L.ST_OK, L.ST_TOUCH, L.ST_EMPTY, L.ST_NULL, L.ST_UNRESOLVED
MIN_GAP, REL_TOL, TRANSLATION = L.MIN_GAP, L.REL_TOL, L.TRANSLATION
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polysymdiff_lattice.npz")
sq, S10, DONUT = L.sq, L.S10, L.DONUT


# ---- the two sides of a piece ------------------------------------------------------------------------------------------------------------


def _meets(m, s, a, b, p, q):
    """does the way from m (an inner point of a piece of pq, no vertex of any ring) to s meet the edge ab anywhere but at m"""
    if L._cross(a, b, m) == 0 and L._on_segment(m, a, b):
        assert L._cross(a, b, p) == 0 and L._cross(a, b, q) == 0, "an edge through the inside of a piece that does not run along it"
        return False  # (the piece's own edge, or one it shares: the way leaves their carrier at m)
    c1, c2, c3, c4 = L._cross(m, s, a), L._cross(m, s, b), L._cross(a, b, m), L._cross(a, b, s)
    if (c1 > 0) != (c2 > 0) and c1 != 0 and c2 != 0 and (c3 > 0) != (c4 > 0) and c3 != 0 and c4 != 0:
        return True
    return (c4 == 0 and L._on_segment(s, a, b)) or (c1 == 0 and L._on_segment(a, m, s)) or (c2 == 0 and L._on_segment(b, m, s))


def _sides_in_result(p, q, t0, t1, ra, rb, edges, vertices):
    """(is the left side in the result, is the right side) of the piece [t0, t1] of the segment p -> q"""
    k = 2
    while True:  # an inner point of the piece that is no vertex (a ring of the same row may touch the segment there)
        tm = t0 + (t1 - t0) / k
        m = (p[0] + tm * (q[0] - p[0]), p[1] + tm * (q[1] - p[1]))
        if m not in vertices:
            break
        k += 1
    out = []
    for sign in (1, -1):
        eps = Fraction(1, 4)
        while True:
            s = (m[0] - sign * eps * (q[1] - p[1]), m[1] + sign * eps * (q[0] - p[0]))
            lo, hi = (min(m[0], s[0]), min(m[1], s[1])), (max(m[0], s[0]), max(m[1], s[1]))
            near = (e for e in edges if not (max(e[1][0], e[2][0]) < lo[0] or min(e[1][0], e[2][0]) > hi[0] or max(e[1][1], e[2][1]) < lo[1]
                                             or min(e[1][1], e[2][1]) > hi[1]))  # (the cheap test first)
            if not any(_meets(m, s, a, b, p, q) for _k, a, b, _l in near):
                break
            eps /= 2
        pa, pb = L.row_position(s, ra), L.row_position(s, rb)
        assert pa != 0 and pb != 0
        out.append((pa == L.INT) != (pb == L.INT))
    return out[0], out[1]


def _walk_arcs(rings_w, rings_o, ra, rb, walk, gaps):
    """the arcs of one walk: dicts with pts (exact points in the EMITTED direction, both ends included), key, whole.  The key of an
    arc is (walk, segment of its emitted start, 0 at the segment's first coordinate / 1 inside it, its rank among the arcs of its ring
    in the order in which the walk ENDS them — the arc that holds the ring's first piece last): the header's key, with the arc number
    that breaks its ties."""
    edges_o = L._edges(rings_o)
    edges = L._edges(ra) + L._edges(rb)
    vertices = {v for _m, _h, _c0, c in ra + rb for v in c}
    arcs = []
    for _m, hole, c0, c in rings_w:
        w = c if (L._shoelace2(c) > 0) != hole else c[::-1]  # interior on the left
        pieces, ip = [], 0  # (segment, t0, start, kept, backwards)
        for iq in range(1, len(w)):
            p, q = w[ip], w[iq]
            if p == q:
                continue
            ts = L._cuts(p, q, edges_o)
            gaps.extend(t1 - t0 for t0, t1 in zip(ts, ts[1:]))
            for t0, t1 in zip(ts, ts[1:]):
                left, right = _sides_in_result(p, q, t0, t1, ra, rb, edges, vertices)
                start = (p[0] + t0 * (q[0] - p[0]), p[1] + t0 * (q[1] - p[1]))
                pieces.append((c0 + iq - 1, t0, start, left != right, right))
            ip = iq
        n = len(pieces)
        if not any(pc[3] for pc in pieces):
            continue
        # an arc ends wherever the boundary of the other row is met: there a piece is dropped, turns round, or may touch another ring
        brk = [pieces[i - 1][3] != pieces[i][3] or (pieces[i][3] and L.row_position(pieces[i][2], rings_o) == 0) for i in range(n)]
        breaks = [i for i in range(n) if brk[i]]
        if not breaks:
            pts = [pc[2] for pc in pieces if pc[1] == 0]
            pts = pts + [pts[0]]
            arcs.append({"pts": pts[::-1] if pieces[0][4] else pts, "key": (walk, c0, 0, 0), "whole": True})
            continue
        ring_arcs = []
        for i in breaks:
            if not pieces[i][3]:
                continue
            pts, j = [pieces[i][2]], i + 1
            while not brk[j % n]:
                assert pieces[j % n][1] == 0 and pieces[j % n][4] == pieces[i][4]  # (a piece turns round only on the other row's boundary)
                pts.append(pieces[j % n][2])
                j += 1
            pts.append(pieces[j % n][2])
            back = pieces[i][4]
            at = pieces[j % n] if back else pieces[i]  # the piece that begins where the emitted arc starts
            holds_first = i == 0 or j > n
            ring_arcs.append({"pts": pts[::-1] if back else pts, "seg": at[0], "inside": 0 if at[1] == 0 else 1, "whole": False, "ended": (holds_first, j)})
        for rank, a in enumerate(sorted(ring_arcs, key=lambda a: a["ended"])):
            a["key"] = (walk, a["seg"], a["inside"], rank)
        arcs.extend(ring_arcs)
    return arcs


stitch = U.stitch  # arcs by key, links by exact point equality, the leftmost turn, shoelace signs, the innermost shell


def symdiff(ka, row_a, kb, row_b, mode=SYMDIFF, a_valid=True, b_valid=True):
    """(parts, status, min gap) of one pair; parts None for a null result row"""
    assert mode == SYMDIFF
    if P.usable(ka, row_a, a_valid) is None or P.usable(kb, row_b, b_valid) is None:
        return None, ST_NULL, None
    ra, rb = L.row_rings(ka, row_a), L.row_rings(kb, row_b)
    gaps = []
    arcs = _walk_arcs(ra, rb, ra, rb, WALK_A, gaps) + _walk_arcs(rb, ra, ra, rb, WALK_B, gaps)
    parts, status = stitch(arcs)
    return parts, status, (min(gaps) if gaps else None)


def arc_count(ka, row_a, kb, row_b) -> int:
    """the number of arcs of a pair under this rule (what decides between the LDS slice and the global scratch of the stitch)"""
    ra, rb = L.row_rings(ka, row_a), L.row_rings(kb, row_b)
    return len(_walk_arcs(ra, rb, ra, rb, WALK_A, [])) + len(_walk_arcs(rb, ra, ra, rb, WALK_B, []))


def comb_pair(teeth, free):
    """(row of a as a multipolygon, row of b as a polygon) with a known number of arcs: a comb of `teeth` teeth of width 2 and height
    10 on a base of height 4 (the comb of tests/test_gpu_polyclip.py) crossed by a bar through its teeth — every tooth crosses the bar
    four times, and under this rule every crossing ends an arc of either walk: 8 arcs a tooth — with `free` further members of a far
    from the bar, one whole arc each.  With teeth = 0: two squares that overlap at a corner, 4 arcs."""
    if teeth == 0:
        a_row, b_row = [[S10]], [sq(5, 5, 15, 15)]
    else:
        ring = [(0, 0), (4 * teeth - 2, 0)]
        for k in range(teeth - 1, -1, -1):
            ring += [(4 * k + 2, 10), (4 * k, 10)] + ([(4 * k, 4), (4 * k - 2, 4)] if k else [])
        a_row, b_row = [[ring + [(0, 0)]]], [sq(-1, 6, 4 * teeth + 1, 8)]
    return a_row + [[sq(100 + 4 * k, 100, 102 + 4 * k, 102)] for k in range(free)], b_row


# (teeth, free members) of the pairs with one arc less than the stitch's LDS slice, exactly the slice, and one arc more, by lanes
SLICE_SHAPES = {4: [(0, 3), (1, 0), (1, 1)], 16: [(3, 7), (4, 0), (4, 1)]}


area_of, row_area = L.area_of, L.row_area
scaled_back, shape_of, counts_of, check_rows = L.scaled_back, L.shape_of, L.counts_of, L.check_rows
face_samples, in_parts = U.face_samples, U.in_parts


def canonical(parts):
    """a result up to ring rotation and part order: what the swap (b, a) leaves of the result of (a, b)"""
    if parts is None:
        return None

    def ring(r):
        body = r[:-1]
        k = body.index(min(body))
        return tuple(body[k:] + body[:k])

    return sorted(tuple([ring(p[0])] + sorted(ring(h) for h in p[1:])) for p in parts)


# ---- hand cases: (name, a, b, (rings per part, coordinates per ring — the closing one included —, status)), stated by hand ----------------
TRI_UP = [(0, 0), (12, 0), (6, 12), (0, 0)]
TRI_DOWN = [(0, 8), (6, -4), (12, 8), (0, 8)]
S20 = sq(0, 0, 20, 20)
HAND_CASES = [
    ("two triangles crossing six times: six parts that touch at the crossings", [[TRI_UP]], [[TRI_DOWN]], ([1] * 6, [4] * 6, ST_OK)),
    ("squares overlapping at a corner: two parts that touch at both crossings", [[S10]], [[sq(5, 5, 15, 15)]], ([1, 1], [7, 7], ST_OK)),
    ("equal polygons: empty", [[S10]], [[[(10, 0), (10, 10), (0, 10), (0, 0), (10, 0)]]], ([], [], ST_EMPTY)),
    ("edge neighbours: merged", [[S10]], [[sq(10, 0, 20, 10)]], ([1], [7], ST_OK)),
    ("neighbours sharing part of an edge", [[S10]], [[sq(10, 2, 20, 8)]], ([1], [9], ST_OK)),
    ("a shared edge with the interiors on the same side", [[S10]], [[sq(0, 2, 5, 5)]], ([1], [9], ST_OK)),
    ("b inside a: a hole, b's ring kept whole backwards", [[S10]], [[sq(2, 2, 5, 5)]], ([2], [5, 5], ST_OK)),
    ("a inside b: a's ring kept whole backwards", [[sq(2, 2, 5, 5)]], [[S10]], ([2], [5, 5], ST_OK)),
    ("annulus b inside a: a shell inside a hole", [[S20]], [U.SMALL_RING], ([2, 1], [5, 5, 5], ST_OK)),
    ("annulus b in the hole of annulus a", [U.BIG_RING], [U.SMALL_RING], ([2, 2], [5, 5, 5, 5], ST_OK)),
    ("b touching a from inside at a vertex: one ring twice through the point", [[S10]], [[[(5, 0), (8, 4), (2, 4), (5, 0)]]], ([1], [9], ST_TOUCH)),
    ("a crossing exactly at a vertex of a third ring, a's first piece kept backwards", [[[(3, -2), (9, 4), (9, -2), (3, -2)]]],
     [[sq(0, -5, 5, 5), [(5, 0), (2, -1), (2, 1), (5, 0)]]], ([1, 1], [5, 11], ST_TOUCH)),
    ("a ring whose first piece is kept backwards", [[sq(5, 5, 15, 15)]], [[S10]], ([1, 1], [7, 7], ST_OK)),
    ("corner touching corner", [[S10]], [[sq(10, 10, 20, 20)]], ([1, 1], [5, 5], ST_OK)),
    ("two bars forming a plus: four parts", [[sq(0, 4, 12, 8)]], [[sq(4, 0, 8, 12)]], ([1] * 4, [5] * 4, ST_OK)),
    ("b equal to a's hole: the hole is filled", [DONUT], [[sq(4, 4, 8, 8)]], ([1], [5], ST_OK)),
    ("a multipolygon whose two members each overlap b", [[sq(0, 0, 4, 4)], [sq(10, 0, 14, 4)]], [[sq(2, 1, 12, 3)]], ([1, 1, 1], [5, 9, 9], ST_OK)),
]


def _hand_selection(ka, kb):
    return [c for c in HAND_CASES if (ka == MPG or len(c[1]) == 1) and (kb == MPG or len(c[2]) == 1)]


@lru_cache(maxsize=None)
def rows(ka, kb):
    """(rows of a, rows of b, validity of a, validity of b, names): the hand cases the two kinds can hold, then every row of
    polyunion_ref.rows — the input rows of tests/golden/polyunion_lattice.npz, its null / empty / invalid-ring rows among them
    (tests/golden/make_polysymdiff_golden.py checks them against that file).  A row whose pair misses the 1e-6 gap is left out."""
    sel = _hand_selection(ka, kb)
    A, B = [P.as_row(ka, c[1]) for c in sel], [P.as_row(kb, c[2]) for c in sel]
    names = [c[0] for c in sel]
    av, bv = [1] * len(A), [1] * len(A)
    found = [symdiff(ka, a, kb, b) for a, b in zip(A, B)]
    UA, UB, uav, ubv, unames = U.rows(ka, kb)
    for a, b, x, y, name in zip(UA, UB, uav, ubv, unames):
        res = symdiff(ka, a, kb, b, SYMDIFF, bool(x), bool(y))
        if res[1] == ST_UNRESOLVED or (res[2] is not None and res[2] < MIN_GAP):
            continue
        A.append(a), B.append(b), av.append(x), bv.append(y), names.append("union: " + name), found.append(res)
    _RESULTS[(ka, kb)] = found
    return A, B, av, bv, names


_RESULTS = {}


def results(ka, kb):
    """[(parts, status, min gap)] of every row of rows(ka, kb), computed once"""
    rows(ka, kb)
    return _RESULTS[(ka, kb)]


def hand_expectations(ka, kb):
    """{row: (rings per part, coordinates per ring, status)} of the hand cases in rows(ka, kb)"""
    return {i: c[3] for i, c in enumerate(_hand_selection(ka, kb))}


def hand_row(ka, kb, name_start):
    """the row of the hand case whose name starts with `name_start`"""
    return next(i for i, c in enumerate(_hand_selection(ka, kb)) if c[0].startswith(name_start))


def expected_columns(ka, kb):
    """the fixture arrays of one family: the two input columns, and the expected offsets, coordinates, tags and status (the layout of
    polyclip_ref.expected_columns)"""
    A, B, av, bv, _names = rows(ka, kb)
    ca, cb = X.column(ka, A, av), X.column(kb, B, bv)
    sa, sb = L._row_starts(ca), L._row_starts(cb)
    out = {}
    O._pack("a_", ca, out)
    O._pack("b_", cb, out)
    out["a_valid"], out["b_valid"] = np.array(av, dtype=np.uint8), np.array(bv, dtype=np.uint8)
    for mode, mname in MODES.items():
        geom, part, ring, xy, tag, ea, eb, valid, status = [0], [0], [0], [], [], [], [], [], []
        for i, (a, b) in enumerate(zip(A, B)):
            parts, st, gap = results(ka, kb)[i]
            assert st != ST_UNRESOLVED and (gap is None or gap >= MIN_GAP), (NAMES[ka], NAMES[kb], i, st, gap)  # the 1e-6 gap, on every row
            valid.append(0 if parts is None else 1)
            status.append(st)
            if parts is not None:
                ra, rb = L.row_rings(ka, a), L.row_rings(kb, b)
                for p in parts:
                    for r in p:
                        for pt in r:
                            t, e0, e1 = L.tag_point(pt, ra, rb)
                            tag.append(t)
                            ea.append(int(sa[i]) + e0 if t == L.TAG_X else -1)
                            eb.append(int(sb[i]) + e1 if t == L.TAG_X else -1)
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


fixture_key = L.fixture_key


def build_arrays():
    """every array of tests/golden/polysymdiff_lattice.npz"""
    out = {}
    for ka, kb in FAMILIES:
        for k, v in expected_columns(ka, kb).items():
            out[fixture_key(ka, kb) + k] = v
    return out


def fixture_bytes() -> bytes:
    buf = io.BytesIO()
    np.savez_compressed(buf, **build_arrays())
    return buf.getvalue()


load = L.load  # (column a, column b) of one family of the fixture: the input arrays have polyclip_ref's names


class _AsClipFixture:
    """this fixture's arrays under the names polyclip_ref.check_result reads its first mode by"""

    def __init__(self, z, mode):
        self.z, self.mine, self.theirs = z, MODES[mode] + "_", L.MODES[L.INTERSECTION] + "_"

    def __getitem__(self, key):
        return self.z[key.replace("_" + self.theirs, "_" + self.mine)]


def check_result(z, ka, kb, mode, ca, cb, got, status=None, offset=(0.0, 0.0), rows_sel=None):
    """polyclip_ref.check_result — offsets, validity, status and ring starts exactly, input coordinates bit for bit, crossings within
    REL_TOL * d of both carrying edges — against this fixture's expectation for the family.  Returns the worst ratio of a crossing's
    distance to its bound."""
    return L.check_result(_AsClipFixture(z, mode), ka, kb, L.INTERSECTION, ca, cb, got, status, offset, rows_sel)


# ---- records of tests/polysymdiff_host_driver.cpp: the format of tests/polyclip_host_driver.cpp, over given rows ---------------------------


def driver_records(ka, kb, mode, ca, cb, the_rows=None) -> bytes:
    """the input records of the host driver for every pair of `the_rows` (default: rows(ka, kb)) with the coordinates of the columns
    ca, cb: per non-degenerate segment of every ring walk its exact touch points in REVERSE order, every piece as its exact class
    and, along an edge of the other row, the carrying edge (the records of polyclip_ref.driver_records)"""
    A, B, av, bv, _names = rows(ka, kb) if the_rows is None else the_rows
    sa, sb = np.append(L._row_starts(ca), len(ca.xy)), np.append(L._row_starts(cb), len(cb.xy))
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
        ra, rb = L.row_rings(ka, a), L.row_rings(kb, b)
        for rings_w, rings_o, xw, xo, start_w, start_o in ((ra, rb, xa, xb, int(sa[i]), int(sb[i])), (rb, ra, xb, xa, int(sb[i]), int(sa[i]))):
            edges_o, full_o = L._edges(rings_o), L._edges_full(rings_o)
            where, own_where = {}, {}
            for _m, _h, c0, c in rings_o:
                for k, v in enumerate(c):
                    where.setdefault(v, c0 + k)
            for _m, _h, c0, c in rings_w:
                for k, v in enumerate(c):
                    own_where.setdefault(v, c0 + k)

            def piece(mid, p, q):
                pos = L.row_position(mid, rings_o)
                if pos:
                    return i4(pos) + f8(0, 0, 0, 0) + i4(0, 0)
                k, _a, _b, ccw, hole = next(e for e in full_o if L._cross(e[1], e[2], p) == 0 and L._cross(e[1], e[2], q) == 0 and L._on_segment(mid, e[1], e[2]))
                return i4(2) + f8(*xo[k], *xo[k + 1]) + i4(ccw, hole)

            buf.write(i4(len(rings_w)))
            for _m, hole, c0, c in rings_w:
                rev = (L._shoelace2(c) > 0) == hole
                idx = list(range(len(c)))[::-1] if rev else list(range(len(c)))
                segs, ip = [], 0
                for iq in range(1, len(idx)):
                    p, q = c[idx[ip]], c[idx[iq]]
                    if p == q:
                        continue
                    ts = L._cuts(p, q, edges_o)
                    at = lambda t: (p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1]))  # noqa: E731
                    mids = [at((t0 + t1) / 2) for t0, t1 in zip(ts, ts[1:])]
                    edge = c0 + (idx[iq] if rev else idx[iq] - 1)
                    rec = i4(c0 + iq - 1, start_w + edge) + f8(*xw[c0 + idx[ip]], *xw[c0 + idx[iq]], *xw[edge], *xw[edge + 1])
                    rec += i4(int(L.row_position(p, rings_o) == 0)) + piece(mids[0], p, q) + piece(mids[-1], p, q) + i4(len(ts) - 2)
                    events = []
                    for k in range(1, len(ts) - 1):
                        pt = at(ts[k])
                        ipt = (int(pt[0]), int(pt[1])) if pt[0].denominator == 1 and pt[1].denominator == 1 else None
                        if ipt in where:
                            events.append(i4(0) + f8(*xo[where[ipt]]) + piece(mids[k - 1], p, q) + piece(mids[k], p, q))
                        else:
                            e = next(e for e in full_o if L._cross(p, q, e[1]) * L._cross(p, q, e[2]) < 0 and L._on_segment(pt, e[1], e[2]))
                            own = own_where.get(ipt, -1)
                            events.append(i4(1) + f8(*xo[e[0]], *xo[e[0] + 1]) + i4(start_o + e[0], e[3], e[4], int(own >= 0)) + f8(*xw[max(own, 0)]))
                    segs.append(rec + b"".join(reversed(events)))
                    ip = iq
                buf.write(i4(c0, len(segs)) + b"".join(segs))
    return buf.getvalue()


def swapped_rows(ka, kb):
    """rows(ka, kb) with a and b exchanged: rows for the family (kb, ka)"""
    A, B, av, bv, names = rows(ka, kb)
    return B, A, bv, av, names


parse_driver_output = L.parse_driver_output
