"""Exact reference of the polygon union (gpk_polygon_union, csrc/gpk_polyunion.h) and its fixture.

Built on the exact helpers of tests/polyclip_ref.py (every segment cut at ALL its exact meets with the other row, rational midpoints
classified by crossing numbers, the side of a shared edge from the carrying ring's signed area, arcs linked by EXACT POINT EQUALITY,
the junction order from exact cross and dot products of the true neighbours, ring signs from shoelace areas), with the kept table of
the union, and with its own nesting: a hole goes to the enclosing shell of the SMALLEST exact area — the innermost one, found without
asking which shell encloses which.  tests/test_polyunion_ref.py pins this file by identities it shares no code with.  All fixtures live
on small integer lattices; rows are what tests/exact_ref.column takes."""
from __future__ import annotations

import io
import os
from fractions import Fraction
from functools import cmp_to_key, lru_cache

import numpy as np

from tests import exact_ref as X
from tests import overlay_ref as O
from tests import polyclip_ref as L
from tests import polyrel_ref as P

PG, MPG, NAMES, FAMILIES = L.PG, L.MPG, L.NAMES, L.FAMILIES
UNION = 0
MODES = {UNION: "union"}
WALK_A, WALK_B = L.WALK_A, L.WALK_B
INT, SAME, EXT, OPP = L.INT, L.SAME, L.EXT, L.OPP
ST_OK, ST_TOUCH, ST_EMPTY, ST_NULL, ST_UNRESOLVED = L.ST_OK, L.ST_TOUCH, L.ST_EMPTY, L.ST_NULL, L.ST_UNRESOLVED
MIN_GAP, REL_TOL, TRANSLATION = L.MIN_GAP, L.REL_TOL, L.TRANSLATION
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polyunion_lattice.npz")
sq, S10, DONUT = L.sq, L.S10, L.DONUT


def kept(cls: int, walk: int, mode: int) -> bool:
    """the kept table of gpk_polyunion.h"""
    assert mode == UNION
    return cls == EXT if walk == WALK_B else cls in (EXT, SAME)


def _walk_arcs(rings_w, rings_o, walk, mode, gaps):
    """the arcs of one walk (polyclip_ref._walk_arcs with the table above; nothing is emitted backwards)"""
    edges_o = L._edges(rings_o)
    arcs = []
    for _m, hole, c0, c in rings_w:
        w = c if (L._shoelace2(c) > 0) != hole else c[::-1]  # interior on the left
        pieces, ip = [], 0
        for iq in range(1, len(w)):
            p, q = w[ip], w[iq]
            if p == q:
                continue
            ts = L._cuts(p, q, edges_o)
            gaps.extend(t1 - t0 for t0, t1 in zip(ts, ts[1:]))
            for t0, t1 in zip(ts, ts[1:]):
                tm = (t0 + t1) / 2
                mid = (p[0] + tm * (q[0] - p[0]), p[1] + tm * (q[1] - p[1]))
                cls = L._piece_class(mid, p, q, rings_o, edges_o)
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
            return cur[4] and prev[3] in (INT, EXT) and cur[3] in (INT, EXT) and L.row_position(cur[2], rings_o) == 0

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
    return arcs


def stitch(arcs):
    """(parts, status): polyclip_ref.stitch with the innermost nesting — parts = a list of lists of closed rings of exact points, shell
    first; None when the arcs do not close"""
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
            cmp = L._cw_order(E, back)
            k = sorted(cand, key=cmp_to_key(lambda i, j: cmp(arcs[i]["pts"][1], arcs[j]["pts"][1])))[0]
            if k == k0:
                break
        ring.append(ring[0])
        rings.append(ring)
    status = ST_TOUCH if any(len(set(r[:-1])) != len(r) - 1 for r in rings) else ST_OK
    signs = [L._shoelace2(r) for r in rings]
    if any(s == 0 for s in signs):
        return None, ST_UNRESOLVED
    shells = [k for k, s in enumerate(signs) if s > 0]
    holes_of = {k: [] for k in shells}
    for k, s in enumerate(signs):
        if s > 0:
            continue
        around = [sh for sh in shells if next((v for v in (L.ring_position(t, rings[sh]) for t in rings[k][:-1]) if v != 0), 0) > 0]
        if not around:
            return None, ST_UNRESOLVED
        holes_of[min(around, key=lambda sh: signs[sh])].append(k)
    parts = [[rings[sh]] + [rings[h] for h in holes_of[sh]] for sh in shells]
    return parts, (ST_EMPTY if not parts else status)


def union(ka, row_a, kb, row_b, mode=UNION, a_valid=True, b_valid=True):
    """(parts, status, min gap) of one pair; parts None for a null result row"""
    if P.usable(ka, row_a, a_valid) is None or P.usable(kb, row_b, b_valid) is None:
        return None, ST_NULL, None
    ra, rb = L.row_rings(ka, row_a), L.row_rings(kb, row_b)
    gaps = []
    arcs = _walk_arcs(ra, rb, WALK_A, mode, gaps) + _walk_arcs(rb, ra, WALK_B, mode, gaps)
    parts, status = stitch(arcs)
    return parts, status, (min(gaps) if gaps else None)


def transition_gap(ka, row_a, kb, row_b, mode=UNION):
    """polyclip_ref.transition_gap with the kept table of the union: the least distance between two distinct transition points of one
    segment, as a share of the segment; None when no segment carries two"""
    return L.transition_gap(ka, row_a, kb, row_b, mode, kept_fn=kept)


area_of, row_area = L.area_of, L.row_area
scaled_back, shape_of, counts_of, check_rows = L.scaled_back, L.shape_of, L.counts_of, L.check_rows


# ---- hand cases: (name, a, b, {mode: (rings per part, coordinates per ring — the closing one included —, status)}), stated by hand; None: what
# the reference says ------------------------------------------------------------------------------------------------------------------------
C_SHAPE = [(0, 0), (10, 0), (10, 3), (3, 3), (3, 7), (10, 7), (10, 10), (0, 10), (0, 0)]  # open to the right between y = 3 and y = 7
NOTCHED = [(10, 2), (15, 2), (15, 8), (10, 8), (12, 5), (10, 2)]  # touches x = 10 at two points around a triangular gap
BIG_RING = [sq(0, 0, 20, 20), sq(4, 4, 16, 16, cw=True)]
SMALL_RING = [sq(6, 6, 14, 14), sq(8, 8, 12, 12, cw=True)]
HAND_CASES = [
    ("disjoint squares", [[S10]], [[sq(20, 0, 30, 10)]], {UNION: ([1, 1], [5, 5], 0)}),
    ("equal squares", [[S10]], [[[(10, 0), (10, 10), (0, 10), (0, 0), (10, 0)]]], {UNION: ([1], [5], 0)}),
    ("squares sharing a whole edge", [[S10]], [[sq(10, 0, 20, 10)]], {UNION: ([1], [7], 0)}),
    ("squares sharing part of an edge", [[S10]], [[sq(10, 2, 20, 8)]], {UNION: ([1], [9], 0)}),
    ("squares overlapping at a corner", [[S10]], [[sq(5, 5, 15, 15)]], {UNION: ([1], [9], 0)}),
    ("two bars forming a plus", [[sq(0, 4, 12, 8)]], [[sq(4, 0, 8, 12)]], {UNION: ([1], [13], 0)}),
    ("b strictly inside a", [[S10]], [[sq(2, 2, 5, 5)]], {UNION: ([1], [5], 0)}),
    ("b inside a's hole", [DONUT], [[sq(5, 5, 7, 7)]], {UNION: ([2, 1], [5, 5, 5], 0)}),
    ("annulus b inside the hole of annulus a: the innermost shell", [BIG_RING], [SMALL_RING], {UNION: ([2, 2], [5, 5, 5, 5], 0)}),
    ("corner touching corner", [[S10]], [[sq(10, 10, 20, 20)]], {UNION: ([1, 1], [5, 5], 0)}),
    ("touching at two points around a gap", [[S10]], [[NOTCHED]], {UNION: ([1, 1], [7, 6], 0)}),
    ("a C closed by a bar that overlaps both ends", [[C_SHAPE]], [[sq(8, 1, 12, 9)]], {UNION: ([2], [9, 5], 0)}),
    ("a C closed by a wedge that overlaps one end and touches the other at a point", [[C_SHAPE]], [[[(8, 1), (12, 1), (10, 7), (8, 1)]]], {UNION: None}),
    ("b equal to a's hole", [DONUT], [[sq(4, 4, 8, 8)]], {UNION: ([1], [5], 0)}),
    ("b overlapping a's hole partly", [DONUT], [[sq(6, 6, 10, 10)]], {UNION: ([2], [5, 7], 0)}),
    ("a multipolygon whose two members each overlap b", [[sq(0, 0, 4, 4)], [sq(10, 0, 14, 4)]], [[sq(2, 1, 12, 3)]], {UNION: ([1], [13], 0)}),
    ("a crossing exactly at a vertex of a on an edge of b", [[S10]], [[[(-2, -2), (15, -5), (12, 12), (-2, -2)]]], {UNION: ([1], [7], 0)}),
    ("the comb against a bar through its teeth", [[L.COMB]], [[sq(-1, 6, 15, 8)]], {UNION: ([4], [25, 5, 5, 5], 0)}),
    ("two thin rectangles crossing", [[L.THIN_A]], [[L.THIN_B]], {UNION: ([1], [13], 0)}),
    ("an apex on the top edge of a square", [[S10]], [[L.APEX]], {UNION: ([1], [10], 0)}),
]


def _hand_selection(ka, kb):
    return [c for c in HAND_CASES if (ka == MPG or len(c[1]) == 1) and (kb == MPG or len(c[2]) == 1)]


@lru_cache(maxsize=None)
def rows(ka, kb):
    """(rows of a, rows of b, validity of a, validity of b, names): the hand cases the two kinds can hold, then every row of
    polyclip_ref.rows (its hand cases, its null / empty / invalid-ring rows, its random lattice rows).  A row whose pair misses the 1e-6
    gap is left out: no fixture row may come back unresolved."""
    sel = _hand_selection(ka, kb)
    A, B = [P.as_row(ka, c[1]) for c in sel], [P.as_row(kb, c[2]) for c in sel]
    names = [c[0] for c in sel]
    av, bv = [1] * len(A), [1] * len(A)
    LA, LB, lav, lbv, lnames = L.rows(ka, kb)
    for a, b, x, y, name in zip(LA, LB, lav, lbv, lnames):
        _parts, status, gap = union(ka, a, kb, b, UNION, bool(x), bool(y))
        if status == ST_UNRESOLVED or (gap is not None and gap < MIN_GAP):
            continue
        A.append(a), B.append(b), av.append(x), bv.append(y), names.append("clip: " + name)
    return A, B, av, bv, names


def hand_expectations(ka, kb):
    """{row: {mode: (rings per part, coordinates per ring, status) or None}} of the hand cases in rows(ka, kb)"""
    return {i: c[3] for i, c in enumerate(_hand_selection(ka, kb))}


def expected_columns(ka, kb):
    """the fixture arrays of one family: the two input columns, and per mode the expected offsets, coordinates, tags and status (the
    layout of polyclip_ref.expected_columns)"""
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
            parts, st, gap = union(ka, a, kb, b, mode, bool(av[i]), bool(bv[i]))
            assert st != ST_UNRESOLVED and (gap is None or gap >= MIN_GAP), (NAMES[ka], NAMES[kb], i, st, gap)
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
    """every array of tests/golden/polyunion_lattice.npz"""
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


load = L.load  # (column a, column b) of one family of the fixture: the input arrays have polyclip_ref's names


class _AsClipFixture:
    """this fixture's arrays of one mode under the names polyclip_ref.check_result reads its first mode by"""

    def __init__(self, z, mode):
        self.z, self.mine, self.theirs = z, MODES[mode] + "_", L.MODES[L.INTERSECTION] + "_"

    def __getitem__(self, key):
        return self.z[key.replace("_" + self.theirs, "_" + self.mine)]


def check_result(z, ka, kb, mode, ca, cb, got, status=None, offset=(0.0, 0.0), rows_sel=None):
    """polyclip_ref.check_result — offsets, validity, status and ring starts exactly, input coordinates bit for bit, crossings within
    REL_TOL * d of both carrying edges — against this fixture's expectation for the family and mode.  Returns the worst ratio of a
    crossing's distance to its bound."""
    return L.check_result(_AsClipFixture(z, mode), ka, kb, L.INTERSECTION, ca, cb, got, status, offset, rows_sel)


# ---- exact point membership: one rational sample point strictly inside every face of the arrangement of the two rows' edges ------------------


def face_samples(ra, rb):
    """a point strictly inside every bounded face of the arrangement of all edges of both rows (and in some unbounded ones): the plane is
    cut into vertical slabs at every vertex and every exact meet, and on the middle line of each slab the midpoints between consecutive
    edge crossings are taken"""
    edges = [(a, b) for _k, a, b, _l in L._edges(ra) + L._edges(rb)]
    xs = {Fraction(v[0]) for e in edges for v in e}
    ea, eb = L._edges(ra), L._edges(rb)
    for _k, p, q, _l in ea:
        for t in L._cuts(p, q, eb):
            xs.add(p[0] + t * (q[0] - p[0]))
    xs = sorted(xs)
    out = []
    for x0, x1 in zip(xs, xs[1:]):
        x = (x0 + x1) / 2
        ys = sorted({a[1] + Fraction(x - a[0]) * (b[1] - a[1]) / (b[0] - a[0]) for a, b in edges if a[0] != b[0] and min(a[0], b[0]) < x < max(a[0], b[0])})
        out.extend((x, (y0 + y1) / 2) for y0, y1 in zip(ys, ys[1:]))
    return out


def in_parts(t, parts) -> bool:
    """is the exact point t (on no ring) inside the result: inside a shell and outside its holes"""
    return any(L.ring_position(t, p[0]) > 0 and all(L.ring_position(t, h) < 0 for h in p[1:]) for p in parts)


# ---- records of tests/polyunion_host_driver.cpp: the format of tests/polyclip_host_driver.cpp, over this fixture's rows ----------------------


def driver_records(ka, kb, mode, ca, cb) -> bytes:
    """the input records of the host driver for every pair of the family (polyclip_ref.driver_records over rows() of this file): per
    non-degenerate segment of every ring walk its exact touch points in REVERSE order, every piece as its exact class and, along an edge
    of the other row, the carrying edge"""
    A, B, av, bv, _names = rows(ka, kb)
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


parse_driver_output = L.parse_driver_output


if __name__ == "__main__":
    regenerate()
