"""Exact reference of the line clip (gpk_line_clip, csrc/gpk_lineclip.h) and its fixture.

Not computed the way the kernel computes it (a walk from event to event with exact types and a depth): every segment is cut at ALL its
exact meets with the ring edges (relation_ref._cuts, Fractions), the rational midpoint of every piece is classified against every
member (exact_predicates._rational_pos), and maximal runs of kept pieces are collected.  A vertex of a part is tagged
    (TAG_L, i)      coordinate i of the line row
    (TAG_P, i)      coordinate i of the polygon row (a ring vertex on the open segment)
    (TAG_X, k)      crossing k: an exact rational point with the segment (p, q) and the ring edge (a, a + 1) that make it
All fixtures live on small integer lattices.  Rows are what tests/exact_ref.column takes."""
from __future__ import annotations

import io
import os
from fractions import Fraction
from functools import lru_cache

import numpy as np

from tests import exact_predicates as E
from tests import exact_ref as X
from tests import overlay_ref as O
from tests import polyrel_ref as P
from tests import relation_ref as R

LS, MLS, PG, MPG = R.LS, R.MLS, R.PG, R.MPG
NAMES = R.NAMES
FAMILIES = O.LENGTH_FAMILIES
INSIDE, OUTSIDE = 0, 1
MODES = {INSIDE: "inside", OUTSIDE: "outside"}
TAG_L, TAG_P, TAG_X = 0, 1, 2
MIN_GAP = Fraction(1, 10**6)  # the contract's condition: distinct transitions of a segment at least this far apart, relative to |pq|
REL_TOL = 1e-9  # a computed crossing lies within REL_TOL * d of its segment and of its ring edge, d = the diagonal of the pair's joint box
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lineclip_lattice.npz")
TRANSLATION = O.TRANSLATION
sq = R.sq


def kept(cls: int, mode: int) -> bool:
    return cls != R.EXTERIOR if mode == INSIDE else cls == R.EXTERIOR


# ---- the exact clip ------------------------------------------------------------------------------------------------------------------


def _flat_line(kl, row):
    """[(first coordinate number in the row, integer sequence)] of every sequence of a line row, empty ones included"""
    out, at = [], 0
    for s in R.line_seqs(kl, row):
        out.append((at, R._int_ring(s) if len(s) else np.zeros((0, 2), dtype=np.int64)))
        at += len(s)
    return out


def _flat_vertices(kp, row):
    """every coordinate of a polygonal row in storage order, and its non-degenerate edges as (coordinate number of a, a, b)"""
    polys = [row] if kp == PG else list(row)
    verts, edges = [], []
    for p in polys:
        for r in p:
            c = [(int(x), int(y)) for x, y in r]
            for k in range(len(c) - 1):
                if c[k] != c[k + 1]:
                    edges.append((len(verts) + k, c[k], c[k + 1]))
            verts.extend(c)
    return verts, edges


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def analyse(kl, row_l, kp, row_p, l_valid=True, p_valid=True):
    """None for a pair whose result row is null, else the pieces of every sequence: [(first coordinate number, [segment...])], a
    segment = (number of p, number of q, p, q, [(t0, t1, class)...]) for every p != q (p: the previous distinct coordinate)"""
    seqs_ok, polys = O._line_seqs(kl, row_l, l_valid), P.usable(kp, row_p, p_valid)
    if seqs_ok is None or polys is None:
        return None
    edges = E._edges([r for p in polys for r in p])
    dt = O.int_dtype(edges)  # (Python ints of any size: rows of arbitrary doubles on one integer grid, tests/hard_orient.on_integer_grid)
    elo = np.array([[min(a[0], b[0]), min(a[1], b[1])] for a, b in edges], dtype=dt).reshape(-1, 2)
    ehi = np.array([[max(a[0], b[0]), max(a[1], b[1])] for a, b in edges], dtype=dt).reshape(-1, 2)
    out = []
    for first, s in _flat_line(kl, row_l):
        c = [(int(x), int(y)) for x, y in s]
        segs, ip = [], 0
        for iq in range(1, len(c)):
            p, q = c[ip], c[iq]
            if p == q:
                continue
            ts = R._cuts(p, q, edges, elo, ehi)
            mids = [(p[0] + (t0 + t1) / 2 * (q[0] - p[0]), p[1] + (t0 + t1) / 2 * (q[1] - p[1])) for t0, t1 in zip(ts, ts[1:])]
            pos = R._positions(mids, polys)
            segs.append((first + ip, first + iq, p, q, [(t0, t1, int(w)) for (t0, t1), w in zip(zip(ts, ts[1:]), pos)]))
            ip = iq
        out.append((first, segs))
    return out


def clip(kl, row_l, kp, row_p, mode, l_valid=True, p_valid=True, pieces=None):
    """(parts, crossings, min_gap) of one pair, None for a null result row.  parts: a list of lists of (tag, number); crossings: a list
    of (x, y, number of p, number of q, number of a) with Fractions x, y; min_gap: the smallest distance between two distinct
    transition parameters of one segment (None when no segment has two)."""
    pieces = analyse(kl, row_l, kp, row_p, l_valid, p_valid) if pieces is None else pieces
    if pieces is None:
        return None
    verts, edges = _flat_vertices(kp, row_p)
    where = {}
    for k, v in enumerate(verts):
        where.setdefault(v, k)
    parts, crossings, min_gap = [], [], None

    def point(ip, iq, p, q, t):
        if t == 0:
            return (TAG_L, ip)
        if t == 1:
            return (TAG_L, iq)
        x, y = p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])
        if x.denominator == 1 and y.denominator == 1 and (int(x), int(y)) in where:
            return (TAG_P, where[(int(x), int(y))])
        for ia, a, b in edges:  # the ring edge that pq crosses properly at (x, y)
            if _cross(p, q, a) * _cross(p, q, b) < 0 and (b[0] - a[0]) * (y - a[1]) - (b[1] - a[1]) * (x - a[0]) == 0:
                crossings.append((x, y, ip, iq, ia))
                return (TAG_X, len(crossings) - 1)
        raise AssertionError(f"a transition at {(x, y)} that is neither a vertex nor a proper crossing")

    for _first, segs in pieces:
        open_ = False
        for ip, iq, p, q, pcs in segs:
            trans = []
            for k, (t0, _t1, cls) in enumerate(pcs):
                k_now = kept(cls, mode)
                if k > 0 and k_now != kept(pcs[k - 1][2], mode):
                    trans.append(t0)
                if k_now and not open_:
                    parts.append([point(ip, iq, p, q, t0)])
                    open_ = True
                elif not k_now and open_:
                    if t0 > 0:  # (at t0 == 0 the run ended at p, which it holds already)
                        parts[-1].append(point(ip, iq, p, q, t0))
                    open_ = False
            if open_:
                parts[-1].append((TAG_L, iq))
            for t0, t1 in zip(trans, trans[1:]):
                min_gap = t1 - t0 if min_gap is None else min(min_gap, t1 - t0)
    return parts, crossings, min_gap


def transition_gap(kl, row_l, kp, row_p, mode, l_valid=True, p_valid=True, pieces=None):
    """What the contract of gpk_lineclip.h conditions on, by the header's own definition: a transition is a touch point or a vertex of
    L where the kept-ness of the piece before differs from that of the piece after (the first and the last coordinate of a sequence
    have one piece only and are none).  Returns the least distance between two distinct transition points of one segment, as a share
    of the segment (a Fraction), None when no segment carries two.  Unlike `clip`'s min_gap it counts a transition at a vertex of L for
    both segments that meet there."""
    pieces = analyse(kl, row_l, kp, row_p, l_valid, p_valid) if pieces is None else pieces
    if pieces is None:
        return None
    best = None
    for _first, segs in pieces:
        trans, prev = [], None
        for _ip, _iq, _p, _q, pcs in segs:
            ks = [kept(cls, mode) for _t0, _t1, cls in pcs]
            here = {pcs[k][0] for k in range(1, len(pcs)) if ks[k] != ks[k - 1]}
            if prev is not None and prev != ks[0]:
                here.add(Fraction(0))
                trans[-1].add(Fraction(1))
            trans.append(here)
            prev = ks[-1]
        for here in trans:
            ts = sorted(here)
            for t0, t1 in zip(ts, ts[1:]):
                best = t1 - t0 if best is None else min(best, t1 - t0)
    return best


def scaled_back(result, scale):
    """A result of `clip` on rows that tests/hard_orient.on_integer_grid brought to an integer grid, in the units of the doubles
    (scale = hard_orient.integer_grid_scale of the same rows, a power of two).  The parts name coordinates of the two rows by number
    and need nothing: those come back bit for bit from the columns.  The crossings become (x, y, p, q, a) with Fractions x, y."""
    if result is None:
        return None
    parts, crossings, _gap = result
    return parts, [(Fraction(x) / scale, Fraction(y) / scale, ip, iq, ia) for x, y, ip, iq, ia in crossings]


def check_rows(want, cl, cp, got):
    """check_result for rows that are in no fixture file: `want[i]` is None (a null row) or (parts, crossings) of scaled_back for row
    i of the columns cl, cp, `got` the downloaded MULTILINESTRING column.  Offsets and validity exactly, (a) / (b) coordinates bit for
    bit, (c) within REL_TOL * d of the segment and of the ring edge.  Returns (the worst ratio of a (c) distance to its bound, the
    number of (c) coordinates)."""
    n = len(want)
    assert got.n_geoms == n == cl.n_geoms
    gv = np.ones(n, dtype=bool) if got.validity is None else np.unpackbits(got.validity, bitorder="little")[:n].astype(bool)
    wv = np.array([w is not None for w in want])
    assert (gv == wv).all(), np.nonzero(gv != wv)[0][:10]
    n_parts = np.array([0 if w is None else len(w[0]) for w in want])
    assert (np.diff(got.geom_offsets) == n_parts).all(), np.nonzero(np.diff(got.geom_offsets) != n_parts)[0][:10]
    sizes = np.array([len(pt) for w in want if w is not None for pt in w[0]], dtype=np.int64)
    assert (np.diff(got.ring_offsets) == sizes).all(), np.nonzero(np.diff(got.ring_offsets) != sizes)[0][:10]
    ls, ps, diag = _row_starts(cl), _row_starts(cp), pair_diagonals(cl, cp)
    at, worst, n_x = 0, 0.0, 0
    for i, w in enumerate(want):
        if w is None:
            continue
        for pt in w[0]:
            for tag, k in pt:
                g = got.xy[at]
                if tag == TAG_L:
                    assert g.tobytes() == cl.xy[ls[i] + k].tobytes(), (i, "a coordinate of the line is not returned bit for bit")
                elif tag == TAG_P:
                    assert g.tobytes() == cp.xy[ps[i] + k].tobytes(), (i, "a vertex of the polygon is not returned bit for bit")
                else:
                    _x, _y, ip, iq, ia = w[1][k]
                    far = max(_off_segment(g, cl.xy[ls[i] + ip], cl.xy[ls[i] + iq]), _off_segment(g, cp.xy[ps[i] + ia], cp.xy[ps[i] + ia + 1]))
                    worst, n_x = max(worst, far / (REL_TOL * diag[i])), n_x + 1
                    assert far <= REL_TOL * diag[i], (i, far, diag[i])
                at += 1
    assert at == len(got.xy)
    return worst, n_x


def _off_segment(pt, u, v):
    """distance of the point pt to the closed segment uv, around u"""
    e, w = v - u, pt - u
    s = min(1.0, max(0.0, float(w @ e) / float(e @ e)))
    return float(np.hypot(*(w - s * e)))


def measures(pieces, mode):
    """[(p, q, kept share of the parameter range as a Fraction)] over every non-degenerate segment"""
    return [(p, q, sum((t1 - t0 for t0, t1, cls in pcs if kept(cls, mode)), Fraction(0))) for _f, segs in pieces for _ip, _iq, p, q, pcs in segs]


# ---- hand cases: the smallest shapes that can go wrong ---------------------------------------------------------------------------------

S10, DONUT = P.S10, P.DONUT
TWO_WINDOWS = [sq(0, 0, 20, 12), sq(4, 4, 8, 8, cw=True), sq(12, 4, 16, 8, cw=True)]
# (name, line as a list of sequences, polygonal row as a list of polygons, parts INSIDE, parts OUTSIDE)
HAND_CASES = [
    ("a segment crossing a square twice", [[(-2, 5), (12, 5)]], [[S10]], 1, 2),
    ("ending exactly on a ring", [[(-3, 5), (0, 5)]], [[S10]], 0, 1),
    ("starting on a ring", [[(0, 5), (4, 5)]], [[S10]], 1, 0),
    ("along an edge, then leaving inward", [[(2, 0), (6, 0), (6, 4)]], [[S10]], 1, 0),
    ("along an edge, then leaving outward", [[(2, 0), (6, 0), (6, -4)]], [[S10]], 1, 1),
    ("inside one segment: interior, along an edge, interior", [[(2, 3), (2, 0), (8, 0), (8, 3)]], [[S10]], 1, 0),
    ("through a ring vertex", [[(-2, -2), (3, 3)]], [[S10]], 1, 1),
    ("grazing a ring vertex from outside", [[(-2, 2), (2, -2)]], [[S10]], 0, 1),
    ("through the point where a hole touches the shell", [[(6, -3), (6, 3)]], [R.HOLE_ON_SHELL], 0, 1),
    ("crossing the shell edge at the hole's vertex into the interior", [[(2, -1), (10, 1)]], [R.HOLE_ON_SHELL], 1, 1),
    ("through two holes: three inside parts from one segment", [[(-2, 6), (22, 6)]], [TWO_WINDOWS], 3, 4),
    ("a closed linestring around the polygon", [[(-2, -2), (12, -2), (12, 12), (-2, 12), (-2, -2)]], [[S10]], 0, 1),
    ("a closed linestring inside the polygon", [[(2, 2), (8, 2), (8, 8), (2, 2)]], [[S10]], 1, 0),
    ("wholly inside", [[(1, 1), (3, 2)]], [DONUT], 1, 0),
    ("wholly outside, within the box", [[(5, 5), (7, 6)]], [DONUT], 0, 1),
    ("repeated coordinates inside a run", [[(2, 2), (2, 2), (3, 2), (3, 2), (5, 2)]], [DONUT], 1, 0),
    ("repeated coordinates across a transition", [[(2, 2), (2, 2), (-3, 2), (-3, 2)]], [DONUT], 1, 1),
    ("a one-coordinate sequence and an empty member", [[(1, 1)], [], [(1, 1), (3, 2)]], [DONUT], 1, 0),
    ("the second member continues where the first ended", [[(1, 1), (3, 1)], [(3, 1), (5, 1)]], [DONUT], 2, 0),
    ("parts touching at a point on the line", [[(7, 5), (13, 5)]], R.PARTS, 1, 0),
    ("parts touching at a point, the line outside both", [[(11, 1), (10, 5), (11, 9)]], R.PARTS, 0, 1),
    ("the same stretch twice", [[(2, 0), (9, 0), (2, 0)]], [DONUT], 1, 0),
    ("in and out three times", [[(-1, 1), (1, 3), (-1, 5), (1, 7), (-1, 9)]], [[S10]], 2, 3),
]


@lru_cache(maxsize=None)
def rows(kl, kp, n_random=120):
    """(line rows, polygon rows, line validity, polygon validity, names): the hand cases the two kinds can hold, the ring-touch rows of
    relation_ref.TIES, null and empty rows on either side, then the rows of overlay_ref.length_rows"""
    sel = [c for c in HAND_CASES if (kl == MLS or len(c[1]) == 1) and (kp == MPG or len(c[2]) == 1)]
    lines = [O._as_line(kl, c[1]) if len(c[1]) == 1 else [list(s) for s in c[1]] for c in sel]
    polys = [P.as_row(kp, c[2]) for c in sel]
    names = [c[0] for c in sel]
    for name, tkp, poly, seq, _mask in R.TIES:
        if tkp == PG or kp == MPG:
            lines.append(O._as_line(kl, [seq]))
            polys.append(P.as_row(kp, [poly] if tkp == PG else poly))
            names.append(name)
    lv, pv = [1] * len(lines), [1] * len(lines)
    inside = O._as_line(kl, [[(1, 1), (3, 2)]])
    for name, line, poly, a, b in (("a null line", inside, P.as_row(kp, [DONUT]), 0, 1), ("a null polygon", inside, P.as_row(kp, [DONUT]), 1, 0),
                                   ("an empty line", [], P.as_row(kp, [DONUT]), 1, 1), ("an empty polygon", inside, [], 1, 1)):
        lines.append(line), polys.append(poly), lv.append(a), pv.append(b), names.append(name)
    L, Q = O.length_rows(kl, kp, n_random)
    lines += list(L)
    polys += list(Q)
    names += ["length row %d" % i for i in range(len(L))]
    n = len(lines)
    return lines, polys, lv + [1] * (n - len(lv)), pv + [1] * (n - len(pv)), names


def hand_expectations(kl, kp):
    """{row: (parts INSIDE, parts OUTSIDE)} of the hand cases in rows(kl, kp)"""
    sel = [c for c in HAND_CASES if (kl == MLS or len(c[1]) == 1) and (kp == MPG or len(c[2]) == 1)]
    return {i: (c[3], c[4]) for i, c in enumerate(sel)}


def _row_starts(col):
    """the first coordinate of every row of a column"""
    g = col.geom_offsets
    if col.geom_type == LS:
        return g[:-1]
    if col.geom_type in (MLS, PG):
        return col.ring_offsets[g[:-1]]
    return col.ring_offsets[col.part_offsets[g[:-1]]]


def pair_diagonals(cl, cp):
    """d of the contract for the identity pairs of two columns: the diagonal of the joint box of row i of each (NaN for a row without
    coordinates on either side)"""
    ls, ps = np.append(_row_starts(cl), len(cl.xy)), np.append(_row_starts(cp), len(cp.xy))
    out = np.full(cl.n_geoms, np.nan)
    for i in range(cl.n_geoms):
        a, b = cl.xy[ls[i]:ls[i + 1]], cp.xy[ps[i]:ps[i + 1]]
        if len(a) and len(b):
            both = np.concatenate([a, b])
            out[i] = np.sqrt(((both.max(axis=0) - both.min(axis=0)) ** 2).sum())
    return out


def expected_columns(kl, kp):
    """the fixture arrays of one family: the two input columns, and per mode the expected offsets, coordinates and tags"""
    lines, polys, lv, pv, _names = rows(kl, kp)
    cl, cp = X.column(kl, lines, lv), X.column(kp, polys, pv)
    ls, ps = _row_starts(cl), _row_starts(cp)
    out = {}
    O._pack("a_", cl, out)
    O._pack("b_", cp, out)
    out["a_valid"], out["b_valid"] = np.array(lv, dtype=np.uint8), np.array(pv, dtype=np.uint8)
    pieces = [analyse(kl, a, kp, b, bool(x), bool(y)) for a, b, x, y in zip(lines, polys, lv, pv)]
    for mode, mname in MODES.items():
        geom, part, xy, tag, num, cross, valid = [0], [0], [], [], [], [], []
        for i, (a, b) in enumerate(zip(lines, polys)):
            r = None if pieces[i] is None else clip(kl, a, kp, b, mode, pieces=pieces[i])
            valid.append(0 if r is None else 1)
            if r is not None:
                parts, crossings, gap = r
                assert gap is None or gap >= MIN_GAP, (NAMES[kl], NAMES[kp], i, gap)
                for pt in parts:
                    assert len(pt) >= 2
                    for t, k in pt:
                        tag.append(t)
                        if t == TAG_L:
                            num.append(int(ls[i]) + k)
                            xy.append(tuple(cl.xy[num[-1]]))
                        elif t == TAG_P:
                            num.append(int(ps[i]) + k)
                            xy.append(tuple(cp.xy[num[-1]]))
                        else:
                            x, y, ip, iq, ia = crossings[k]
                            num.append(len(cross))
                            cross.append((int(ls[i]) + ip, int(ls[i]) + iq, int(ps[i]) + ia, x.numerator, x.denominator, y.numerator, y.denominator))
                            xy.append((float(x), float(y)))  # (Fraction -> float rounds correctly)
                    part.append(len(xy))
            geom.append(len(part) - 1)
        key = mname + "_"
        out[key + "geom_offsets"] = np.array(geom, dtype=np.int32)
        out[key + "part_offsets"] = np.array(part, dtype=np.int32)
        out[key + "xy"] = np.array(xy, dtype=np.float64).reshape(-1, 2)
        out[key + "tag"] = np.array(tag, dtype=np.uint8)
        out[key + "num"] = np.array(num, dtype=np.int32)
        out[key + "cross"] = np.array(cross, dtype=np.int64).reshape(-1, 7)
        out[key + "valid"] = np.array(valid, dtype=np.uint8)
    return out


def fixture_key(kl, kp):
    return f"{NAMES[kl]}_{NAMES[kp]}_"


def build_arrays():
    """every array of tests/golden/lineclip_lattice.npz"""
    out = {}
    for kl, kp in FAMILIES:
        for k, v in expected_columns(kl, kp).items():
            out[fixture_key(kl, kp) + k] = v
    return out


def fixture_bytes() -> bytes:
    buf = io.BytesIO()
    np.savez_compressed(buf, **build_arrays())
    return buf.getvalue()


def regenerate(path=GOLDEN):
    with open(path, "wb") as f:
        f.write(fixture_bytes())


def load(z, kl, kp, offset=(0.0, 0.0)):
    """(lines column, polygons column) of one family of the fixture, translated by `offset`, with their validity"""
    key = fixture_key(kl, kp)
    cl, cp = O.unpack(z, key + "a_", kl, offset), O.unpack(z, key + "b_", kp, offset)
    cl.validity = np.packbits(z[key + "a_valid"].astype(bool), bitorder="little")
    cp.validity = np.packbits(z[key + "b_valid"].astype(bool), bitorder="little")
    return cl, cp


def check_result(z, kl, kp, mode, cl, cp, got, offset=(0.0, 0.0), rows_sel=None):
    """Compare a downloaded MULTILINESTRING column `got` with the fixture's expectation for the family and mode: offsets and validity
    exactly, (a) / (b) coordinates bit for bit, (c) within REL_TOL * d of the segment and of the ring edge.  `rows_sel`: the fixture row of
    every row of `got` (default: all, in order).  Returns the worst ratio of a (c) distance to its bound."""
    key = fixture_key(kl, kp) + MODES[mode] + "_"
    geom, part, tag, num, cross, valid = (z[key + n] for n in ("geom_offsets", "part_offsets", "tag", "num", "cross", "valid"))
    sel = np.arange(len(valid)) if rows_sel is None else np.asarray(rows_sel)
    assert got.n_geoms == len(sel)
    gv = np.ones(len(sel), dtype=bool) if got.validity is None else np.unpackbits(got.validity, bitorder="little")[: len(sel)].astype(bool)
    assert (gv == valid[sel].astype(bool)).all(), np.nonzero(gv != valid[sel].astype(bool))[0][:10]
    n_parts = geom[sel + 1] - geom[sel]
    assert (np.diff(got.geom_offsets) == n_parts).all(), np.nonzero(np.diff(got.geom_offsets) != n_parts)[0][:10]
    want_parts = np.concatenate([np.arange(geom[r], geom[r + 1]) for r in sel] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    sizes = part[want_parts + 1] - part[want_parts]
    assert (np.diff(got.ring_offsets) == sizes).all(), np.nonzero(np.diff(got.ring_offsets) != sizes)[0][:10]
    want_c = np.concatenate([np.arange(part[k], part[k + 1]) for k in want_parts] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    assert len(want_c) == len(got.xy)
    t, k = tag[want_c], num[want_c]
    la, pa = t == TAG_L, t == TAG_P
    assert (got.xy[la].view(np.uint64) == cl.xy[k[la]].view(np.uint64)).all(), "a coordinate of the line is not returned bit for bit"
    assert (got.xy[pa].view(np.uint64) == cp.xy[k[pa]].view(np.uint64)).all(), "a vertex of the polygon is not returned bit for bit"
    xa = np.nonzero(t == TAG_X)[0]
    worst = 0.0
    if len(xa):
        c = cross[k[xa]]
        pt, p, q, a, b = got.xy[xa], cl.xy[c[:, 0]], cl.xy[c[:, 1]], cp.xy[c[:, 2]], cp.xy[c[:, 2] + 1]
        row = np.searchsorted(_row_starts(cl), c[:, 0], side="right") - 1  # the fixture row of every crossing
        d = pair_diagonals(cl, cp)[row]

        def off_segment(u, v):  # distance of pt to the closed segment uv, around u
            e, w = v - u, pt - u
            s = np.clip((w * e).sum(axis=1) / (e * e).sum(axis=1), 0.0, 1.0)
            return np.sqrt(((w - s[:, None] * e) ** 2).sum(axis=1))

        ratio = np.maximum(off_segment(p, q), off_segment(a, b)) / (REL_TOL * d)
        worst = float(ratio.max())
        assert worst <= 1.0, (worst, int(xa[np.argmax(ratio)]))
    return worst


# ---- records of tests/lineclip_host_driver.cpp -------------------------------------------------------------------------------------------


def driver_case(kl, kp, mode, cl, cp):
    """(input records, expectations) for the host driver over every non-degenerate segment of every usable pair of the family, with the
    coordinates of the (translated) columns cl, cp.  A record hands the segment's touch points over in REVERSE order with their exact
    types; an expectation is the list of sink calls (begin_part, event number or -1, tag, x, y) plus (p, q, d) and per event (a, b)."""
    lines, polys, lv, pv, _names = rows(kl, kp)
    ls, ps, diag = _row_starts(cl), _row_starts(cp), pair_diagonals(cl, cp)
    buf, want = io.BytesIO(), []
    f8 = lambda *v: np.array(v, dtype=np.float64).tobytes()  # noqa: E731
    i4 = lambda *v: np.array(v, dtype=np.int32).tobytes()  # noqa: E731
    for i, (a_row, b_row) in enumerate(zip(lines, polys)):
        pieces = analyse(kl, a_row, kp, b_row, bool(lv[i]), bool(pv[i]))
        if pieces is None:
            continue
        verts, edges = _flat_vertices(kp, b_row)
        where = {}
        for k, v in enumerate(verts):
            where.setdefault(v, k)
        la, pa = cl.xy[ls[i]:(ls[i + 1] if i + 1 < len(ls) else len(cl.xy))], cp.xy[ps[i]:(ps[i + 1] if i + 1 < len(ps) else len(cp.xy))]
        o = (0.5 * max(la[:, 0].min(), pa[:, 0].min()) + 0.5 * min(la[:, 0].max(), pa[:, 0].max()),
             0.5 * max(la[:, 1].min(), pa[:, 1].min()) + 0.5 * min(la[:, 1].max(), pa[:, 1].max()))
        for _first, segs in pieces:
            for ip, iq, p, q, pcs in segs:
                P_, Q_ = cl.xy[ls[i] + ip], cl.xy[ls[i] + iq]
                events = []  # in exact order: (kind, type, a, b, tag)
                for k in range(1, len(pcs)):
                    t = pcs[k][0]
                    x, y = p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])
                    typ = int(kept(pcs[k][2], mode)) - int(kept(pcs[k - 1][2], mode))
                    if x.denominator == 1 and y.denominator == 1 and (int(x), int(y)) in where:
                        v = cp.xy[ps[i] + where[(int(x), int(y))]]
                        events.append((0, typ, v, v, TAG_P))
                    else:
                        ia = next(ia for ia, a, b in edges
                                  if _cross(p, q, a) * _cross(p, q, b) < 0 and (b[0] - a[0]) * (y - a[1]) - (b[1] - a[1]) * (x - a[0]) == 0)
                        events.append((1, typ, cp.xy[ps[i] + ia], cp.xy[ps[i] + ia + 1], TAG_X))
                n = len(events)
                kept0 = kept(pcs[0][2], mode)
                buf.write(i4(mode, int(kept0)) + f8(*P_, *Q_, *o) + i4(n))
                for kind, typ, a, b, _tag in reversed(events):
                    buf.write(i4(kind, typ) + f8(*a, *b))
                calls, open_ = ([(1, -1, TAG_L, P_[0], P_[1])] if kept0 else []), kept0
                for k, (kind, typ, a, b, tag) in enumerate(events):
                    if typ:
                        calls.append((1 if typ > 0 else 0, n - 1 - k, tag, a[0], a[1]))  # (a crossing: x, y are not compared)
                        open_ = typ > 0
                if open_:
                    calls.append((0, -1, TAG_L, Q_[0], Q_[1]))
                want.append((calls, P_, Q_, diag[i], [(a, b) for _k, _t, a, b, _g in reversed(events)]))
    return buf.getvalue(), want


if __name__ == "__main__":
    regenerate()
