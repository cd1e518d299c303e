"""Exact reference of linear referencing (closest point, locate / project, interpolate) over the f64 inputs.

Rows are described as in tests/exact_ref.py: (kind, rows), rows[i] a POINT (x, y) (None: empty), a MULTIPOINT's list of points, a
LINESTRING's list of coordinates, a MULTILINESTRING's list of linestrings, a POLYGON's list of closed rings or a MULTIPOLYGON's list
of polygons.  Squared distances, the parameter t and the nearest point q are `fractions.Fraction`; measures are `decimal` values at
60 digits (square roots by Decimal.sqrt).  Segment indices are LOCAL: coordinate positions within the row, in storage order;
coord_base() gives the row's first coordinate in the column's buffer.

No GPU and no library call here: tests/test_linref_ref.py pins this module on hand-made answers.
"""
import decimal
from fractions import Fraction

import numpy as np

from geopolars_amd import _abi, synth
from geopolars_amd.geoarrow import GeoArrowArray
from tests import exact_ref as X

DEC = decimal.Context(prec=60)
Q_REL = 2.0**-48  # closest point: each component within Q_REL * max(|p|, |s|, |e|) (largest magnitudes) of the exact point
M_REL = 1e-9  # measures and interpolated points: within M_REL * total length


def F(v) -> Fraction:
    return Fraction(float(v))


def dec(q: Fraction) -> decimal.Decimal:
    return DEC.divide(decimal.Decimal(q.numerator), decimal.Decimal(q.denominator))


def dec_sqrt(q: Fraction) -> decimal.Decimal:
    return DEC.sqrt(dec(q))


def sequences(kind: int, row):
    """[(local index of the first coordinate, coordinates)] of the row's non-empty coordinate sequences, in storage order"""
    out, at = [], 0
    for s in X.row_seqs(kind, row):
        if len(s):
            out.append((at, [(float(c[0]), float(c[1])) for c in s]))
            at += len(s)
    return out


def segments(kind: int, row):
    """[(start index, end index, s, e)] in storage order; a one-coordinate sequence is the degenerate segment (i, i, s, s)"""
    out = []
    for at, s in sequences(kind, row):
        if len(s) == 1:
            out.append((at, at, s[0], s[0]))
        out += [(at + i, at + i + 1, s[i], s[i + 1]) for i in range(len(s) - 1)]
    return out


def seg_len2(s, e) -> Fraction:
    return (F(e[0]) - F(s[0])) ** 2 + (F(e[1]) - F(s[1])) ** 2


def seg_nearest(p, s, e):
    """(squared distance, t, (qx, qy)) of the point of the closed segment se nearest to p, exactly"""
    px, py, sx, sy, ex, ey = F(p[0]), F(p[1]), F(s[0]), F(s[1]), F(e[0]), F(e[1])
    dx, dy = ex - sx, ey - sy
    d2 = dx * dx + dy * dy
    t = Fraction(0) if d2 == 0 else min(max(((px - sx) * dx + (py - sy) * dy) / d2, Fraction(0)), Fraction(1))
    qx, qy = sx + t * dx, sy + t * dy
    return (px - qx) ** 2 + (py - qy) ** 2, t, (qx, qy)


def _f64_dists(p, segs):
    a = np.array([s[2] for s in segs], dtype=np.float64)
    b = np.array([s[3] for s in segs], dtype=np.float64)
    return X._f64_seg_dist(np.asarray(p, dtype=np.float64), a, b), float(np.max(np.hypot(*(b - a).T)))


def q_bound(p, s, e) -> float:
    return Q_REL * max(abs(p[0]), abs(p[1]), abs(s[0]), abs(s[1]), abs(e[0]), abs(e[1]))


def closest(p, kind: int, row):
    """None for an empty row, else a dict:
      inside   the row is polygonal and p is inside or on it (then d2 = 0, seg = -1, q = p)
      d2       exact minimum squared distance
      seg, end local coordinate indices of the LOWEST-index minimising segment
      s, e     its ends; t, q: the exact parameter and nearest point
      near     [(seg, d2, q)] of every segment whose squared distance is within 1e-9 relative of the minimum (for ambiguous())"""
    if X.row_is_empty(kind, row):
        return None
    segs = segments(kind, row)
    if not segs:
        return None
    if kind in X.POLYGONAL and X.geom_position(p, [g for g in X.row_polys(kind, row) if len(g) and len(g[0])]) >= 0:
        return {"inside": True, "d2": Fraction(0), "seg": -1, "end": -1, "t": Fraction(0), "q": (F(p[0]), F(p[1])), "near": []}
    df, lmax = _f64_dists(p, segs)
    cut = np.min(df) * (1 + 1e-6) + 1e-9 * (lmax + np.max(np.abs(p)) * 1e-6)
    cand = [(segs[i], seg_nearest(p, segs[i][2], segs[i][3])) for i in np.flatnonzero(df <= cut)]
    best = min(c[1][0] for c in cand)
    (i0, i1, s, e), (d2, t, q) = next(c for c in cand if c[1][0] == best)  # candidates are in index order: the lowest index
    near = [(sg[0], r[0], r[2]) for sg, r in cand if r[0] <= best * (1 + Fraction(1, 10**9))]
    return {"inside": False, "d2": d2, "seg": i0, "end": i1, "s": s, "e": e, "t": t, "q": q, "near": near}


def ambiguous(p, res) -> bool:
    """some segment's exact minimum squared distance is within relative 1e-12 of the best and its nearest point differs from the
    best q by more than the accuracy bound: f64 arithmetic may then pick either.  Segments that meet at the winning vertex have
    the same nearest point and never count."""
    if res is None or res["inside"]:
        return False
    tol = q_bound(p, res["s"], res["e"])
    lim = res["d2"] * (1 + Fraction(1, 10**12))
    for seg, d2, q in res["near"]:
        if seg != res["seg"] and d2 <= lim and max(abs(q[0] - res["q"][0]), abs(q[1] - res["q"][1])) > tol:
            return True
    return False


def on_some_segment(q, kind, row, tol: float) -> bool:
    """q (floats) lies within tol (per component, of its nearest point) of some segment of the row"""
    segs = segments(kind, row)
    df, _ = _f64_dists(q, segs)
    for i in np.flatnonzero(df <= np.min(df) + 4 * tol):
        _, _, n = seg_nearest(q, segs[i][2], segs[i][3])
        if max(abs(F(q[0]) - n[0]), abs(F(q[1]) - n[1])) <= tol:
            return True
    return False


def lengths(kind: int, row):
    """[(start index, Decimal length)] of the row's segments with two ends, in storage order (the gap between members has none)"""
    return [(i0, dec_sqrt(seg_len2(s, e))) for i0, i1, s, e in segments(kind, row) if i1 != i0]


def total_length(kind: int, row) -> decimal.Decimal:
    return sum((l for _, l in lengths(kind, row)), decimal.Decimal(0))


def measure(kind: int, row, res, normalized: bool = False) -> decimal.Decimal:
    """the measure of res["q"] on segment res["seg"]: lengths of the segments before it plus t |e - s|"""
    before = sum((l for i, l in lengths(kind, row) if i < res["seg"]), decimal.Decimal(0))
    m = DEC.add(before, DEC.multiply(dec(res["t"]), dec_sqrt(seg_len2(res["s"], res["e"]))))
    if normalized:
        L = total_length(kind, row)
        return decimal.Decimal(0) if L == 0 else DEC.divide(m, L)
    return m


def locate(p, kind: int, row, normalized: bool = False):
    res = closest(p, kind, row)
    return None if res is None else measure(kind, row, res, normalized)


def interpolate(kind: int, row, d, normalized: bool = False):
    """(x, y) as Decimals (a vertex: exactly its coordinates), or None for an empty row or a NaN distance.  The first-segment rule:
    the point lies on the first segment in storage order whose cumulative end measure is >= d."""
    seqs = sequences(kind, row)
    if not seqs or d != d:
        return None
    first = seqs[0][1][0]
    segs = [(s, e, dec_sqrt(seg_len2(s, e))) for i0, i1, s, e in segments(kind, row) if i1 != i0]
    L = sum((l for _, _, l in segs), decimal.Decimal(0))
    if L == 0:
        return decimal.Decimal(first[0]), decimal.Decimal(first[1])
    if d in (float("inf"), float("-inf")):
        d = L if d > 0 else decimal.Decimal(0)
    else:
        d = decimal.Decimal(float(d))
        if normalized:
            d = DEC.multiply(d, L)
        if d < 0:
            d = DEC.add(d, L)
        d = min(max(d, decimal.Decimal(0)), L)
    cum = decimal.Decimal(0)
    for s, e, l in segs:
        m0, cum = cum, DEC.add(cum, l)
        if cum >= d:
            if cum == d:
                return decimal.Decimal(e[0]), decimal.Decimal(e[1])
            if d <= m0 or l == 0:
                return decimal.Decimal(s[0]), decimal.Decimal(s[1])
            t = DEC.divide(DEC.subtract(d, m0), l)
            return tuple(DEC.add(decimal.Decimal(s[k]), DEC.multiply(t, DEC.subtract(decimal.Decimal(e[k]), decimal.Decimal(s[k])))) for k in (0, 1))
    e = segs[-1][1]
    return decimal.Decimal(e[0]), decimal.Decimal(e[1])


def dec_err(got: float, exact) -> float:
    """|got - exact| for an exact Fraction or Decimal"""
    if isinstance(exact, Fraction):
        return float(abs(Fraction(float(got)) - exact))
    return float(abs(DEC.subtract(decimal.Decimal(float(got)), exact)))


# ---- columns ------------------------------------------------------------------------------------------------------------------


def rows_of(a: GeoArrowArray):
    """(kind, rows) of a host column (validity not looked at)"""
    k, xy, go = a.geom_type, a.xy, a.geom_offsets
    c = lambda i0, i1: [(float(x), float(y)) for x, y in xy[i0:i1]]  # noqa: E731
    n = len(a)
    if k == _abi.GEOM_POINT:
        return k, [None if np.isnan(xy[i, 0]) else (float(xy[i, 0]), float(xy[i, 1])) for i in range(n)]
    if k in (_abi.GEOM_MULTIPOINT, _abi.GEOM_LINESTRING):
        return k, [c(go[i], go[i + 1]) for i in range(n)]
    ro = a.ring_offsets
    if k in (_abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON):
        return k, [[c(ro[r], ro[r + 1]) for r in range(go[i], go[i + 1])] for i in range(n)]
    po = a.part_offsets
    return k, [[[c(ro[r], ro[r + 1]) for r in range(po[q], po[q + 1])] for q in range(go[i], go[i + 1])] for i in range(n)]


def coord_base(a: GeoArrowArray, j: int) -> int:
    """index, in the column's coordinate buffer, of row j's first coordinate"""
    k = a.geom_type
    if k == _abi.GEOM_POINT:
        return j
    g = int(a.geom_offsets[j])
    if k in (_abi.GEOM_MULTIPOINT, _abi.GEOM_LINESTRING):
        return g
    if k in (_abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON):
        return int(a.ring_offsets[g])
    return int(a.ring_offsets[a.part_offsets[g]])


def grouped_lines(lines: GeoArrowArray, seed: int) -> GeoArrowArray:
    """a MULTILINESTRING column whose rows are 1 to 3 consecutive linestrings of `lines`"""
    rng = np.random.default_rng(seed)
    cuts = [0]
    while cuts[-1] < len(lines):
        cuts.append(min(len(lines), cuts[-1] + int(rng.integers(1, 4))))
    return GeoArrowArray(_abi.GEOM_MULTILINESTRING, lines.xy, geom_offsets=np.array(cuts, dtype=np.int32), ring_offsets=lines.geom_offsets)


def random_columns():
    """{name: (column, points (n, 2))}: the random columns of the mirror test and the GPU test, point i against row i.  Even
    points are uniform over the domain, odd ones lie within the row's extent around its middle (inside and near cases)."""
    lines = synth.random_linestrings(160, seed=11)
    cols = {
        "linestrings": lines,
        "multilinestrings": grouped_lines(synth.random_linestrings(300, seed=12, max_log2=6.0), 13),
        "star_polygons": synth.star_polygons(120, 32, seed=14),
        "clustered_polygons": synth.clustered_polygons(160, seed=15),
        "powerlaw_multipolygons": synth.powerlaw_multipolygons(160, seed=16, cap=400),
    }
    out = {}
    for k, (name, col) in enumerate(cols.items()):
        rng = np.random.default_rng(100 + k)
        n = len(col)
        pts = rng.uniform(0.0, synth.DOMAIN, (n, 2))
        for i in range(1, n, 2):
            c0 = coord_base(col, i)
            c1 = coord_base(col, i + 1) if i + 1 < n else col.n_coords
            if c1 > c0:
                lo, hi = col.xy[c0:c1].min(axis=0), col.xy[c0:c1].max(axis=0)
                pts[i] = (lo + hi) / 2 + rng.uniform(-0.75, 0.75, 2) * (hi - lo)
        out[name] = (col, pts)
    return out


# ---- the kernel's formulas in f64 (Python floats round exactly like the device code: no fused operations) -------------------------


def mirror_segment_dist2(px, py, sx, sy, ex, ey):
    dx, dy, qx, qy = ex - sx, ey - sy, px - sx, py - sy
    d2 = dx * dx + dy * dy
    dot = qx * dx + qy * dy
    cross = qx * dy - qy * dx
    if d2 == 0.0 or dot <= 0.0:
        return qx * qx + qy * qy, 1.0
    if dot >= d2:
        rx, ry = px - ex, py - ey
        return rx * rx + ry * ry, 1.0
    return cross * cross, d2


def mirror_closest(p, kind: int, row):
    """(q, local seg, measure before + along, total length) by the formulas of gpk_linref.h in sequential order (G = 1); None for
    an empty row.  The polygon position is taken from the exact reference (the kernel's position test is exact)."""
    segs = segments(kind, row)
    if X.row_is_empty(kind, row) or not segs:
        return None
    px, py = float(p[0]), float(p[1])
    if kind in X.POLYGONAL and X.geom_position(p, [g for g in X.row_polys(kind, row) if len(g) and len(g[0])]) >= 0:
        return (px, py), -1, None, None
    best, arg = (float("inf"), 1.0), None
    for sg in segs:
        n, d = mirror_segment_dist2(px, py, sg[2][0], sg[2][1], sg[3][0], sg[3][1])
        if n * best[1] < best[0] * d:
            best, arg = (n, d), sg
    i0, i1, s, e = arg
    dx, dy, qx, qy = e[0] - s[0], e[1] - s[1], px - s[0], py - s[1]
    d2 = dx * dx + dy * dy
    dot = qx * dx + qy * dy
    if d2 == 0.0 or dot <= 0.0:
        q, along = s, 0.0
    elif dot >= d2:
        q, along = e, float(np.sqrt(d2))
    else:
        t = dot / d2
        q, along = (s[0] + t * dx, s[1] + t * dy), t * float(np.sqrt(d2))
    before = total = 0.0
    for j0, j1, a, b in segs:
        if j1 != j0:
            l = float(np.sqrt((b[0] - a[0]) * (b[0] - a[0]) + (b[1] - a[1]) * (b[1] - a[1])))
            total += l
            before += l if j0 < i0 else 0.0
    return q, i0, before + along, total
