"""Exact answers and a-priori error bounds for the f64 measures and predicates, at any coordinate magnitude.

Every f64 is an integer times a power of two, so the coordinates of a geometry are integers at a common exponent and every
polynomial of them (twice the signed area of a ring, its centroid moments, an orientation, a squared point-segment distance)
is an exact Python integer.  Square roots (lengths, distances) are taken with `decimal` at 50 digits.

The bounds are forward-error bounds of geo 0.27's f64 formulas (the ones the oracle and the HIP kernels restate), computed
from the input; u = 2^-53 is the unit roundoff and gamma(k) = k u / (1 - k u).  They hold whatever the order of the sums
(a tree or a chunked sum is no worse than the left-to-right one bounded here), with or without FMA contraction.

The mutants restate geo's shifted sums with the wrong shift (0, or the previous ring's first coordinate).  In exact arithmetic
the shift cancels, so a kernel that drops or borrows it stays within 1e-9 of the oracle near the origin; the mutants exist only
to show that the bounds below separate the correct shift from a wrong one on every fixture of this module.

Fixtures place metre-scale features where projected data lives: UTM (x ~ 5e5, y ~ 5e6) and Web Mercator (|x|, |y| up to 2e7),
with consecutive rows alternating between placements far apart."""
from __future__ import annotations

import decimal
from fractions import Fraction

import numpy as np

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray

U = 2.0**-53
_DEC = decimal.Context(prec=50)


def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


# ---- exact integers ------------------------------------------------------------------------------------------------------------


def to_ints(values):
    """floats -> (python ints m_i, D) with value_i == m_i / D exactly; D is the largest power-of-two denominator among them"""
    ratios = [float(v).as_integer_ratio() for v in values]
    D = max((d for _, d in ratios), default=1)
    return [n * (D // d) for n, d in ratios], D


def ring_ints(xy):
    m, D = to_ints(np.asarray(xy, dtype=np.float64).ravel().tolist())
    return m[0::2], m[1::2], D


def is_closed(xy) -> bool:
    return len(xy) >= 3 and xy[0][0] == xy[-1][0] and xy[0][1] == xy[-1][1]


def ring_area2(xy) -> Fraction:
    """exact twice-signed area by geo's rule (area.rs twice_signed_ring_area): < 3 coordinates or open -> 0"""
    xy = np.asarray(xy, dtype=np.float64)
    if not is_closed(xy):
        return Fraction(0)
    X, Y, D = ring_ints(xy)
    s = 0
    for i in range(len(X) - 1):
        s += X[i] * Y[i + 1] - X[i + 1] * Y[i]
    return Fraction(s, D * D)


def ring_moments(xy):
    """exact (A2, Mx, My) of a closed ring: A2 twice the signed area, M = sum (p_i + p_i+1) * cross_i (= 6 * first moment)"""
    X, Y, D = ring_ints(xy)
    a = mx = my = 0
    for i in range(len(X) - 1):
        c = X[i] * Y[i + 1] - X[i + 1] * Y[i]
        a += c
        mx += (X[i] + X[i + 1]) * c
        my += (Y[i] + Y[i + 1]) * c
    return Fraction(a, D * D), Fraction(mx, D**3), Fraction(my, D**3)


def polygon_signed_area(rings) -> Fraction:
    """geo's polygon rule: sign(ext) * (|ext| - sum |holes|) / 2"""
    if not rings:
        return Fraction(0)
    e = ring_area2(rings[0]) / 2
    v = abs(e) - sum((abs(ring_area2(h)) / 2 for h in rings[1:]), Fraction(0))
    return -v if e < 0 else v


def geom_area(polys, signed=False) -> Fraction:
    return sum((polygon_signed_area(p) if signed else abs(polygon_signed_area(p)) for p in polys), Fraction(0))


def exact_centroid(polys):
    """exact area-weighted centroid of a (multi)polygon whose every polygon has a non-zero exterior (geo's dimension-2 case):
    sum over rings of sign(ext or hole) * M / (3 * sum of +-|A2|).  None when the total weight is 0."""
    w = Fraction(0)
    mx = Fraction(0)
    my = Fraction(0)
    for rings in polys:
        for k, r in enumerate(rings):
            if not is_closed(np.asarray(r)):
                continue
            a2, x, y = ring_moments(r)
            if a2 == 0:
                continue
            sgn = (1 if a2 > 0 else -1) * (1 if k == 0 else -1)
            w += abs(a2) * (1 if k == 0 else -1)
            mx += sgn * x
            my += sgn * y
    if w == 0:
        return None
    return mx / (3 * w), my / (3 * w)


def dec_sqrt(q: Fraction) -> decimal.Decimal:
    return _DEC.sqrt(_DEC.divide(decimal.Decimal(q.numerator), decimal.Decimal(q.denominator)))


def segment_length(a, b) -> decimal.Decimal:
    (ax, ay), (bx, by) = [Fraction(float(v)) for v in a], [Fraction(float(v)) for v in b]
    return dec_sqrt((bx - ax) ** 2 + (by - ay) ** 2)


def exact_length(seqs) -> decimal.Decimal:
    """sum of the segment lengths of every coordinate sequence, 50 digits"""
    t = decimal.Decimal(0)
    for s in seqs:
        for i in range(len(s) - 1):
            t = _DEC.add(t, segment_length(s[i], s[i + 1]))
    return t


def linestring_centroid_exact(xy):
    """length-weighted centroid of a linestring (geo's dimension-1 case), 50 digits; None for zero total length"""
    tot = decimal.Decimal(0)
    cx = decimal.Decimal(0)
    cy = decimal.Decimal(0)
    for i in range(len(xy) - 1):
        L = segment_length(xy[i], xy[i + 1])
        mx = (decimal.Decimal(float(xy[i][0])) + decimal.Decimal(float(xy[i + 1][0]))) / 2
        my = (decimal.Decimal(float(xy[i][1])) + decimal.Decimal(float(xy[i + 1][1]))) / 2
        tot, cx, cy = _DEC.add(tot, L), _DEC.add(cx, _DEC.multiply(mx, L)), _DEC.add(cy, _DEC.multiply(my, L))
    if tot == 0:
        return None
    return _DEC.divide(cx, tot), _DEC.divide(cy, tot)


def orient(a, b, c) -> int:
    """exact sign of the orientation of (a, b, c): +1 counter-clockwise, -1 clockwise, 0 collinear (an f64 estimate decides
    when it is farther from 0 than its error can be, exact rationals otherwise)"""
    l = (float(b[0]) - float(a[0])) * (float(c[1]) - float(a[1]))
    r = (float(b[1]) - float(a[1])) * (float(c[0]) - float(a[0]))
    if np.isfinite(l) and np.isfinite(r) and abs(l - r) > 1e-14 * (abs(l) + abs(r)) and abs(l - r) > 1e-280:
        return 1 if l > r else -1
    (ax, ay), (bx, by), (cx, cy) = [[Fraction(float(v)) for v in p] for p in (a, b, c)]
    d = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    return (d > 0) - (d < 0)


def on_segment(p, a, b) -> bool:
    if orient(a, b, p) != 0:
        return False
    return min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def ring_position(p, ring) -> int:
    """+1 inside, 0 on the boundary, -1 outside, by an exact winding number"""
    w = 0
    for i in range(len(ring) - 1):
        a, b = ring[i], ring[i + 1]
        if on_segment(p, a, b):
            return 0
        if a[1] <= p[1]:
            if b[1] > p[1] and orient(a, b, p) > 0:
                w += 1
        elif b[1] <= p[1] and orient(a, b, p) < 0:
            w -= 1
    return 1 if w != 0 else -1


def polygon_position(p, rings) -> int:
    """+1 interior, 0 boundary, -1 exterior of a polygon with holes"""
    pe = ring_position(p, rings[0])
    if pe <= 0:
        return pe
    for h in rings[1:]:
        ph = ring_position(p, h)
        if ph == 0:
            return 0
        if ph > 0:
            return -1
    return 1


def geom_position(p, polys) -> int:
    best = -1
    for rings in polys:
        best = max(best, polygon_position(p, rings))
    return best


def point_segment_dist2(p, a, b) -> Fraction:
    """exact squared distance from p to the closed segment ab"""
    (px, py), (ax, ay), (bx, by) = [[Fraction(float(v)) for v in q] for q in (p, a, b)]
    dx, dy = bx - ax, by - ay
    d2 = dx * dx + dy * dy
    if d2 == 0:
        return (px - ax) ** 2 + (py - ay) ** 2
    t = (px - ax) * dx + (py - ay) * dy
    if t <= 0:
        return (px - ax) ** 2 + (py - ay) ** 2
    if t >= d2:
        return (px - bx) ** 2 + (py - by) ** 2
    c = (px - ax) * dy - (py - ay) * dx
    return c * c / d2


def _f64_seg_dist(p, a, b):
    d = b - a
    d2 = np.sum(d * d, axis=1)
    t = np.clip(np.sum((p - a) * d, axis=1) / np.where(d2 > 0, d2, 1.0), 0.0, 1.0)
    q = a + t[:, None] * d - p
    return np.hypot(q[:, 0], q[:, 1])


def point_seqs_dist2(p, seqs):
    """exact squared distance from p to the nearest segment of the sequences, and the length of the longest segment (f64).
    Segments whose f64 distance is clearly farther than the nearest one's are not evaluated exactly."""
    segs = [(np.asarray(s[:-1], dtype=np.float64), np.asarray(s[1:], dtype=np.float64)) for s in seqs if len(s) >= 2]
    a = np.concatenate([s[0] for s in segs])
    b = np.concatenate([s[1] for s in segs])
    pf = np.asarray(p, dtype=np.float64)
    df = _f64_seg_dist(pf, a, b)
    lmax = float(np.max(np.hypot(*(b - a).T)))
    cut = np.min(df) * (1 + 1e-9) + 1e-9 * (lmax + np.max(np.abs(pf)) * 1e-6)
    best = None
    for i in np.nonzero(df <= cut)[0]:
        d = point_segment_dist2(p, a[i], b[i])
        best = d if best is None or d < best else best
    return best, lmax


def distance_bound(d: float, lmax: float) -> float:
    """a-priori error of geo's line_segment_distance at a point at distance d from a sequence whose longest segment is lmax.
    Differences of nearby coordinates are exact (Sterbenz), the cross product (s - p) x (e - s) loses at most 2u of
    |s - p| |e - s| <= (d + lmax) lmax, the division by |e - s|^2 and the hypot add a few u relative: the absolute error is at
    most 16 u (d + 2 lmax) — relative to the feature's extent, not to its coordinates."""
    return 16 * U * (d + 2 * lmax)


# ---- a-priori bounds of geo's shifted f64 sums ---------------------------------------------------------------------------------


def _shifted(xy):
    xy = np.asarray(xy, dtype=np.float64)
    return xy[:, 0] - xy[0, 0], xy[:, 1] - xy[0, 1]


def ring_area2_bound(xy) -> float:
    """|fl(twice_signed_ring_area) - A2| <= gamma(4) * sum_i (|sx_i ey_i| + |ex_i sy_i|) + gamma(n) * sum_i |t_i| over the
    SHIFTED coordinates, t_i = sx_i ey_i - sy_i ex_i: each term carries the rounding of the shift of its two coordinates, of
    its two products and of their difference (4 u of the products' magnitudes); the sum of the n computed terms, in any order,
    adds at most gamma(n - 1) of the sum of their magnitudes.  This is the issue's (n + 4) eps sum (|sx ey| + |ex sy|) with the
    summation part taken over the terms (which cancel pairwise along the ring) instead of the products; the sums are computed
    in f64 from the shifted coordinates, hence the 1.01."""
    xy = np.asarray(xy, dtype=np.float64)
    if not is_closed(xy):
        return 0.0
    sx, sy = _shifted(xy)
    p = np.abs(sx[:-1] * sy[1:]) + np.abs(sx[1:] * sy[:-1])
    t = np.abs(sx[:-1] * sy[1:] - sy[:-1] * sx[1:])
    sp = float(np.sum(p))
    return 1.01 * (gamma(4) * sp + gamma(len(xy)) * (float(np.sum(t)) + gamma(4) * sp))


def area_bound(polys) -> float:
    """polygon = |ext|/2 - sum |hole|/2, multipolygon = sum of polygons: the ring bounds halved plus one rounding per
    subtraction / addition on the running value, bounded by gamma(rings + polygons) * sum |ring area|"""
    b = 0.0
    tot = 0.0
    k = 0
    for rings in polys:
        for r in rings:
            b += ring_area2_bound(r) / 2
            tot += abs(float(ring_area2(r))) / 2 + ring_area2_bound(r)
            k += 1
        k += 1
    return 1.01 * (b + gamma(k + 1) * tot)


def ring_moment_bounds(xy):
    """error bounds of the two moment sums acc = sum (e + s) t_i of centroid.rs add_ring over the shifted coordinates: a term
    carries gamma(4) of the products in t_i (as in ring_area2_bound) times |e + s|, plus gamma(3) of |(e + s) t_i| (the shift
    and the addition of e + s, the product); the sum of n terms adds gamma(n - 1) of the terms' magnitudes"""
    sx, sy = _shifted(xy)
    p = np.abs(sx[:-1] * sy[1:]) + np.abs(sx[1:] * sy[:-1])
    t = np.abs(sx[:-1] * sy[1:] - sy[:-1] * sx[1:]) + gamma(4) * p
    out = []
    for s in (sx, sy):
        m = np.abs(s[:-1] + s[1:]) * (1 + gamma(2))
        out.append(1.01 * (gamma(4) * float(np.sum(m * p)) + gamma(len(xy) + 3) * float(np.sum(m * t))))
    return out


def centroid_bound(polys, c):
    """a-priori error of geo's area-weighted centroid (centroid.rs) of a (multi)polygon with exact centroid c = (cx, cy).

    Per ring r (area A_r = A2_r / 2 > 0 in magnitude, shift s_r, moment sum acc_r): the ring centroid s_r + acc_r / (6 A_r)
    carries  e_r <= dacc_r / |3 A2_r| + |acc_r / (3 A2_r)| (dA2_r / |A2_r| + 3u) + u |c_r|
    (moment error from ring_moment_bounds, the relative error of the area in the quotient, the division and the final add of the shift).
    The geometry's sums w = sum +-|A_r|, ax = sum +-c_r |A_r| then cancel the exterior against its holes: with W = sum |A_r|
    (no signs),  |err| <= (sum |A_r| e_r + sum |c_r - c| dA_r + gamma(2 k + 2) (sum |c_r| |A_r| + |c| W)) / |w|  + u |c|,
    where the |c_r - c| dA_r term is how an error in a weight moves the mean and the gamma term the roundings of the products
    and sums.  Only the last two terms carry the coordinate's magnitude and they are a few ulps of c: everything else scales
    with the feature's extent and is amplified by W / |w| when the holes nearly cover the exterior."""
    out = []
    for axis in (0, 1):
        cc = abs(float(c[axis]))
        num = 0.0
        W = 0.0
        w = 0.0
        big = 0.0
        k = 0
        for rings in polys:
            for j, r in enumerate(rings):
                r = np.asarray(r, dtype=np.float64)
                a2 = float(ring_area2(r))
                if a2 == 0.0:
                    continue
                k += 1
                b_a2 = ring_area2_bound(r)
                b_acc = ring_moment_bounds(r)[axis]
                A2, Mx, My = ring_moments(r)
                cr_off = float((Mx if axis == 0 else My) / (3 * A2)) - float(r[0, axis])
                cr = abs(float(r[0, axis]) + cr_off)
                e_r = b_acc / abs(3 * a2) + abs(cr_off) * (b_a2 / abs(a2) + 3 * U) + U * cr
                Ar = abs(a2) / 2
                num += Ar * e_r + abs(cr - cc) * b_a2 / 2 + 0.0
                W += Ar
                w += Ar if j == 0 else -Ar
                big += cr * Ar
        w = abs(w) - sum(ring_area2_bound(r) / 2 for rings in polys for r in rings)
        out.append(1.01 * ((num + gamma(2 * k + 2) * (big + cc * W)) / max(w, 1e-300) + U * cc))
    return out


def length_bound(seqs, exact_len: float) -> float:
    """sum of hypot(dx, dy): each difference 1 u, hypot 2 u, the sum n u relative to the total (all terms are positive)"""
    n = sum(len(s) for s in seqs)
    return 1.01 * gamma(n + 4) * exact_len


# ---- mutants: geo's shifted sums with the wrong shift (only used to show the bounds are sharp) ---------------------------------


def mutant_ring_area2(xy, shift) -> float:
    xy = np.asarray(xy, dtype=np.float64)
    if not is_closed(xy):
        return 0.0
    sx, sy = xy[:, 0] - shift[0], xy[:, 1] - shift[1]
    t = 0.0
    for v in sx[:-1] * sy[1:] - sy[:-1] * sx[1:]:
        t += v
    return t


def mutant_ring_centroid(xy, shift):
    """(c, |A|) of one ring by centroid.rs with the given shift; None for a zero (computed) area"""
    xy = np.asarray(xy, dtype=np.float64)
    a = mutant_ring_area2(xy, shift) / 2.0
    if a == 0.0:
        return None
    sx, sy = xy[:, 0] - shift[0], xy[:, 1] - shift[1]
    tmp = sx[:-1] * sy[1:] - sy[:-1] * sx[1:]
    accx = float(np.sum((sx[1:] + sx[:-1]) * tmp))
    accy = float(np.sum((sy[1:] + sy[:-1]) * tmp))
    return (accx / (6.0 * a) + shift[0], accy / (6.0 * a) + shift[1]), abs(a)


def shifts(geoms, kind):
    """the shift each ring of `geoms` (a list of lists of polygons) gets: 'zero', or 'prev' (the previous ring's first
    coordinate, cyclically: the column's first ring borrows the last ring's)"""
    rings = [r for g in geoms for p in g for r in p]
    if kind == "zero":
        return [(0.0, 0.0)] * len(rings)
    firsts = [(float(r[0][0]), float(r[0][1])) if len(r) else (0.0, 0.0) for r in rings]
    return [firsts[i - 1] for i in range(len(rings))]


def mutant_areas(geoms, kind, signed=False):
    sh = iter(shifts(geoms, kind))
    out = []
    for g in geoms:
        v = 0.0
        for rings in g:
            s = [next(sh) for _ in rings]
            if not rings:
                continue
            e = mutant_ring_area2(rings[0], s[0]) / 2.0
            a = abs(e)
            for r, t in zip(rings[1:], s[1:]):
                a -= abs(mutant_ring_area2(r, t) / 2.0)
            pa = -a if e < 0 else a
            v += pa if signed else abs(pa)
        out.append(v)
    return np.array(out)


def mutant_centroids(geoms, kind):
    sh = iter(shifts(geoms, kind))
    out = []
    for g in geoms:
        w = ax = ay = 0.0
        for rings in g:
            for j, r in enumerate(rings):
                m = mutant_ring_centroid(r, next(sh))
                if m is None:
                    continue
                (cx, cy), a = m
                sgn = 1.0 if j == 0 else -1.0
                w += sgn * a
                ax += sgn * cx * a
                ay += sgn * cy * a
        out.append((ax / w, ay / w) if w != 0 else (np.nan, np.nan))
    return np.array(out)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------

# where projected data lives: UTM zones (easting ~ 1.6e5 .. 8.4e5, northing up to 9.3e6) and Web Mercator (|x|, |y| < 2.0037e7)
PLACEMENTS = [
    (512345.678, 5412345.25),
    (-19998765.4321, 19987654.125),
    (166021.0, 9329005.5),
    (19991234.75, -19993456.0625),
    (-12345678.9, -19876543.21),
    (834000.5, 3456789.125),
]


def _star(rng, cx, cy, size, n, cw=False):
    """closed simple ring of n distinct vertices (n + 1 coordinates) of diameter ~ size around (cx, cy); not dyadic"""
    t = np.sort(rng.uniform(0, 2 * np.pi, n)) if n > 8 else 2 * np.pi * (np.arange(n) + rng.uniform(0, 0.5, n)) / n
    r = 0.5 * size * rng.uniform(0.6, 1.0, n)
    if cw:
        t = -t
    xy = np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], axis=1)
    return np.concatenate([xy, xy[:1]])


def _place(rng, i, jitter=1000.0):
    px, py = PLACEMENTS[i % len(PLACEMENTS)]
    return px + rng.uniform(-jitter, jitter), py + rng.uniform(-jitter, jitter)


def buildings(n=600, seed=1, holes=True, multi=True):
    """geometries (list of multipolygons: polygons of rings of (x, y)) of 0.5 - 50 m with 4 - 64 vertices, consecutive rows on
    alternating placements; some with 1 - 2 holes, some of 2 - 3 polygons"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        cx, cy = _place(rng, i)
        size = float(np.exp(rng.uniform(np.log(0.5), np.log(50.0))))
        polys = []
        for p in range(int(rng.integers(2, 4)) if multi and rng.random() < 0.3 else 1):
            ox, oy = cx + 3 * size * p, cy + 1.5 * size * p
            ring = _star(rng, ox, oy, size, int(rng.integers(4, 65)))
            rings = [ring]
            if holes and rng.random() < 0.35:
                for h in range(int(rng.integers(1, 3))):
                    hs = 0.15 * size
                    rings.append(_star(rng, ox + (h - 0.5) * 0.3 * size * 0.5, oy, hs, int(rng.integers(4, 12)), cw=True))
            polys.append(rings)
        out.append(polys)
    return out


def ring_lengths(seed=2):
    """one polygon per coordinate count at every size-class and chunk boundary of the two-stage form (2-, 8-, 16-lane classes
    up to 16 / 128 / 512 coordinates, whole-work-group rings, 8192-coordinate chunks) and beyond a 5e4 ring, alternating
    placements, radii 5 - 50 m.  (A closed ring of 3 coordinates has area 0 whatever the shift: it is in the strip fixtures.)"""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate((4, 5, 16, 17, 18, 128, 129, 511, 512, 513, 514, 8191, 8192, 8193, 3 * 8192 + 5, 50001)):
        cx, cy = _place(rng, i)
        out.append([[_star(rng, cx, cy, float(rng.uniform(10, 100)), n - 1)]])
    return out


def coastline(n=20000, seed=3):
    """long ragged rings: 300 m with a long hole at a UTM placement, 3 km at Web Mercator.  (A UTM coastline of many km loses
    less than the a-priori bound without its shift — the sum's rounding grows with n, the mutant's as sqrt(n) — so it could
    not tell a dropped shift from a correct one.)"""
    rng = np.random.default_rng(seed)

    def ragged(cx, cy, R, m, cw=False):
        t = 2 * np.pi * np.arange(m) / m
        r = R * (1 + 0.05 * np.cumsum(rng.normal(0, 0.02, m)).clip(-5, 5) + 0.1 * np.sin(13 * t))
        if cw:
            t = -t
        xy = np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], axis=1)
        return np.concatenate([xy, xy[:1]])

    return [[[ragged(512345.5, 5412345.5, 300.0, n), ragged(512345.5, 5412345.5, 80.0, n // 4, cw=True)]],
            [[ragged(-19990000.25, 19980000.5, 3000.0, n // 2)]]]


def small_rings(n=1500, seed=4):
    """rings of 4 - 16 coordinates (odd and even counts), one a row: rings straddle every 512-coordinate window of the staged
    class-0 kernel and every 1024-coordinate strip of the one-pass form"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        cx, cy = _place(rng, i)
        out.append([[_star(rng, cx, cy, float(rng.uniform(0.5, 20.0)), int(rng.integers(3, 16)))]])
    return out


def strip_column(seed=5):
    """(geoms, validity): a column of exactly 2 * 1024 coordinates whose rings are cut by the strip boundary, a geometry of
    several rings crossing it, an empty geometry whose coordinate offset is exactly the strip base 1024, 3-coordinate rings,
    and a tail of empty and null rows"""
    rng = np.random.default_rng(seed)
    geoms = []
    used = 0
    i = 0
    while used < 1024 - 40:  # rings of 11 and 7 coordinates up to a few short of the strip
        n = 11 if i % 2 else 7
        geoms.append([[_star(rng, *_place(rng, i), 5.0, n - 1)]])
        used += n
        i += 1
    rest = 1024 - used
    # pad to exactly 1024 with one ring (>= 4 coordinates) and a degenerate 3-coordinate ring
    a = _star(rng, *_place(rng, i), 3.0, rest - 3 - 1)
    b = _star(rng, *_place(rng, i + 1), 3.0, 2)[[0, 1, 0]]
    geoms.append([[a], [b]])
    geoms.append([])  # empty geometry at coordinate offset 1024
    # a multipolygon crossing nothing, then one of many rings: the second strip is filled to exactly 2048
    many = [[_star(rng, *_place(rng, 1), 8.0, 40)]]
    for k in range(6):
        many.append([_star(rng, PLACEMENTS[1][0] + 30 * k, PLACEMENTS[1][1], 6.0, 60), _star(rng, PLACEMENTS[1][0] + 30 * k, PLACEMENTS[1][1], 1.0, 9, cw=True)])
    geoms.append(many)
    used = sum(len(r) for g in geoms for p in g for r in p)
    while 2048 - used > 600:
        g = [[_star(rng, *_place(rng, len(geoms)), 40.0, 500)]]
        geoms.append(g)
        used += 501
    last = 2048 - used
    geoms.append([[_star(rng, *_place(rng, 3), 12.0, last - 1)]])
    assert sum(len(r) for g in geoms for p in g for r in p) == 2048
    valid = [True] * len(geoms) + [True, False, True, False]
    geoms += [[], [], [], []]  # empty and null rows after the last coordinate
    return geoms, valid


def to_array(geoms, validity=None) -> GeoArrowArray:
    """a MULTIPOLYGON column (rings taken as they are: closed by the generators)"""
    a = GeoArrowArray.from_multipolygons([[[np.asarray(r).tolist() for r in p] for p in g] for g in geoms], close=False)
    if validity is not None:
        a = GeoArrowArray(a.geom_type, a.xy, geom_offsets=a.geom_offsets, part_offsets=a.part_offsets, ring_offsets=a.ring_offsets,
                          validity=np.packbits(np.asarray(validity, dtype=bool), bitorder="little"))
    return a


def to_polygon_array(geoms) -> GeoArrowArray:
    """a POLYGON column of the first polygon of each geometry (an empty polygon for an empty geometry)"""
    return GeoArrowArray.from_polygons([[np.asarray(r).tolist() for r in g[0]] if g else [] for g in geoms], close=False)


def area_fixtures():
    """name -> geoms, validity (None: all valid); the fixtures the area / centroid bounds and mutants are held on"""
    sc, sv = strip_column()
    return {
        "buildings": (buildings(), None),
        "ring_lengths": (ring_lengths(), None),
        "coastline": (coastline(), None),
        "small_rings": (small_rings(), None),
        "strip_column": (sc, sv),
    }


# ---- per-geometry exact answers ------------------------------------------------------------------------------------------------


def exact_areas(geoms, validity=None, signed=False):
    """(exact Fractions or None for null rows, bounds)"""
    ex, bd = [], []
    for i, g in enumerate(geoms):
        if validity is not None and not validity[i]:
            ex.append(None)
            bd.append(0.0)
            continue
        ex.append(geom_area(g, signed))
        bd.append(area_bound(g))
    return ex, bd


def abs_err(got: float, exact) -> float:
    """|got - exact| rounded once (exact: Fraction or Decimal); a non-finite `got` is infinitely wrong"""
    if not np.isfinite(got):
        return float("inf")
    if isinstance(exact, decimal.Decimal):
        return float(abs(_DEC.subtract(decimal.Decimal(got), exact)))
    return float(abs(Fraction(got) - exact))


def scaled(a: GeoArrowArray, k: int, t=(0.0, 0.0)) -> GeoArrowArray:
    """the column with every coordinate times 2^k plus t (exact by construction of the callers: they check it)"""
    xy = np.ldexp(a.xy, k) + np.asarray(t, dtype=np.float64)
    return GeoArrowArray(a.geom_type, xy, geom_offsets=a.geom_offsets, part_offsets=a.part_offsets, ring_offsets=a.ring_offsets,
                         validity=a.validity)


def translated_exactly(a: GeoArrowArray, t) -> GeoArrowArray:
    b = scaled(a, 0, t)
    assert np.array_equal(b.xy - np.asarray(t, dtype=np.float64), a.xy), "translation is not exact"
    return b


# offsets at which the lattice goldens stay exact: powers of two and sums of a few
LATTICE_OFFSETS = [(2.0**30, 2.0**30), (-(2.0**33) + 2.0**20, 5 * 2.0**20), (5 * 2.0**20, -(2.0**33) + 2.0**20), (-(2.0**24), 2.0**44)]


def polygon_geoms(a: GeoArrowArray):
    """GeoArrowArray (POLYGON / MULTIPOLYGON) -> list of geometries, each a list of polygons of ring coordinate arrays"""
    out = []
    for g in range(a.n_geoms):
        if a.geom_type == _abi.GEOM_POLYGON:
            r0, r1 = a.geom_offsets[g], a.geom_offsets[g + 1]
            polys = [[a.xy[a.ring_offsets[r] : a.ring_offsets[r + 1]] for r in range(r0, r1)]] if r1 > r0 else []
        else:
            polys = []
            for p in range(a.geom_offsets[g], a.geom_offsets[g + 1]):
                polys.append([a.xy[a.ring_offsets[r] : a.ring_offsets[r + 1]] for r in range(a.part_offsets[p], a.part_offsets[p + 1])])
        out.append(polys)
    return out


def dyadic_buildings(n=200, seed=6):
    """rectangles and diamonds with vertices on multiples of 2^-4 at the placements (edge midpoints are exact coordinates: points
    exactly on an edge), some with a dyadic hole"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        px, py = PLACEMENTS[i % len(PLACEMENTS)]
        cx = np.round((px + rng.uniform(-1000, 1000)) * 16) / 16
        cy = np.round((py + rng.uniform(-1000, 1000)) * 16) / 16
        w, h = [float(rng.integers(8, 800)) / 16 for _ in range(2)]
        if i % 2:
            ring = [(cx, cy), (cx + w, cy), (cx + w, cy + h), (cx, cy + h), (cx, cy)]
        else:
            ring = [(cx, cy - h), (cx + w, cy), (cx, cy + h), (cx - w, cy), (cx, cy - h)]
        rings = [np.array(ring)]
        if i % 3 == 0 and w >= 2 and h >= 2:
            q = 0.25
            rings.append(np.array([(cx + q, cy + q), (cx + q, cy + 2 * q), (cx + 2 * q, cy + 2 * q), (cx + 2 * q, cy + q), (cx + q, cy + q)]) - (0 if i % 2 else (q * 3, q * 6)))
        out.append([rings])
    return out


def probe_points(geoms, seed=7):
    """(points, rows): for every geometry, points on a vertex, on an edge's rounded midpoint and 1 - 2 ulps either side of it in
    x and in y, a vertex moved by 1 ulp, and points 1 cm, 1 m and 3 m off the edge along its normal"""
    rng = np.random.default_rng(seed)
    pts, rows = [], []
    for g, polys in enumerate(geoms):
        if not polys:
            continue
        ring = np.asarray(polys[int(rng.integers(0, len(polys)))][0], dtype=np.float64)
        j = int(rng.integers(0, len(ring) - 1))
        a, b = ring[j], ring[j + 1]
        m = (a + b) / 2
        nrm = np.array([b[1] - a[1], a[0] - b[0]])
        nrm = nrm / np.hypot(*nrm)
        cand = [a, m, a + [np.spacing(a[0]), 0.0]]
        for k in (1, 2):
            cand += [np.array([x, m[1]]) for x in (m[0] + k * np.spacing(m[0]), m[0] - k * np.spacing(m[0]))]
            cand += [np.array([m[0], y]) for y in (m[1] + k * np.spacing(m[1]), m[1] - k * np.spacing(m[1]))]
        cand += [m + s * d * nrm for d in (0.01, 1.0, 3.0) for s in (1, -1)]
        pts += cand
        rows += [g] * len(cand)
    return np.array(pts, dtype=np.float64), np.array(rows, dtype=np.uint32)


def exact_distance(p, polys):
    """(Decimal distance, bound) from point p to a (multi)polygon: 0 inside or on the boundary, else to the nearest ring"""
    if not polys or geom_position(p, polys) >= 0:
        return decimal.Decimal(0), 0.0
    d2, lmax = point_seqs_dist2(p, [r for rings in polys for r in rings])
    d = dec_sqrt(d2)
    return d, distance_bound(float(d), lmax)


def exact_hull(points):
    """the convex hull's vertices (collinear points dropped) as a closed counter-clockwise ring, by exact orientations"""
    pts = sorted(set((float(x), float(y)) for x, y in points))
    if len(pts) < 3:
        return np.array(pts + pts[:1])

    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and orient(h[-2], h[-1], p) <= 0:
                h.pop()
            h.append(p)
        return h

    lo, up = half(pts), half(pts[::-1])
    ring = lo[:-1] + up[:-1]
    return np.array(ring + ring[:1])


def near_collinear_sets(n_sets=60, seed=8):
    """point sets along lines at 2e7 with coordinates moved by -2 .. 2 ulps: orientations whose f64 estimate cannot decide"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_sets):
        px, py = PLACEMENTS[i % len(PLACEMENTS)]
        k = int(rng.integers(5, 40))
        t = np.sort(rng.uniform(0, 10.0, k))
        dx, dy = rng.normal(size=2)
        x = px + t * dx
        y = py + t * dy
        x += rng.integers(-2, 3, k) * np.spacing(x)
        y += rng.integers(-2, 3, k) * np.spacing(y)
        if i % 3 == 0:
            x = np.append(x, px + 5 * dx - 1e-6 * dy)  # one point a micrometre off the line
            y = np.append(y, py + 5 * dy + 1e-6 * dx)
        out.append(np.stack([x, y], axis=1))
    return out


def canon(ring):
    """a closed ring without its closing coordinate, rolled to start at its lexicographically smallest vertex"""
    ring = np.asarray(ring)
    ring = ring[:-1] if len(ring) > 1 and np.array_equal(ring[0], ring[-1]) else ring
    if len(ring) == 0:
        return ring
    return np.roll(ring, -np.lexsort((ring[:, 1], ring[:, 0]))[0], axis=0)


# ---- point -> geometry distance for every right family (row-wise distance and the nearest join) ---------------------------------
#
# A column is described on the host as (kind, rows, validity): rows[i] is a POINT (x, y) (None: empty), a MULTIPOINT's list of
# points, a LINESTRING's list of coordinates, a MULTILINESTRING's list of linestrings, a POLYGON's list of closed rings (exterior
# first) or a MULTIPOLYGON's list of polygons.  Null rows keep their coordinates (the index lists them; the kernels must skip them).

POLYGONAL = (_abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON)
FAMILIES = {
    "point": _abi.GEOM_POINT,
    "multipoint": _abi.GEOM_MULTIPOINT,
    "linestring": _abi.GEOM_LINESTRING,
    "multilinestring": _abi.GEOM_MULTILINESTRING,
    "polygon": _abi.GEOM_POLYGON,
    "multipolygon": _abi.GEOM_MULTIPOLYGON,
}
DBL_MAX = float(np.finfo(np.float64).max)
# what geo's distance gives for an empty right row: an empty LINESTRING / POLYGON is at 0, an empty multi-geometry folds its
# (no) parts from f64::MAX; an empty POINT (NaN coordinates) gives NaN
EMPTY_DISTANCE = {_abi.GEOM_POINT: float("nan"), _abi.GEOM_MULTIPOINT: DBL_MAX, _abi.GEOM_LINESTRING: 0.0,
                  _abi.GEOM_MULTILINESTRING: DBL_MAX, _abi.GEOM_POLYGON: 0.0, _abi.GEOM_MULTIPOLYGON: DBL_MAX}


def distance_group_size(kind: int, n_coords: int, n_geoms: int) -> int:
    """lanes per row of gpk_distance_rowwise's per-row kernel and of gpk_nearest_join, restated from gpk_distance.h
    (pick_group_rows / distance_group_size): about 8 segments per lane from the column's mean vertex count (empty and null rows
    count), rounded to the instantiated sizes 1 / 8 / 32 — 1 below a mean of 16, 8 from 16 to 127, 32 from 128 up; POINT: 1"""
    if kind == _abi.GEOM_POINT:
        return 1
    mean = n_coords / n_geoms if n_geoms > 0 else 1.0
    G = 1
    while G < 64 and G * 2 * 8 <= mean:
        G <<= 1
    return 1 if G <= 1 else (8 if G <= 8 else 32)


def group_size_of(a: GeoArrowArray) -> int:
    return distance_group_size(a.geom_type, a.n_coords, a.n_geoms)


def column(kind: int, rows, validity=None) -> GeoArrowArray:
    """(kind, rows, validity) -> GeoArrowArray (rings taken as they are)"""
    bits = None if validity is None else np.packbits(np.asarray(validity, dtype=bool), bitorder="little")
    if kind == _abi.GEOM_POINT:
        xy = np.array([(np.nan, np.nan) if r is None else r for r in rows], dtype=np.float64).reshape(-1, 2)
        return GeoArrowArray(kind, xy, validity=bits)
    if kind in (_abi.GEOM_MULTIPOINT, _abi.GEOM_LINESTRING):
        off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        xy = np.array([c for r in rows for c in r], dtype=np.float64).reshape(-1, 2)
        return GeoArrowArray(kind, xy, geom_offsets=off, validity=bits)
    if kind == _abi.GEOM_MULTILINESTRING:
        goff = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        parts = [p for r in rows for p in r]
        roff = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
        xy = np.array([c for p in parts for c in p], dtype=np.float64).reshape(-1, 2)
        return GeoArrowArray(kind, xy, geom_offsets=goff, ring_offsets=roff, validity=bits)
    if kind == _abi.GEOM_POLYGON:
        a = GeoArrowArray.from_polygons([[np.asarray(r).tolist() for r in g] for g in rows], close=False)
    else:
        a = GeoArrowArray.from_multipolygons([[[np.asarray(r).tolist() for r in p] for p in g] for g in rows], close=False)
    return GeoArrowArray(a.geom_type, a.xy, geom_offsets=a.geom_offsets, part_offsets=a.part_offsets, ring_offsets=a.ring_offsets,
                         validity=bits)


def row_is_empty(kind: int, row) -> bool:
    return row is None if kind == _abi.GEOM_POINT else len(row) == 0


def row_polys(kind: int, row):
    """a polygonal row as a list of polygons"""
    return [row] if kind == _abi.GEOM_POLYGON else row


def row_seqs(kind: int, row):
    """the coordinate sequences whose segments a row's distance is taken over (points: one point per sequence)"""
    if kind == _abi.GEOM_POINT:
        return [] if row is None else [[row]]
    if kind == _abi.GEOM_MULTIPOINT:
        return [[q] for q in row]
    if kind == _abi.GEOM_LINESTRING:
        return [row] if len(row) else []
    if kind == _abi.GEOM_MULTILINESTRING:
        return list(row)
    return [r for p in row_polys(kind, row) for r in p]


def row_lmax(kind: int, row) -> float:
    """longest segment of the row (0 for points)"""
    m = 0.0
    for s in row_seqs(kind, row):
        s = np.asarray(s, dtype=np.float64)
        if len(s) >= 2:
            m = max(m, float(np.max(np.hypot(*(s[1:] - s[:-1]).T))))
    return m


def exact_row_distance2(p, kind: int, row):
    """exact squared distance (Fraction) from point p to a non-empty row, and the row's longest segment; None for an empty row.
    Polygonal: 0 when p is not outside, else the minimum over every ring of every part.  Only near-minimal segments and points
    (by the f64 pre-filter of point_seqs_dist2) are evaluated exactly."""
    if row_is_empty(kind, row):
        return None, 0.0
    if kind in (_abi.GEOM_POINT, _abi.GEOM_MULTIPOINT):
        q = np.asarray([row] if kind == _abi.GEOM_POINT else row, dtype=np.float64)
        pf = np.asarray(p, dtype=np.float64)
        df = np.hypot(q[:, 0] - pf[0], q[:, 1] - pf[1])
        cut = np.min(df) * (1 + 1e-9) + 1e-9 * np.max(np.abs(pf)) * 1e-6
        px, py = Fraction(float(p[0])), Fraction(float(p[1]))
        return min((px - Fraction(float(q[i, 0]))) ** 2 + (py - Fraction(float(q[i, 1]))) ** 2 for i in np.nonzero(df <= cut)[0]), 0.0
    if kind in POLYGONAL and geom_position(p, row_polys(kind, row)) >= 0:
        return Fraction(0), row_lmax(kind, row)
    return point_seqs_dist2(p, row_seqs(kind, row))


def exact_row_distance(p, kind: int, row):
    """(Decimal distance or None for an empty row, distance_bound of the f64 evaluation)"""
    d2, lmax = exact_row_distance2(p, kind, row)
    if d2 is None:
        return None, 0.0
    d = dec_sqrt(d2)
    return d, distance_bound(float(d), lmax)


def f64_distance_matrix(P, kind: int, rows, usable=None, chunk_elems: int = 1 << 22) -> np.ndarray:
    """(n_points, n_rows) f64 estimate of every point -> row distance, vectorised: the nearest segment (or point) of the row, 0
    inside a polygonal row by an even-odd crossing count over all its rings; inf for empty rows and rows not `usable`.  A filter
    only: near a boundary the crossing count may be wrong, but there the boundary distance is near 0 anyway."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    nr = len(rows)
    A, B, owner, part = [], [], [], []
    n_parts = 0
    for j, row in enumerate(rows):
        if (usable is not None and not usable[j]) or row_is_empty(kind, row):
            continue
        polys = row_polys(kind, row) if kind in POLYGONAL else [row_seqs(kind, row)]
        for rings in polys:  # (the crossing count is taken per polygon: the parts of a multipolygon may overlap)
            n_parts += 1
            for s in rings:
                s = np.asarray(s, dtype=np.float64).reshape(-1, 2)
                a, b = (s, s) if len(s) == 1 else (s[:-1], s[1:])
                A.append(a)
                B.append(b)
                owner.append(np.full(len(a), j))
                part.append(np.full(len(a), n_parts))
    out = np.full((len(P), nr), np.inf)
    if not A:
        return out
    A, B, owner, part = np.concatenate(A), np.concatenate(B), np.concatenate(owner), np.concatenate(part)
    starts = np.flatnonzero(np.concatenate([[True], owner[1:] != owner[:-1]]))
    pstarts = np.flatnonzero(np.concatenate([[True], part[1:] != part[:-1]]))
    ids = owner[starts]
    D = B - A
    d2 = np.sum(D * D, axis=1)
    step = max(1, chunk_elems // len(A))
    for c in range(0, len(P), step):
        px, py = P[c : c + step, 0:1], P[c : c + step, 1:2]
        qx, qy = px - A[:, 0], py - A[:, 1]
        t = np.clip((qx * D[:, 0] + qy * D[:, 1]) / np.where(d2 > 0, d2, 1.0), 0.0, 1.0)
        seg = np.hypot(qx - t * D[:, 0], qy - t * D[:, 1])
        best = np.minimum.reduceat(seg, starts, axis=1)
        if kind in POLYGONAL:
            with np.errstate(divide="ignore", invalid="ignore"):
                xc = A[:, 0] + (py - A[:, 1]) * D[:, 0] / D[:, 1]
            cross = ((A[:, 1] > py) != (B[:, 1] > py)) & (px < xc)
            inside_part = np.add.reduceat(cross.astype(np.int32), pstarts, axis=1) % 2 == 1
            inside = np.zeros(best.shape, dtype=bool)
            np.logical_or.at(inside, (slice(None), np.searchsorted(starts, pstarts, side="right") - 1), inside_part)
            best = np.where(inside, 0.0, best)
        out[c : c + step, ids] = best
    return out


def exact_min_distance(p, kind: int, rows, frow, lmax=None):
    """exact minimum distance (Decimal) from p over the rows, given the f64 estimates `frow` of f64_distance_matrix (inf: not a
    candidate), and its bound: the largest distance_bound among the rows the f64 pre-filter kept.  (None, 0) when no row counts.
    lmax: row_lmax of every row (computed when not given)."""
    m = float(np.min(frow))
    if not np.isfinite(m):
        return None, 0.0
    fin = np.flatnonzero(np.isfinite(frow))
    lm = np.asarray(lmax)[fin] if lmax is not None else [row_lmax(kind, rows[j]) for j in fin]
    cut = m * (1 + 1e-9) + 1e-9 * (float(np.max(lm)) + float(np.max(np.abs(p))) * 1e-6)
    best, bound = None, 0.0
    for j in np.flatnonzero(frow <= cut):
        d2, lmax = exact_row_distance2(p, kind, rows[j])
        best = d2 if best is None or d2 < best else best
        bound = max(bound, lmax)
    d = dec_sqrt(best)
    return d, distance_bound(float(d), bound)


# ---- one fixture per (family, G) instance of the distance kernels -------------------------------------------------------------

INSTANCES = [(f, g) for f in FAMILIES for g in ((1,) if f == "point" else (1, 8, 32))]
DOMAIN = 1000.0
# per G: vertices per row (MULTIPOINT: points) well inside the band distance_group_size maps to G
_VERTS = {1: (2, 9), 8: (30, 60), 32: (200, 300)}
_ROWS = {1: 300, 8: 150, 32: 60}


def _walk(rng, cx, cy, size, n):
    xy = np.cumsum(np.concatenate([[[cx, cy]], rng.normal(0, size / np.sqrt(n), (n - 1, 2))]), axis=0)
    return [tuple(c) for c in xy]


def _dyadic_rect(cx, cy, m, s=0.125):
    """closed axis-parallel square with m vertices per side on multiples of s (4 m vertices): every coordinate, and the middle of
    every edge piece, is an exact double"""
    x0, y0 = np.floor(cx / s) * s, np.floor(cy / s) * s
    w = m * s * 8
    side = [x0 + i * w / m for i in range(m)]
    ring = [(x, y0) for x in side] + [(x0 + w, y0 + i * w / m) for i in range(m)]
    ring += [(x0 + w - i * w / m, y0 + w) for i in range(m)] + [(x0, y0 + w - i * w / m) for i in range(m)]
    return ring + ring[:1], (x0 + 0.5 * w / m, y0)


def instance_rows(family: str, G: int, seed: int = 0):
    """(kind, rows, validity, meta) of a right column built for (family, G): rows of a vertex count inside G's band, every
    23rd row empty, every 19th null (its coordinates kept), every 10th an exact copy of an earlier row (exact ties), and — lines
    and polygons — every 7th row dyadic (points exactly on its edges).  Polygons carry holes.  meta[i]: dict of the row's
    centre, size, a point inside a hole (or None) and a point exactly on an edge (or None)."""
    kind = FAMILIES[family]
    rng = np.random.default_rng(1000 * kind + G + seed)
    n = 400 if kind == _abi.GEOM_POINT else _ROWS[G]
    lo, hi = _VERTS[G]
    rows, meta = [], []
    for i in range(n):
        cx, cy = rng.uniform(0.02 * DOMAIN, 0.98 * DOMAIN, 2)
        size = float(rng.uniform(5.0, 30.0))
        hole = edge = None
        k = int(rng.integers(lo, hi + 1))
        dy = i % 7 == 3
        if kind == _abi.GEOM_POINT:
            row = (float(cx), float(cy))
        elif kind == _abi.GEOM_MULTIPOINT:
            row = [tuple(q) for q in rng.normal((cx, cy), size / 3, (max(k, 1), 2))]
        elif kind == _abi.GEOM_LINESTRING:
            if dy:
                x0, y0 = np.floor(cx * 8) / 8, np.floor(cy * 8) / 8
                row = [(x0 + j * 0.5, y0) for j in range(k)]
                edge = (x0 + 0.25, y0)
            else:
                row = _walk(rng, cx, cy, size, k)
        elif kind == _abi.GEOM_MULTILINESTRING:
            parts = int(rng.integers(1, 3)) if G == 1 else int(rng.integers(2, 4))
            kk = max(2, k // parts)
            row = [_walk(rng, cx + 2 * size * p, cy, size, kk) for p in range(parts)]
            if dy:
                x0, y0 = np.floor(cx * 8) / 8, np.floor(cy * 8) / 8
                row[0] = [(x0, y0 + j * 0.5) for j in range(kk)]
                edge = (x0, y0 + 0.25)
        else:
            parts = 1 if kind == _abi.GEOM_POLYGON else (int(rng.integers(1, 3)) if G == 1 else 2)
            kk = max(3, k // parts - (3 if G == 1 else 0))
            row = []
            for p in range(parts):
                ox = cx + 1.5 * size * p
                if dy:
                    ring, e = _dyadic_rect(ox, cy, max(1, kk // 4))
                    edge = edge or e
                    rings = [np.asarray(ring)]
                else:
                    rings = [_star(rng, ox, cy, size, kk)]
                if (G > 1 or i % 3 == 0) and not dy:
                    rings.append(_star(rng, ox, cy, 0.15 * size, 3 if G == 1 else max(4, kk // 8), cw=True))
                    hole = hole or (float(ox), float(cy))
                row.append([np.asarray(r, dtype=np.float64) for r in rings])
            if kind == _abi.GEOM_POLYGON:
                row = row[0]
        if i % 10 == 9 and not row_is_empty(kind, rows[i - 3]):
            row, m = rows[i - 3], dict(meta[i - 3])
        else:
            m = {"center": (float(cx), float(cy)), "size": size, "hole": hole, "edge": edge}
        if i % 23 == 11:
            row = None if kind == _abi.GEOM_POINT else []
            m = dict(m, hole=None, edge=None)
        rows.append(row)
        meta.append(m)
    validity = [i % 19 != 4 for i in range(n)]
    return kind, rows, validity, meta


def _vertices(kind, row):
    return [c for s in row_seqs(kind, row) for c in s]


def _query(rng, kind, row, m, q):
    """one query point for a row: q selects a point in the widened bbox, a vertex, a hole's inside, a vertex moved by one ulp, a
    point exactly on an edge"""
    cx, cy = m["center"]
    s = m["size"]
    if row_is_empty(kind, row) or q in (0, 5):
        return (float(cx + rng.uniform(-s, s)), float(cy + rng.uniform(-s, s)))
    vs = _vertices(kind, row)
    v = vs[int(rng.integers(0, len(vs)))]
    if q == 1:
        return (float(v[0]), float(v[1]))
    if q == 2:
        if m["hole"] is not None:
            return m["hole"]
        a = rng.uniform(0, 2 * np.pi)
        return (float(cx + 3 * s * np.cos(a)), float(cy + 3 * s * np.sin(a)))
    if q == 3:
        return (float(np.nextafter(v[0], np.inf)), float(v[1]))
    return m["edge"] if m["edge"] is not None else (float(v[0]), float(np.nextafter(v[1], -np.inf)))


_CACHE = {}


def instance_fixture(family: str, G: int):
    """dict: kind, rows, validity, meta, array (the right column), queries ((n_rows, 2): query i pairs with row i), left ((300, 2):
    the nearest join's points: uniform over the extent, vertices, vertices moved by one ulp, points inside holes and on edges, near
    duplicated rows); cached per process"""
    key = (family, G)
    if key in _CACHE:
        return _CACHE[key]
    kind, rows, validity, meta = instance_rows(family, G)
    rng = np.random.default_rng(7 + 100 * kind + G)
    queries = np.array([_query(rng, kind, rows[i], meta[i], i % 6) for i in range(len(rows))], dtype=np.float64)
    usable = [validity[i] and not row_is_empty(kind, rows[i]) for i in range(len(rows))]
    good = np.flatnonzero(usable)
    copies = [j for j in range(9, len(rows), 10) if usable[j] and usable[j - 3] and rows[j] is rows[j - 3]]  # rows with an exact twin
    left = [tuple(rng.uniform(-0.05 * DOMAIN, 1.05 * DOMAIN, 2)) for _ in range(140)]
    for t in range(160):
        j = int(good[rng.integers(0, len(good))]) if t % 4 else copies[int(rng.integers(0, len(copies)))]
        left.append(_query(rng, kind, rows[j], meta[j], t % 6))
    fx = {"kind": kind, "rows": rows, "validity": validity, "meta": meta, "array": column(kind, rows, validity),
          "queries": queries, "left": np.array(left, dtype=np.float64), "usable": np.array(usable)}
    _CACHE[key] = fx
    return fx


def exact_rowwise(fx, queries=None, rows_of=None):
    """exact (Decimal or None for empty rows) and bound of distance(queries[i], rows[rows_of[i]]); cached for the fixture's own
    queries"""
    own = queries is None
    if own and "exact_rowwise" in fx:
        return fx["exact_rowwise"]
    queries = fx["queries"] if own else queries
    rows_of = np.arange(len(queries)) if rows_of is None else rows_of
    out = [exact_row_distance(queries[i], fx["kind"], fx["rows"][int(rows_of[i])]) for i in range(len(queries))]
    if own:
        fx["exact_rowwise"] = out
    return out


def exact_nearest_minima(fx, left=None):
    """per left point the exact minimum distance over the usable rows and its bound (None where no row counts)"""
    own = left is None
    if own and "exact_min" in fx:
        return fx["exact_min"]
    left = fx["left"] if own else left
    F = f64_distance_matrix(left, fx["kind"], fx["rows"], fx["usable"])
    lmax = [row_lmax(fx["kind"], r) for r in fx["rows"]]
    out = [exact_min_distance(left[l], fx["kind"], fx["rows"], F[l], lmax) for l in range(len(left))]
    if own:
        fx["exact_min"] = out
    return out
