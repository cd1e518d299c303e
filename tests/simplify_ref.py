"""Exact reference for simplify (gpk_simplify, csrc/gpk_lineal_ops.hip; oracle: gpko_simplify) — test infrastructure.

`rdp_exact` walks geo 0.27's compute_rdp on exact rationals: squared distances compared with eps^2, the LAST index among equals,
a split only when strictly farther than eps, the left part first, `simplified_len` shared by the whole walk, min_pts 2 for
linestring / multilinestring sequences and 4 for polygon / multipolygon rings; fewer than 3 coordinates or eps <= 0: unchanged.
It is iterative (the rings here are longer than Python's recursion limit).  Coordinates are doubles, so every rational is held
as an integer over one power-of-two denominator per sequence.

At every node the project's f64 distance expression (seg_dist / o_seg_dist: plain sqrt, no FMA) is evaluated as well, in plain
Python floats (`seg_dist_f64`; long ranges go through the same operations in numpy, `test_simplify_ref` holds the two together).
A sequence is SETTLED when at every node it visits the float last-argmax equals the rational one and `float_best > eps` equals
`rational_best^2 > eps^2`.  The expected output always comes from the rationals; the floats only say which sequences the exact
reference is entitled to judge (`compare_exact` asserts the unsettled share against a cap BEFORE it compares anything).

The floats also spare work, conservatively: only candidates whose f64 distance is within FILTER * (|p - s| + |e - s|) of the f64
maximum are evaluated exactly.  The f64 expression is off by a few u of those lengths at most (differences of doubles carry a
relative error u, the cross product 4u |p - s| |e - s|, division, sqrt and product a few u more; where r is within rounding of
0 or 1 the two branches differ by |r_err| |e - s| <= 4u |p - s|), and FILTER is 2048 u.

`check_properties` is independent of the recursion: subsequence, ends kept, every dropped vertex within eps of the kept chord
that spans it, rings closed with at least 4 coordinates, short sequences unchanged."""
from __future__ import annotations

import math
from fractions import Fraction as F

import numpy as np

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from tests import exact_ref as X

LS, MLS, PG, MPG = _abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON
FILTER = 2.0**-42
CAP = 0.10  # at most this share of a randomized fixture's sequences may be unsettled
VECTOR_FROM = 24  # interior points from which the f64 distances of a node are taken in numpy


def simplify_group_size(n_coords: int, n_seq: int) -> int:
    """lanes per sequence of rdp_kernel / rdp_compact_kernel, restated from gpk_simplify: 8 up to a column mean of 48 coordinates
    per sequence (empty sequences count), 64 above; 0: no sequence, no launch"""
    if n_seq <= 0:
        return 0
    return 8 if n_coords / n_seq <= 48.0 else 64


def min_pts_of(geom_type: int) -> int:
    return 4 if geom_type in (PG, MPG) else 2


def inner_offsets(a: GeoArrowArray) -> np.ndarray:
    return a.ring_offsets if a.ring_offsets is not None else a.geom_offsets


def group_size_of(a: GeoArrowArray) -> int:
    return simplify_group_size(a.n_coords, len(inner_offsets(a)) - 1)


def sequences(a: GeoArrowArray):
    off = inner_offsets(a)
    return [a.xy[off[i] : off[i + 1]] for i in range(len(off) - 1)]


# ---- the f64 expression -------------------------------------------------------------------------------------------------------


def seg_dist_f64(px, py, sx, sy, ex, ey):
    """seg_dist of gpk_lineal_ops.hip / o_seg_dist of the oracle, operation for operation, in Python floats"""
    dx, dy = ex - sx, ey - sy
    if sx == ex and sy == ey:
        return math.sqrt((px - sx) * (px - sx) + (py - sy) * (py - sy))
    d2 = dx * dx + dy * dy
    r = ((px - sx) * dx + (py - sy) * dy) / d2
    if r <= 0.0:
        return math.sqrt((px - sx) * (px - sx) + (py - sy) * (py - sy))
    if r >= 1.0:
        return math.sqrt((px - ex) * (px - ex) + (py - ey) * (py - ey))
    t = ((sy - py) * dx - (sx - px) * dy) / d2
    return math.fabs(t) * math.sqrt(d2)


def seg_dist_f64_many(p: np.ndarray, s, e) -> np.ndarray:
    """the same operations on an (m, 2) array of points (numpy's elementwise f64 arithmetic and sqrt are IEEE, unfused)"""
    px, py = p[:, 0], p[:, 1]
    sx, sy, ex, ey = float(s[0]), float(s[1]), float(e[0]), float(e[1])
    ax, ay = px - sx, py - sy
    ds = np.sqrt(ax * ax + ay * ay)
    if sx == ex and sy == ey:
        return ds
    dx, dy = ex - sx, ey - sy
    d2 = dx * dx + dy * dy
    r = (ax * dx + ay * dy) / d2
    bx, by = px - ex, py - ey
    de = np.sqrt(bx * bx + by * by)
    t = ((sy - py) * dx - (sx - px) * dy) / d2
    return np.where(r <= 0.0, ds, np.where(r >= 1.0, de, np.abs(t) * math.sqrt(d2)))


# ---- exact arithmetic ---------------------------------------------------------------------------------------------------------


def _scaled_ints(xy: np.ndarray):
    """doubles -> integers over one power-of-two denominator: (list of (X, Y), denominator)"""
    ratios = [float(v).as_integer_ratio() for v in np.asarray(xy, dtype=np.float64).reshape(-1)]
    den = max((d for _, d in ratios), default=1)
    flat = [n * (den // d) for n, d in ratios]
    return list(zip(flat[0::2], flat[1::2])), den


def _d2_exact(p, s, e):
    """squared distance from p to the segment s-e as (numerator, denominator) of integers — line_segment_distance's three cases"""
    ax, ay = p[0] - s[0], p[1] - s[1]
    dx, dy = e[0] - s[0], e[1] - s[1]
    if dx == 0 and dy == 0:
        return ax * ax + ay * ay, 1
    dd = dx * dx + dy * dy
    dot = ax * dx + ay * dy
    if dot <= 0:
        return ax * ax + ay * ay, 1
    if dot >= dd:
        bx, by = p[0] - e[0], p[1] - e[1]
        return bx * bx + by * by, 1
    c = ax * dy - ay * dx
    return c * c, dd


class Rdp:
    """what rdp_exact found: keep[] (the expected answer), settled, and what the walk met on its way"""

    __slots__ = ("keep", "settled", "nodes", "depth", "ties", "eps_ties", "culled_ranges", "refused_ranges")

    def __init__(self, n):
        self.keep = np.ones(n, dtype=bool)
        self.settled = True
        self.nodes = 0  # ranges with an interior
        self.depth = 0  # most right-hand parts waiting at once (the kernel's explicit stack)
        self.ties = 0  # nodes whose rational maximum (> 0) is reached by more than one candidate
        self.eps_ties = 0  # nodes whose rational maximum equals eps exactly
        self.culled_ranges = 0
        self.refused_ranges = 0  # ranges within eps that kept their interior because of min_pts


def rdp_exact(xy, eps: float, min_pts: int) -> Rdp:
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    n = len(xy)
    res = Rdp(n)
    eps = float(eps)
    if n < 3 or eps <= 0.0:  # (a NaN eps is not <= 0: upstream goes on, and nothing is ever `> NaN`)
        return res
    P, den = _scaled_ints(xy)
    never = math.isnan(eps) or math.isinf(eps)
    E = None if never else F(eps) ** 2 * den * den  # eps^2 in the units of the scaled squared distances
    pf = [(float(x), float(y)) for x, y in xy]
    length = n
    stack = []
    ri, rj = 0, n - 1
    while True:
        if rj - ri >= 2:
            res.nodes += 1
            m = rj - ri - 1
            (sx, sy), (ex, ey) = pf[ri], pf[rj]
            if m < VECTOR_FROM:
                fd = [seg_dist_f64(pf[k][0], pf[k][1], sx, sy, ex, ey) for k in range(ri + 1, rj)]
                amax = max(abs(pf[k][0] - sx) + abs(pf[k][1] - sy) for k in range(ri + 1, rj))
                fbest = max(fd)
                f_at = ri + 1 + max(k for k in range(m) if fd[k] == fbest)
                cut = fbest - FILTER * (amax + abs(ex - sx) + abs(ey - sy))
                cand = [ri + 1 + k for k in range(m) if fd[k] >= cut]
            else:
                seg = xy[ri + 1 : rj]
                fd = seg_dist_f64_many(seg, pf[ri], pf[rj])
                amax = float(np.max(np.abs(seg[:, 0] - sx) + np.abs(seg[:, 1] - sy)))
                fbest = float(fd.max())
                f_at = ri + 1 + int(np.nonzero(fd == fbest)[0][-1])
                cut = fbest - FILTER * (amax + abs(ex - sx) + abs(ey - sy))
                cand = (ri + 1 + np.nonzero(fd >= cut)[0]).tolist()
            bn, bd, at, n_best = 0, 1, 0, 0
            for k in cand:  # ascending: `>=` leaves the last one among equals
                dn, dd = _d2_exact(P[k], P[ri], P[rj])
                c = dn * bd - bn * dd
                if c > 0 or n_best == 0:
                    bn, bd, at, n_best = dn, dd, k, 1
                elif c == 0:
                    at, n_best = k, n_best + 1
            if n_best > 1 and bn > 0:
                res.ties += 1
            split = False if never else bn * E.denominator > E.numerator * bd
            if not never and bn * E.denominator == E.numerator * bd:
                res.eps_ties += 1
            if f_at != at or (fbest > eps) != split:
                res.settled = False
            if split:
                stack.append((at, rj))
                res.depth = max(res.depth, len(stack))
                rj = at
                continue
            if length - m >= min_pts:
                length -= m
                res.keep[ri + 1 : rj] = False
                res.culled_ranges += 1
            else:
                res.refused_ranges += 1
        if not stack:
            break
        ri, rj = stack.pop()
    return res


_CACHE: dict = {}


def rdp_cached(xy, eps: float, min_pts: int) -> Rdp:
    """columns repeat sequences (copies, the same cases padded for both kernel instances): one walk per distinct input"""
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    key = (xy.tobytes(), np.float64(eps).tobytes(), min_pts)
    r = _CACHE.get(key)
    if r is None:
        r = _CACHE[key] = rdp_exact(xy, eps, min_pts)
    return r


def compare_exact(a: GeoArrowArray, eps: float, xy, off, cap: float = CAP, what=""):
    """an output (xy, innermost offsets) of simplify(a, eps) against the rationals on the settled sequences; the unsettled share is
    asserted against `cap` first.  -> (unsettled share, list of Rdp)"""
    seqs = sequences(a)
    mp = min_pts_of(a.geom_type)
    res = [rdp_cached(s, eps, mp) for s in seqs]
    judged = [r for s, r in zip(seqs, res) if len(s) >= 3]
    share = sum(not r.settled for r in judged) / max(len(judged), 1)
    assert share <= cap, (what, "unsettled share", share, len(judged))
    assert len(off) == len(seqs) + 1 and off[0] == 0, what
    for i, (s, r) in enumerate(zip(seqs, res)):
        if r.settled:
            got = xy[off[i] : off[i + 1]]
            assert np.array_equal(got, s[r.keep]), (what, i, eps, np.nonzero(r.keep)[0].tolist(), got.tolist())
    return share, res


# ---- properties that owe nothing to the recursion ---------------------------------------------------------------------------


def _frac_d2(p, s, e):
    """squared distance to the segment by the foot of the perpendicular, clamped — on Fractions"""
    dx, dy = e[0] - s[0], e[1] - s[1]
    dd = dx * dx + dy * dy
    t = F(0) if dd == 0 else min(max(((p[0] - s[0]) * dx + (p[1] - s[1]) * dy) / dd, F(0)), F(1))
    qx, qy = s[0] + t * dx - p[0], s[1] + t * dy - p[1]
    return qx * qx + qy * qy


def check_sequence_properties(seq, out, eps: float, min_pts: int, what=""):
    seq, out = np.asarray(seq, dtype=np.float64).reshape(-1, 2), np.asarray(out, dtype=np.float64).reshape(-1, 2)
    n, m = len(seq), len(out)
    eps = float(eps)
    if n < 3 or eps <= 0.0:
        assert np.array_equal(seq, out), (what, "must be unchanged")
        return
    assert m >= min(n, min_pts), (what, "fewer than min_pts", m)
    assert np.array_equal(out[0], seq[0]) and np.array_equal(out[-1], seq[-1]), (what, "ends")
    if np.array_equal(seq[0], seq[-1]):
        assert np.array_equal(out[0], out[-1]), (what, "ring opened")
    within_all = math.isnan(eps) or math.isinf(eps)
    e2 = None if within_all else F(eps) ** 2
    pts = None

    def spans(i, j):  # every vertex strictly between input positions i and j lies within eps of the chord i-j
        nonlocal pts
        if j - i < 2 or within_all:
            return True
        if pts is None:
            pts = [(F(float(x)), F(float(y))) for x, y in seq]
        return all(_frac_d2(pts[k], pts[i], pts[j]) <= e2 for k in range(i + 1, j))

    # some embedding of `out` into `seq` must satisfy the rule (equal coordinates can make more than one embedding possible)
    reach = {0}
    for t in range(1, m):
        where = np.nonzero((seq[:, 0] == out[t, 0]) & (seq[:, 1] == out[t, 1]))[0].tolist()
        if t == m - 1:
            where = [n - 1]
        reach = {j for j in where if any(i < j and spans(i, j) for i in reach)}
        assert reach, (what, "not a subsequence whose dropped vertices lie within eps of their chord", t)


def check_properties(a: GeoArrowArray, eps: float, xy, off, every: int = 1, what=""):
    mp = min_pts_of(a.geom_type)
    seqs = sequences(a)
    assert len(off) == len(seqs) + 1
    for i in range(0, len(seqs), every):
        check_sequence_properties(seqs[i], xy[off[i] : off[i + 1]], eps, mp, (what, i))


# ---- columns --------------------------------------------------------------------------------------------------------------------


def as_column(kind: int, seqs, null_every: int = 0) -> GeoArrowArray:
    """a flat list of sequences nested into rows of `kind` by a fixed ragged pattern (empty rows, several members, holes); with
    null_every = k every k-th row is null and keeps its coordinates"""
    seqs = [np.asarray(s, dtype=np.float64).reshape(-1, 2).tolist() for s in seqs]
    rows, i, step = [], 0, 0
    if kind == LS:
        rows, i = seqs, len(seqs)
    pattern = (1, 2, 0, 3, 1, 4)
    while i < len(seqs):
        k = pattern[step % len(pattern)]
        step += 1
        take = seqs[i : i + k]
        i += k
        if kind in (MLS, PG):
            rows.append(take)
        else:  # multipolygon: split the rings of the row between one or two members (the second ring of a member is a hole)
            rows.append([take[:2], take[2:]] if len(take) > 2 else ([take] if take else []))
    validity = [r % null_every != null_every - 1 for r in range(len(rows))] if null_every else None
    return X.column(kind, rows, validity)


BALLAST = [(float(k), float((k * 37) % 11 - 5)) for k in range(700)]  # a long lattice zigzag: lifts a column's mean


def force_instance(seqs, G: int, ring: bool = False):
    """the sequences plus what moves the column's mean to the 8- or the 64-lane instance: empty sequences, or copies of a long one"""
    seqs = list(seqs)
    total = sum(len(s) for s in seqs)
    if G == 8:
        while total > 48 * len(seqs):
            seqs.append([])
    else:
        long = BALLAST + ([BALLAST[0]] if ring else [])
        while total <= 48 * len(seqs):
            seqs.append(long)
            total += len(long)
    assert simplify_group_size(sum(len(s) for s in seqs), len(seqs)) == G
    return seqs


# ---- randomized lattice fixtures (the capped ones) ----------------------------------------------------------------------------
LATTICE_EPS = (0.5, 2.5, 3.0, 7.0)


def lattice_sequences(n: int, seed: int, ring: bool = False, lo: int = 3, hi: int = 200, step: int = 50):
    """integer walks with steps in +-step (steps in +-4 tie in most walks: kept for the deliberate tie families); rings close"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = int(rng.integers(lo, hi))
        w = np.cumsum(rng.integers(-step, step + 1, (k, 2)), axis=0).astype(np.float64)
        out.append(np.concatenate([w, w[:1]]) if ring else w)
    return out


def lattice_column(kind: int, n: int, seed: int) -> GeoArrowArray:
    return as_column(kind, lattice_sequences(n, seed, ring=kind in (PG, MPG)))


# ---- deliberate tie families ----------------------------------------------------------------------------------------------------
# Chord (0, 0) -> (L, 0) with L a power of two and dyadic interior points: r = x / L, t = -y / L and |t| * sqrt(L^2) = |y| are all
# exact, so every point at height +-h ties bit for bit with the others, and eps = h ties with the threshold.


def tie_line(n: int, ties, h: float = 0.25, signs=None, low: float = 0.0):
    """n coordinates along y = low (|low| < h) from (0, 0) to (L, 0), the interior indices `ties` lifted to +-h"""
    assert n >= 3 and all(1 <= k <= n - 2 for k in ties)
    L = 4.0
    while L < n:
        L *= 2.0
    pts = [(float(k), low) for k in range(n)]
    pts[0], pts[-1] = (0.0, 0.0), (L, 0.0)
    for q, k in enumerate(ties):
        pts[k] = (float(k), h * (1.0 if signs is None else signs[q]))
    return pts


def collinear_line(n: int):
    """every interior distance is exactly 0.0"""
    return tie_line(n, [])


def tie_pairs(n: int, G: int):
    """index pairs (k1 < k2) of a sequence of n coordinates by where the lanes of a G-wide group meet them (interior index k is
    taken by lane (k - 1) % G at the top range): -> {placement: (k1, k2)}"""
    lo, hi = 1, n - 2
    out = {}
    if hi > lo:
        out["first and last"] = (lo, hi)
        out["adjacent lanes"] = (lo, lo + 1)
    if lo + G <= hi:
        out["same lane"] = (lo, lo + G)
        out["same lane, last"] = (hi - G, hi)
    if G + 1 <= hi:
        out["later index in a lower lane"] = (G - 1, G + 1)  # lanes G - 2 and 0
        out["across the second pass"] = (G, G + 1)  # lane G - 1 of the first pass, lane 0 of the second
    if 2 * G + 2 <= hi:
        out["two passes apart, lower lane"] = (3, 2 * G + 2)  # lanes 2 and 1
    return out


def circle_ring(rep: int = 1):
    """a ring from (0, 0) through lattice points at distance exactly 65 from it (x*x + y*y = 4225 without rounding, so every one of
    them gives the double 65.0: the closed ring's chord is a point) with nearer points between, `rep` times round"""
    q1 = [(63, 16), (60, 25), (56, 33), (52, 39), (39, 52), (33, 56), (25, 60), (16, 63)]
    far = q1 + [(-y, x) for x, y in q1] + [(-x, -y) for x, y in q1] + [(y, -x) for x, y in q1]
    pts = [(0.0, 0.0)]
    for _ in range(rep):
        for q, (x, y) in enumerate(far):
            pts.append((float(x), float(y)))
            pts.append((float(x // 2), float(y // 2 + (q % 3) - 1)))
    return pts + [(0.0, 0.0)]


def comb(teeth: int, h: float = 0.5):
    """teeth of equal height on a power-of-two base, every other one pointing down, flat ground between: 3 * teeth + 2 coordinates"""
    L = 4.0
    while L < 3 * teeth + 2:
        L *= 2.0
    pts = [(0.0, 0.0)]
    for q in range(teeth):
        x = 3.0 * q + 1.0
        pts += [(x, 0.0), (x + 1.0, h if q % 2 == 0 else -h), (x + 2.0, 0.0)]
    return pts + [(L, 0.0)]


def staircase(steps: int, h: float = 1.0):
    """unit treads and risers: every chord the recursion meets has the corners of one side exactly tied"""
    pts = [(0.0, 0.0)]
    for q in range(steps):
        pts += [(float(q + 1), h * q), (float(q + 1), h * (q + 1))]
    return pts


def rectangle_with_midpoints(w: float = 8.0, hgt: float = 4.0, m: int = 3):
    """a closed rectangle whose sides carry m collinear dyadic points each"""
    corners = [(0.0, 0.0), (w, 0.0), (w, hgt), (0.0, hgt), (0.0, 0.0)]
    pts = []
    for (x0, y0), (x1, y1) in zip(corners[:-1], corners[1:]):
        pts.append((x0, y0))
        for q in range(1, m + 1):
            pts.append((x0 + (x1 - x0) * q / (m + 1), y0 + (y1 - y0) * q / (m + 1)))
    return pts + [(0.0, 0.0)]


def tie_family_lines():
    """(name, sequence, eps values): linestring sequences"""
    out = []
    for n in (3, 4, 5, 9, 17, 40):
        for name, (k1, k2) in tie_pairs(n, 8).items():
            for signs in ((1, 1), (1, -1)):
                out.append((f"tie_line {n} {name} {signs}", tie_line(n, [k1, k2], signs=signs), (0.25, math.nextafter(0.25, 0.0), 0.125, 1.0)))
        out.append((f"collinear {n}", collinear_line(n), (0.25, 2.0**-40)))
    out.append(("tie_line three", tie_line(30, [4, 11, 23], low=0.125), (0.25, math.nextafter(0.25, 0.0), 0.125, math.nextafter(0.125, 0.0))))
    for teeth in (1, 2, 5, 20):
        out.append((f"comb {teeth}", comb(teeth), (0.5, math.nextafter(0.5, 0.0), 0.25)))
    for steps in (2, 3, 8):
        out.append((f"staircase {steps}", staircase(steps), (0.25, 0.5, 1.0)))
    return out


def tie_family_rings():
    """(name, ring, eps values): polygon rings"""
    out = [(f"circle_ring {rep}", circle_ring(rep), (1.0, 8.0, 65.0, math.nextafter(65.0, 0.0), 1000.0)) for rep in (1, 3)]
    for m in (1, 3, 7):
        out.append((f"rectangle {m}", rectangle_with_midpoints(m=m), (0.5, 1.0, 4.0, 100.0)))
    return out


# ---- rings whose answer depends on the order of the walk (`simplified_len` is shared, the left part goes first) ----------------


def sliver_ring(m_left: int, m_right: int):
    """(0,0) -> m_left points just above the x axis -> (16 * 2^k, 0) -> m_right points just below it -> (0,0).  Under an eps of 4
    the far corner splits the ring, the left range culls first (len - m_left >= 4 as long as m_right >= 1) and the right range is
    then refused (3 coordinates would be left); reversed, the other side culls."""
    L = 16.0
    while L < 2 * max(m_left, m_right) + 2:
        L *= 2.0
    up = [(L * (q + 1) / (m_left + 1), 1.0 + (q % 2)) for q in range(m_left)]
    down = [(L * (m_right - q) / (m_right + 1), -2.0 - (q % 2)) for q in range(m_right)]
    return [(0.0, 0.0)] + up + [(L, 0.0)] + down + [(0.0, 0.0)]


ORDER_EPS = 4.0


def order_rings():
    """(name, ring): each is used forwards and reversed"""
    out = [(f"sliver {a}+{b}", sliver_ring(a, b)) for a, b in ((1, 1), (2, 1), (1, 3), (5, 7), (12, 3), (30, 30), (70, 9))]
    out.append(("triangle", [(0.0, 0.0), (6.0, 0.0), (3.0, 5.0), (0.0, 0.0)]))
    out.append(("five", [(0.0, 0.0), (6.0, 0.0), (6.0, 6.0), (0.0, 6.0), (0.0, 0.0)]))
    out.append(("identical", [(2.0, 3.0)] * 9))
    out.append(("thin sliver", [(0.0, 0.0), (10.0, 0.0), (10.0, 0.125), (5.0, 0.25), (0.0, 0.125), (0.0, 0.0)]))
    return out


# ---- deep stacks ---------------------------------------------------------------------------------------------------------------


def square_spiral(n: int):
    """corners of a square spiral from the centre outwards: seen from the centre the last-but-one corner is always the farthest, so
    every split leaves all but one segment on the left and the waiting right-hand parts pile up to about n - 2"""
    pts, x, y = [(0.0, 0.0)], 0, 0
    dirs = ((1, 0), (0, 1), (-1, 0), (0, -1))
    for q in range(n - 1):
        d = dirs[q % 4]
        x, y = x + d[0] * (q // 2 + 1), y + d[1] * (q // 2 + 1)
        pts.append((float(x), float(y)))
    return pts
