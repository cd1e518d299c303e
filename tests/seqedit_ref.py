"""segmentize, remove_repeated_points, reverse and orient_polygons in plain Python / numpy on a GeoArrowArray, written from the contract
in include/geopolars_hip.h (not from csrc/gpk_seqedit.h), and the hand-built case columns shared by tests/test_seqedit_host.py and
tests/test_gpu_seqedit.py.

A sequence is a run of coordinates under one entry of the innermost offsets level of a LINESTRING / MULTILINESTRING / POLYGON /
MULTIPOLYGON column; POINT and MULTIPOINT columns pass through every operation unchanged.  The segmentize arithmetic runs on scalar
Python floats, one IEEE operation a line, so that the order of operations is the contract's and nothing else; the orientation sign is
taken with rational arithmetic."""
import math
from fractions import Fraction

import numpy as np

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray

STRIP = 1024
EDITED = (_abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON)


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int32)
    off[1:] = np.cumsum(counts)
    return off


def _levels(a: GeoArrowArray):
    return [(k, getattr(a, k)) for k in ("geom_offsets", "part_offsets", "ring_offsets") if getattr(a, k) is not None]


def _rebuilt(a: GeoArrowArray, seq_off, xy) -> GeoArrowArray:
    """`a` with its innermost offsets and its coordinates replaced; every other level and the bitmap are the same arrays"""
    kw = {k: o for k, o in _levels(a)}
    kw[_levels(a)[-1][0]] = np.asarray(seq_off, np.int32)
    return GeoArrowArray(a.geom_type, np.asarray(xy, np.float64).reshape(-1, 2), validity=a.validity, n_geoms=len(a), **kw)


def _copy(a: GeoArrowArray) -> GeoArrowArray:
    return GeoArrowArray(a.geom_type, a.xy.copy(), a.geom_offsets, a.part_offsets, a.ring_offsets, a.validity, n_geoms=len(a))


def sequence_rows(a: GeoArrowArray) -> np.ndarray:
    """the row of every sequence"""
    owner = np.arange(len(a), dtype=np.int64)
    for _, off in _levels(a)[:-1]:
        owner = np.repeat(owner, np.diff(off))
    return owner


def pieces(px, py, qx, qy, m):
    if not m > 0.0:
        return 1
    dx = qx - px
    dy = qy - py
    sq = dx * dx + dy * dy
    len_ = math.sqrt(sq)  # (of NaN: NaN; of inf: inf)
    if not len_ > m or not math.isfinite(len_):
        return 1
    ratio = len_ / m
    return min(math.ceil(ratio), 1 << 31) if math.isfinite(ratio) else 1 << 31


def segmentize(a: GeoArrowArray, m) -> GeoArrowArray:
    """m: a float, or one float per row.  Raises OverflowError when the result does not fit i32 offsets."""
    if a.geom_type not in EDITED:
        return _copy(a)
    off = _levels(a)[-1][1]
    per_seq = np.full(len(off) - 1, float(m)) if np.ndim(m) == 0 else np.asarray(m, np.float64)[sequence_rows(a)]
    xy = a.xy
    out, new_off, total = [], [0], 0
    for s in range(len(off) - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        ms = float(per_seq[s])
        for c in range(lo, hi):
            out.append(xy[c])
            total += 1
            if c + 1 < hi:
                px, py, qx, qy = float(xy[c, 0]), float(xy[c, 1]), float(xy[c + 1, 0]), float(xy[c + 1, 1])
                n = pieces(px, py, qx, qy, ms)
                total += n - 1
                if total > 2**31 - 1:
                    raise OverflowError("segmentize: more than 2^31 - 1 coordinates")
                dx = qx - px
                dy = qy - py
                for j in range(1, n):
                    t = float(j) / float(n)
                    out.append((px + dx * t, py + dy * t))
        new_off.append(total)
    return _rebuilt(a, new_off, np.array(out, np.float64).reshape(-1, 2) if out else np.zeros((0, 2)))


def remove_repeated_points(a: GeoArrowArray) -> GeoArrowArray:
    if a.geom_type not in EDITED:
        return _copy(a)
    off = _levels(a)[-1][1].astype(np.int64)
    xy = a.xy
    keep = np.ones(len(xy), bool)
    if len(xy) > 1:
        with np.errstate(invalid="ignore"):
            keep[1:] = ~((xy[1:, 0] == xy[:-1, 0]) & (xy[1:, 1] == xy[:-1, 1]))
    keep[off[:-1][off[:-1] < len(xy)]] = True  # the first coordinate of every sequence (of an empty one: someone else's first)
    before = np.concatenate([[0], np.cumsum(keep)])
    return _rebuilt(a, before[off], xy[keep])


def reverse(a: GeoArrowArray, which=None) -> GeoArrowArray:
    """which: a bool per sequence (None: all)"""
    if a.geom_type not in EDITED:
        return _copy(a)
    off = _levels(a)[-1][1]
    xy = a.xy.copy()
    for s in range(len(off) - 1):
        if which is None or which[s]:
            xy[off[s]:off[s + 1]] = a.xy[off[s]:off[s + 1]][::-1]
    return _rebuilt(a, off, xy)


def exact_orient(u, v, w) -> int:
    ux, uy, vx, vy, wx, wy = (Fraction(float(t)) for t in (*u, *v, *w))
    d = (ux - wx) * (vy - wy) - (uy - wy) * (vx - wx)
    return (d > 0) - (d < 0)


def ring_turn(ring: np.ndarray):
    """(s, v, u, w): the exact sign of the turn at the lexicographically smallest coordinate and the three indices, or (0, ...) with
    None where the rule copies the ring unchanged without looking at a sign"""
    n = len(ring)
    if n < 4 or not np.isfinite(ring).all():
        return 0, None, None, None
    v = int(np.lexsort((ring[:-1, 1], ring[:-1, 0]))[0])  # (stable: the lowest index among equals; the closing coordinate is no candidate)
    same = lambda c: ring[c, 0] == ring[v, 0] and ring[c, 1] == ring[v, 1]  # noqa: E731
    u = next((c % n for c in (v - k for k in range(1, n)) if not same(c % n)), None)
    w = next((c % n for c in (v + k for k in range(1, n)) if not same(c % n)), None)
    if u is None or w is None:
        return 0, v, u, w
    return exact_orient(ring[u], ring[v], ring[w]), v, u, w


def orient_decisions(a: GeoArrowArray, exterior_cw: bool = False) -> np.ndarray:
    """a bool per ring: reversed or not"""
    roff = a.ring_offsets
    poly_off = a.part_offsets if a.geom_type == _abi.GEOM_MULTIPOLYGON else a.geom_offsets
    shell = np.zeros(len(roff) - 1, bool)
    starts = poly_off[:-1][np.diff(poly_off) > 0]
    shell[starts] = True
    rev = np.zeros(len(roff) - 1, bool)
    for r in range(len(roff) - 1):
        s = ring_turn(a.xy[roff[r]:roff[r + 1]])[0]
        want_ccw = bool(shell[r]) != bool(exterior_cw)
        rev[r] = s != 0 and (s > 0) != want_ccw
    return rev


def orient_polygons(a: GeoArrowArray, exterior_cw: bool = False) -> GeoArrowArray:
    if a.geom_type not in (_abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON):
        return _copy(a)
    return reverse(a, orient_decisions(a, exterior_cw))


OPS = {
    "segmentize": lambda a: segmentize(a, 7.5),
    "remove_repeated_points": remove_repeated_points,
    "reverse": reverse,
    "orient_polygons": orient_polygons,
    "orient_polygons cw": lambda a: orient_polygons(a, True),
}


def shoelace(ring: np.ndarray) -> float:
    """the f64 shoelace sum of a ring, in coordinate order"""
    s = 0.0
    for k in range(len(ring) - 1):
        s += float(ring[k, 0]) * float(ring[k + 1, 1]) - float(ring[k + 1, 0]) * float(ring[k, 1])
    return s


def sliver():
    """A triangle at (500000, 4649776) whose corners lie a few ulps off a line: its f64 shoelace sum is 0 or has the wrong sign, the
    exact orientation is decided.  Returns (ring, exact sign); asserts that the two disagree."""
    X, Y = 500000.0, 4649776.0
    ux, uy = np.spacing(X), np.spacing(Y)
    for k in range(1, 40):
        ring = np.array([[X, Y], [X + 64 * ux, Y + 64 * uy], [X + 128 * ux, Y + (128 + k) * uy], [X, Y]])
        exact = exact_orient(ring[0], ring[1], ring[2])
        f = shoelace(ring)
        if exact != 0 and (f > 0) - (f < 0) != exact:
            assert ring_turn(ring)[0] == exact
            return ring, exact
    raise AssertionError("no sliver found")


def polygons(rings_per_poly, rings) -> GeoArrowArray:
    """a POLYGON column from ring coordinate arrays as they are (nothing is closed or reordered)"""
    rings = [np.asarray(r, np.float64).reshape(-1, 2) for r in rings]
    xy = np.concatenate(rings) if rings else np.zeros((0, 2))
    return GeoArrowArray(_abi.GEOM_POLYGON, xy, geom_offsets=_offsets(rings_per_poly), ring_offsets=_offsets([len(r) for r in rings]))


def linestrings(lines) -> GeoArrowArray:
    lines = [np.asarray(l, np.float64).reshape(-1, 2) for l in lines]
    xy = np.concatenate(lines) if lines else np.zeros((0, 2))
    return GeoArrowArray(_abi.GEOM_LINESTRING, xy, geom_offsets=_offsets([len(l) for l in lines]))


def _circle(n, r=10.0, cx=0.0, cy=0.0, start=0, ccw=True):
    """a closed ring of n coordinates (n - 1 distinct) on a circle; `start` rotates which corner comes first"""
    k = (np.arange(n - 1) + start) % (n - 1)
    t = 2 * np.pi * k / (n - 1) * (1 if ccw else -1)
    ring = np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1)
    return np.concatenate([ring, ring[:1]])


def segmentize_cases():
    """{name: (column, m)}: the strip size of the fill is 1024 output coordinates"""
    c = {}
    c["1025 outputs of one segment"] = (linestrings([[(0, 0), (1024, 0)]]), 1.0)
    c["1024 outputs of one segment"] = (linestrings([[(0, 0), (1024, 0)]]), 1024 / 1023)
    c["1023 outputs of one segment"] = (linestrings([[(0, 0), (1024, 0)]]), 1024 / 1022)
    c["1025 unsplit coordinates"] = (linestrings([np.stack([np.arange(1025.0), np.arange(1025.0) % 2], 1)]), 10.0)
    c["5000 pieces between unsplit neighbours"] = (linestrings([[(-1, 0), (0, 0), (5000, 0), (5000.5, 0.5)]]), 1.0)
    c["zero-length segment"] = (linestrings([[(1, 1), (1, 1), (4, 1)], [(2, 2), (2, 2)]]), 1.0)
    # ring 0 splits into 300 + 299 + 424 pieces: outputs 0 .. 1023; ring 1 begins at output 1024 with a long segment
    ring0 = [(0, 0), (300, 0), (300, 299), (0, 0)]
    ring1 = [(3000, 0), (3007, 0), (3007, 9), (3000, 0)]
    c["sequence boundary at the strip boundary"] = (polygons([2], [ring0, ring1]), 1.0)
    c["m larger than every segment"] = (linestrings([[(0, 0), (3, 4), (-0.0, 2)], [(5, 5), (6, 6)]]), 100.0)
    c["georeferenced"] = (linestrings([[(500000, 4649776), (500003.3, 4649777.7), (500003.3, 4649790.1)]]), 0.1)
    c["NaN and inf"] = (linestrings([[(0, 0), (np.nan, 5), (8, 0), (np.inf, 0), (9, 9), (12, 13)]]), 1.0)
    c["0.3 / 0.1"] = (linestrings([[(0, 0), (0.3, 0)], [(0, 0), (0, 0.3)]]), 0.1)
    return c


def dedup_cases():
    c = {}
    xy = np.stack([np.arange(1100.0), np.zeros(1100)], 1)
    xy[1015:1035] = xy[1015]  # a run of repeats across coordinate 1024
    c["a run across 1024"] = linestrings([xy])
    a, b, d = (0.0, 0.0), (4.0, 0.0), (4.0, 3.0)
    c["repeats across a sequence boundary"] = polygons([2], [[a, b, d, a], [a, a, d, b, b, a]])
    c["-0.0 after 0.0"] = linestrings([[(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (1.0, 0.0)]])
    c["NaN after NaN"] = linestrings([[(np.nan, 1.0), (np.nan, 1.0), (2.0, np.nan), (2.0, np.nan), (3.0, 3.0), (3.0, 3.0)]])
    c["a collapsed ring"] = polygons([1, 1], [[a, a, a, a], [a, b, d, a]])
    c["no repeats"] = linestrings([[(0, 0), (1, 0), (0, 0), (1, 0)], [(1, 0), (2, 2)]])
    c["no coordinates"] = GeoArrowArray(_abi.GEOM_LINESTRING, np.zeros((0, 2)), geom_offsets=_offsets([0, 0, 0]))
    return c


def reverse_cases():
    c = {}
    lens = [2500, 572, 1, 0, 2]
    c["three strips"] = GeoArrowArray(_abi.GEOM_LINESTRING, np.random.default_rng(31).uniform(-50, 50, (sum(lens), 2)), geom_offsets=_offsets(lens))
    lens = [3] + [0] * 5000 + [4, 0, 2]
    c["5000 empty sequences"] = GeoArrowArray(_abi.GEOM_LINESTRING, np.random.default_rng(32).uniform(-50, 50, (sum(lens), 2)), geom_offsets=_offsets(lens))
    c["closed rings"] = polygons([2, 1], [_circle(9), _circle(5, 2.0), _circle(40, 3.0, 100.0, 5.0)])
    return c


def orient_cases():
    c = {}
    sq = np.array([(0, 0), (10, 0), (10, 10), (0, 10), (0, 0)], float)
    hole = np.array([(2, 2), (4, 2), (4, 4), (2, 4), (2, 2)], float)
    c["squares and holes both ways"] = polygons([1, 1, 2, 2, 2, 2], [sq, sq[::-1], sq, hole, sq, hole[::-1], sq[::-1], hole, sq[::-1], hole[::-1]])
    ring, _ = sliver()
    c["sliver"] = polygons([1, 1], [ring, ring[::-1]])
    v, p, q = (0.0, 0.0), (5.0, 1.0), (1.0, 5.0)
    c["smallest repeated"] = polygons([1, 1, 1, 1], [[v, v, p, q, v], [v, v, q, p, v], [v, p, q, v, v], [v, q, p, v, v]])
    c["spike"] = polygons([1, 1], [[v, (3.0, 3.0), (6.0, 6.0), (3.0, 3.0), v], [v, p, v, p, v]])
    c["NaN ring"] = polygons([1], [[v, p, (np.nan, 2.0), q, v]])
    c["inf closing"] = polygons([1], [[(np.inf, 0.0), p, q, v, (np.inf, 0.0)]])
    c["3-coordinate ring"] = polygons([2], [[v, q, p], [v, p, q, v]])
    c["unclosed"] = polygons([1, 1], [[v, q, p, (6.0, 6.0)], [(6.0, 6.0), p, q, v]])
    # 256 coordinates is the longest ring a lane group takes; 257 goes to a work-group
    c["rings of 256 and 257 coordinates"] = polygons([1, 1, 1, 1], [_circle(256, 30.0, ccw=False), _circle(257, 30.0, ccw=False), _circle(256, 30.0), _circle(257, 30.0)])
    n = 5000
    rings = []
    for ccw in (True, False):
        base = _circle(n, 1000.0, ccw=ccw)
        at = int(np.lexsort((base[:-1, 1], base[:-1, 0]))[0])
        for start in (at, at + 1, at + n // 2):  # the minimum at index 0, at the last index before the closing one, mid-ring
            rings.append(_circle(n, 1000.0, start=start, ccw=ccw))
    c["5000-coordinate rings"] = polygons([1, 1, 2, 2], rings)
    return c


def case_columns():
    """every hand-built column by name (for runs of all four operations)"""
    out = {}
    for k, (a, _) in segmentize_cases().items():
        out["segmentize: " + k] = a
    for prefix, cases in (("dedup", dedup_cases()), ("reverse", reverse_cases()), ("orient", orient_cases())):
        for k, a in cases.items():
            out[f"{prefix}: {k}"] = a
    return out
