"""Fixtures on which Shewchuk's stage-A orientation filter gives up although the exact sign is NOT zero, for
tests/test_gpu_hard_orient.py (GPU) and tests/test_hard_orient.py (no GPU: what these fixtures promise is checked there, on the
references alone).

Every exact kernel decides an orientation in two steps: a double-precision determinant with the stage-A error bound, and an
expansion-arithmetic arm when the bound cannot certify the sign.  On coordinates that are small integers times one power of two (the
lattice fixtures, every PLACEMENTS list) the determinant is exact: the exact arm runs only for true zeros, where it returns what
`sign(det)` returns too, and a kernel whose exact arm is wrong — or missing — passes.  The rows here are different: `stage_a`
replicates the filter of csrc line for line, `exact` gives the sign on the doubles' rational values, and the generators draw triples
by rejection until the filter is uncertain and the double determinant has the WRONG sign (or is 0) under all six argument orders.

Classes of an evaluation (an ordered triple): Z exact sign zero; F filter certain; U uncertain, exact sign non-zero, double sign
right; W uncertain, exact sign non-zero, double sign wrong or zero.  Kinds of a triple: see KINDS; the composition of every column
is COMPOSITION (of every 8 rows).

Census of the inexact fixtures the suite had before these tests, evaluations in dev::orient2d's argument order (edge start, edge end,
point); tests/test_hard_orient.py::test_census_of_earlier_fixtures prints it:

    fixture                                                        evaluations       Z        F     U     W
    test_gpu_georeferenced: probe_points on buildings                     3994     962     3032     0     0
    test_gpu_georeferenced: probe_points on linestrings                   2917     683     2234     0     0
    test_gpu_contains: the first 1500 of the 6000 nudged pairs          420336   18807   400696   540   293
    test_gpu_lineclip: the 256 sliver rows                                5632       0     5632     0     0
    test_gpu_validity: the three slope-1/3 rows                             93       2       87     4     0
    hard_orient.triples(gen), each of the three: planted, six orders      1152     144      144   288   576

The constructive kernels — gpk_line_clip, gpk_polygon_clip, gpk_polygon_union with union_all, gpk_intersection_measure and
gpk_orient_polygons — take these rows through the figures at the end of "the figure around a triple" (pass, spike ring, nested hole,
hinge), as columns in tests/hard_clip.py and on the GPU in tests/test_gpu_hard_clip.py.  Two families need no such rows, because they
hold no orientation predicate at all: representative_point (gpk_interior.h) is floating arithmetic defined bit for bit, and
segmentize only divides segments.

For point probes an evaluation is an edge whose closed box holds the point (what coord_pos_relative_to_ring asks); for pairs of rows it
is every segment of one row against every vertex of the other.  The W evaluations of the nudged pairs reach `contains` only; the
georeferenced probes hold none at all, although they lie 1 - 2 ulps off their edges: at UTM magnitudes with metre-sized features the
differences are exact and the determinant is far above the bound.
"""
from __future__ import annotations

import itertools
import math
import os
import re
from fractions import Fraction
from functools import lru_cache
from typing import NamedTuple, Optional

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "geopolars_amd", "csrc")
STAGE_A = 3.3306690738754716e-16  # (3 + 16 eps) eps, eps = 2^-53: the constant of every stage-A site in csrc
NEW = "tests/test_gpu_hard_orient.py"


# ---- the filter and the exact sign -------------------------------------------------------------------------------------------------------


def stage_a(a, b, c):
    """(certain, sign of the double determinant): dev::orient2d of gpk_device.h up to the point where it returns or calls the exact arm"""
    ax, ay, bx, by, cx, cy = float(a[0]), float(a[1]), float(b[0]), float(b[1]), float(c[0]), float(c[1])
    detleft = (ax - cx) * (by - cy)
    detright = (ay - cy) * (bx - cx)
    det = detleft - detright
    detsum = abs(detleft) + abs(detright)
    errbound = STAGE_A * detsum
    opposite = (detleft > 0.0 and detright <= 0.0) or (detleft < 0.0 and detright >= 0.0) or detleft == 0.0
    certain = opposite or abs(det) >= errbound
    return certain, (det > 0.0) - (det < 0.0)


def exact(a, b, c) -> int:
    """the sign of the same determinant on the doubles' exact values: +1 when c is left of a -> b"""
    ax, ay, bx, by, cx, cy = [Fraction(float(v)) for v in (*a, *b, *c)]
    d = (ax - cx) * (by - cy) - (ay - cy) * (bx - cx)
    return (d > 0) - (d < 0)


def naive(a, b, c) -> int:
    """what a kernel without an exact arm computes"""
    return stage_a(a, b, c)[1]


def classify(a, b, c) -> str:
    s = exact(a, b, c)
    if s == 0:
        return "Z"
    certain, d = stage_a(a, b, c)
    if certain:
        assert d == s, "stage A certified a wrong sign"
        return "F"
    return "U" if d == s else "W"


ORDERS = list(itertools.permutations(range(3)))


def classes(a, b, c) -> str:
    """the classes of the six argument orders, as one string"""
    t = (a, b, c)
    return "".join(classify(t[i], t[j], t[k]) for i, j, k in ORDERS)


def uncertain_everywhere(a, b, c) -> bool:
    t = (a, b, c)
    return not any(stage_a(t[i], t[j], t[k])[0] for i, j, k in ORDERS)


HARD_LEFT, HARD_RIGHT, UNSURE, COLLINEAR, EASY = "hard-left", "hard-right", "unsure", "collinear", "easy"
KINDS = {
    HARD_LEFT: "W under ALL six orders (the issue asks for W under one and uncertain under six: whatever order or difference form a "
               "kernel uses, the sign of its double determinant is wrong), c left of a -> b",
    HARD_RIGHT: "the same, c right of a -> b",
    UNSURE: "uncertain under all six orders, exact sign non-zero, the double sign right under all six",
    COLLINEAR: "exactly collinear at wide mantissas: uncertain under all six orders, exact sign zero",
    EASY: "certain under all six orders",
}
# of every 8 rows of a column, in this order (a column's length is a multiple of 8)
COMPOSITION = (HARD_LEFT, HARD_RIGHT, UNSURE, HARD_LEFT, COLLINEAR, HARD_RIGHT, UNSURE, EASY)
HARD = (HARD_LEFT, HARD_RIGHT)


def _parity(p) -> int:
    return 1 if p in ((0, 1, 2), (1, 2, 0), (2, 0, 1)) else -1


def kind_of(a, b, c) -> Optional[str]:
    """the kind of a triple, None when it is none of KINDS.  (One exact evaluation: the sign under another order is the sign times the
    order's parity — tests/test_hard_orient.py holds this short cut to `classes`.)"""
    t = (a, b, c)
    got = [stage_a(t[i], t[j], t[k]) for i, j, k in ORDERS]
    n_certain = sum(1 for certain, _ in got if certain)
    if 0 < n_certain < 6:
        return None
    s = exact(a, b, c)
    if n_certain == 6:
        assert all(d == s * _parity(p) for (_, d), p in zip(got, ORDERS)), "stage A certified a wrong sign"
        return EASY if s != 0 else None
    if s == 0:
        return COLLINEAR
    wrong = [d != s * _parity(p) for (_, d), p in zip(got, ORDERS)]
    if all(wrong):
        return HARD_LEFT if s > 0 else HARD_RIGHT
    return None if any(wrong) else UNSURE


class Triple(NamedTuple):
    a: tuple
    b: tuple
    c: tuple  # between a and b along the edge (0.2 <= t <= 0.8), at most a few ulps off its line — or far off it (EASY)
    kind: str

    @property
    def sign(self) -> int:
        return exact(self.a, self.b, self.c)


# ---- generators --------------------------------------------------------------------------------------------------------------------------

T_LO, T_HI = 0.2, 0.8  # c's parameter along a -> b: well inside the edge, so that no box test and no end-point rule can decide


def _moved(c, rng):
    """c moved by 0 .. +-2 ulps in x or in y"""
    k = int(rng.integers(-2, 3))
    if rng.integers(0, 2):
        return (c[0] + k * float(np.spacing(c[0])), c[1])
    return (c[0], c[1] + k * float(np.spacing(c[1])))


def _near(a, b, rng):
    t = float(rng.uniform(T_LO, T_HI))
    return _moved((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])), rng)


def _easy(a, b, rng):
    """c a tenth of the edge's length off its middle part, to the left or to the right"""
    t, s = float(rng.uniform(T_LO, T_HI)), float(rng.choice([-0.1, 0.1]))
    return (a[0] + t * (b[0] - a[0]) - s * (b[1] - a[1]), a[1] + t * (b[1] - a[1]) + s * (b[0] - a[0]))


def _collinear(lo_a, hi_a, lo_b, hi_b, rng):
    """a, b in their boxes and c = a + (k / m) (b - a) exactly: integers below 2^53 times 2^-47 (the ulp of [32, 64)), so that every
    coordinate has a wide mantissa and no product of the determinant is exact"""
    u = 2.0**-47
    A = [int(rng.uniform(lo_a[i], hi_a[i]) / u) for i in (0, 1)]
    B = [int(rng.uniform(lo_b[i], hi_b[i]) / u) for i in (0, 1)]
    m = int(rng.integers(5, 1000))
    D = [(B[i] - A[i]) // m for i in (0, 1)]
    k = int(rng.integers(max(1, int(T_LO * m) + 1), max(2, int(T_HI * m))))
    pt = lambda j: tuple(float(A[i] + j * D[i]) * u for i in (0, 1))  # noqa: E731
    a, b, c = pt(0), pt(m), pt(k)
    assert all(Fraction(v) == Fraction(A[i] + j * D[i]) * Fraction(u) for j, p in ((0, a), (m, b), (k, c)) for i, v in enumerate(p))
    return a, b, c


MIXED_BOXES = ((0.1, 0.1), (1.0, 1.0), (8.0, 8.0), (64.0, 64.0))  # a in [0.1, 1]^2, b in [8, 64]^2: degrees near Greenwich or the equator
DEGREE_BOXES = ((-3.0, 40.0), (3.0, 60.0), (-3.0, 40.0), (3.0, 60.0))  # x in [-3, 3], y in [40, 60]


def _boxed(boxes):
    lo_a, hi_a, lo_b, hi_b = boxes

    def draw(kind, rng):
        if kind == COLLINEAR:
            return _collinear(lo_a, hi_a, lo_b, hi_b, rng)
        a = (float(rng.uniform(lo_a[0], hi_a[0])), float(rng.uniform(lo_a[1], hi_a[1])))
        b = (float(rng.uniform(lo_b[0], hi_b[0])), float(rng.uniform(lo_b[1], hi_b[1])))
        return a, b, (_easy(a, b, rng) if kind == EASY else _near(a, b, rng))

    return draw


def _grid(kind, rng):
    """the perturbed grid: a = (0.5 + i 2^-53, 0.5 + j 2^-53), i, j < 16, the point (12, 12) and the far end (24, 24); here the point
    between the two others is called c.  The grid has no UNSURE and no EASY triple of its own, so those two kinds move (12, 12): by
    up to 2 ulps, and by a tenth of the edge."""
    i, j = int(rng.integers(0, 16)), int(rng.integers(0, 16))
    a, b, c = (0.5 + i * 2.0**-53, 0.5 + j * 2.0**-53), (24.0, 24.0), (12.0, 12.0)
    if kind == COLLINEAR:
        a = (a[0], a[0])
    elif kind == UNSURE:
        c = _moved(c, rng)
    elif kind == EASY:
        c = _easy(a, b, rng)
    return a, b, c


GENERATORS = {"mixed": _boxed(MIXED_BOXES), "degree": _boxed(DEGREE_BOXES), "grid": _grid}
N_ROWS = 192
SEEDS = {"mixed": 101, "degree": 102, "grid": 103}


@lru_cache(maxsize=None)
def triples(gen: str, n: int = N_ROWS, seed: Optional[int] = None):
    """a column of n triples with exactly COMPOSITION, drawn by rejection"""
    assert n % len(COMPOSITION) == 0
    rng = np.random.default_rng(SEEDS[gen] if seed is None else seed)
    draw, out, seen = GENERATORS[gen], [], set()
    for i in range(n):
        want = COMPOSITION[i % len(COMPOSITION)]
        for _ in range(100000):
            a, b, c = draw(want, rng)
            if ((a, b, c) not in seen or (gen == "grid" and want == COLLINEAR)) and kind_of(a, b, c) == want:  # (the grid has 16 collinear triples)
                break
        else:
            raise AssertionError((gen, want))
        seen.add((a, b, c))
        out.append(Triple(a, b, c, want))
    return tuple(out)


def composition(rows) -> dict:
    """{kind: count} by classifying the rows anew (not by their labels)"""
    out = {}
    for t in rows:
        k = kind_of(t.a, t.b, t.c)
        out[k] = out.get(k, 0) + 1
    return out


def stated_composition(n: int) -> dict:
    return {k: COMPOSITION.count(k) * n // len(COMPOSITION) for k in KINDS}


# ---- exact symmetries ---------------------------------------------------------------------------------------------------------------------
#
# Each returns a Triple and asserts on itself that no evaluation changed its class (a mirror turns left into right: the kind follows).


def _same_classes(t: Triple, u: Triple, permuted: bool = False) -> Triple:
    before, after = classes(t.a, t.b, t.c), classes(u.a, u.b, u.c)
    assert (sorted(before) == sorted(after)) if permuted else (before == after), (t, u, before, after)
    assert kind_of(u.a, u.b, u.c) == u.kind, (t, u)
    return u


def _flipped(kind):
    return {HARD_LEFT: HARD_RIGHT, HARD_RIGHT: HARD_LEFT}.get(kind, kind)


def swap_ab(t: Triple) -> Triple:
    return _same_classes(t, Triple(t.b, t.a, t.c, _flipped(t.kind)), permuted=True)


def mirror_x(t: Triple) -> Triple:
    m = lambda p: (-p[0], p[1])  # noqa: E731
    return _same_classes(t, Triple(m(t.a), m(t.b), m(t.c), _flipped(t.kind)))


def swap_xy(t: Triple) -> Triple:
    m = lambda p: (p[1], p[0])  # noqa: E731
    return _same_classes(t, Triple(m(t.a), m(t.b), m(t.c), _flipped(t.kind)))


def scaled(t: Triple, k: int) -> Triple:
    m = lambda p: (math.ldexp(p[0], k), math.ldexp(p[1], k))  # noqa: E731
    return _same_classes(t, Triple(m(t.a), m(t.b), m(t.c), t.kind))


SYMMETRIES = {"swap a and b": swap_ab, "mirror x": mirror_x, "swap x and y": swap_xy, "scale 2^20": lambda t: scaled(t, 20), "scale 2^-20": lambda t: scaled(t, -20)}


def rotated(ring, k: int):
    """a closed ring started k vertices later: the same edges, so the same evaluations"""
    body = list(ring[:-1])
    k %= len(body)
    out = body[k:] + body[:k]
    out.append(out[0])
    assert ring[0] == ring[-1] and set(zip(ring[:-1], ring[1:])) == set(zip(out[:-1], out[1:]))
    return out


SCALE_STEP, PER_CLASS = 10, 8  # [0.1, 64] times 2^10 lies beyond 64: the boxes of two scale classes are apart


@lru_cache(maxsize=None)
def placed_triples(gen: str, n: int = 64):
    """the first n triples of the column, every block of PER_CLASS rows at its own scale 2^(SCALE_STEP j): rows of different blocks
    have boxes far apart, so a join of two columns built from them has n * PER_CLASS candidate pairs instead of n * n"""
    out = []
    for i, t in enumerate(triples(gen)[:n]):
        out.append(scaled(t, SCALE_STEP * (i // PER_CLASS - n // PER_CLASS // 2)))
    return tuple(out)


# ---- the figure around a triple -----------------------------------------------------------------------------------------------------------
#
# at(t, u, v) = a + u (b - a) + v n, n the left normal of a -> b with the edge's length: u runs along the edge, v > 0 is left of it.
# Far points are tenths of the edge's length away from its line: certain under every order (only_planted_is_uncertain checks it).


def at(t: Triple, u: float, v: float):
    dx, dy = t.b[0] - t.a[0], t.b[1] - t.a[1]
    return (t.a[0] + u * dx - v * dy, t.a[1] + u * dy + v * dx)


def along(t: Triple) -> float:
    dx, dy = t.b[0] - t.a[0], t.b[1] - t.a[1]
    return ((t.c[0] - t.a[0]) * dx + (t.c[1] - t.a[1]) * dy) / (dx * dx + dy * dy)


def far_left(t):
    return at(t, 0.5, 0.6)  # r: the apex of the polygon (a, b, r)


def far_right(t):
    return at(t, along(t), -0.5)  # q: c -> q leaves the edge at a right angle, to the right


def far_right_pair(t):
    u = along(t)
    return at(t, u - 0.2, -0.5), at(t, u + 0.2, -0.5)  # q2, q1: (c, q2, q1) is counter-clockwise


def arc(t: Triple, k: int, side: int = 1):
    """k points over a half ellipse through at(t, 0.5, 0.6 side): side +1 from b back to a on the left of the edge, -1 from a on to b on
    its right (either way the ring through a, b and the arc is counter-clockwise when it starts b, a)"""
    th = [math.pi * (j + 1) / (k + 1) for j in range(k)]
    return [at(t, 0.5 + side * 0.5 * math.cos(x), side * 0.6 * math.sin(x)) for x in th]


def only_planted_is_uncertain(t: Triple, points) -> bool:
    """every triple of a, b, c and `points` other than {a, b, c} itself is certain under all six orders, and every far point lies on
    the side its construction says (EASY rows: also {a, b, c})"""
    named = [t.a, t.b, t.c] + list(points)
    for i, j, k in itertools.combinations(range(len(named)), 3):
        if (i, j, k) == (0, 1, 2):
            continue
        if kind_of(named[i], named[j], named[k]) != EASY:
            return False
    return True


ARC = 45  # a ring a, b, 45 arc points and the closing coordinate: 48 coordinates, past the 32 that select the larger lane group
assert ARC % 2 == 1  # (the middle arc point is at(t, 0.5, 0.6): line_row's cut leaves it at the front)


def polygon_row(t: Triple, long: bool = False):
    """POLYGON (a, b, r), counter-clockwise: c is inside when it is left of a -> b.  long: the planted edge in a ring of 48 coordinates"""
    return [[t.a, t.b] + (arc(t, ARC) if long else [far_left(t)]) + [t.a]]


def line_row(t: Triple, long: bool = False):
    """LINESTRING [a, b]; long: the ring of polygon_row cut open at its top, a -> b in the middle of 47 coordinates"""
    if not long:
        return [t.a, t.b]
    pts = arc(t, ARC)
    return pts[ARC // 2 :] + [t.a, t.b] + pts[: ARC // 2]


def probe_line(t: Triple):
    return [t.c, far_right(t)]  # [c, q]: crosses [a, b] when c is left of it, ends on it when collinear, misses it otherwise


def probe_triangle(t: Triple):
    q2, q1 = far_right_pair(t)
    return [[t.c, q2, q1, t.c]]  # overlaps (a, b, r) / touches it at c / is disjoint


def probe_points(t: Triple):
    return [t.c, far_right(t)]  # MULTIPOINT: c and a point outside everything


def hole_row(t: Triple, long: bool = False):
    """POLYGON: the shell (a, b, r) on the side of a -> b that has the larger x, and a small triangular hole whose lowest (x, y) vertex
    — the one gpk_triangulate bridges from — is c.  Valid when c lies strictly on the shell's side (the hole is inside) or on the edge
    (the hole touches it), RINGS_CROSS when c is an ulp beyond.  long: the shell has 48 coordinates."""
    dx, dy = t.b[0] - t.a[0], t.b[1] - t.a[1]
    L = math.hypot(dx, dy)
    s = 1.0 if -dy > 0 else -1.0
    if s > 0:
        shell = [t.a, t.b] + (arc(t, ARC) if long else [at(t, 0.5, 0.6)]) + [t.a]
    else:
        shell = [t.b, t.a] + (arc(t, ARC, -1) if long else [at(t, 0.5, -0.6)]) + [t.b]
    gx, gy = s * -dy / L + 1.0, s * dx / L  # between the inward normal and +x: within 45 degrees of both
    g = math.hypot(gx, gy)
    hs = []
    for turn in (math.radians(15.0), math.radians(-15.0)):
        ux, uy = (gx * math.cos(turn) - gy * math.sin(turn)) / g, (gx * math.sin(turn) + gy * math.cos(turn)) / g
        hs.append((t.c[0] + 0.08 * L * ux, t.c[1] + 0.08 * L * uy))
    assert t.c[0] < min(h[0] for h in hs)
    return [shell, [t.c, hs[0], hs[1], t.c]]  # the hole clockwise


def chain_row(t: Triple):
    """POLYGON a, c, b, r: the vertex c between a and b is reflex when it is left of a -> b, convex when right, collinear when on it"""
    return [[t.a, t.c, t.b, far_left(t), t.a]]


def notch_row(t: Triple):
    """POLYGON a, x, b, c, w (x right of a -> b, w left): c is a reflex vertex next to the diagonal a - b.  c left of a -> b: (a, x, b)
    is an ear; c right of it or on it: the ear holds c and must not be cut"""
    return [[t.a, at(t, 0.5, -0.6), t.b, t.c, at(t, along(t), 0.6), t.a]]


def members_row(t: Triple, long: bool = False):
    """MULTIPOLYGON: (a, b, r) and the triangle (c, q2, q1) on the other side of a -> b: disjoint, touching at c, or overlapping"""
    return [polygon_row(t, long), probe_triangle(t)]


def inner_point(t: Triple):
    return at(t, along(t), 0.3)  # w: left of the edge, inside (a, b, r) and inside the arc


def self_line_row(t: Triple, long: bool = False):
    """LINESTRING a, b, w, c with w on the left: simple when c stops short of a -> b (c left of it), not simple when c is on it or
    beyond it.  long: the 47 coordinates of line_row(t, True), then w and c"""
    return line_row(t, long) + [inner_point(t), t.c]


def two_lines_row(t: Triple, long: bool = False):
    """MULTILINESTRING [a, b] and [w, c]: the same question between two members"""
    return [line_row(t, long), [inner_point(t), t.c]]


def hull_row(t: Triple):
    return [t.a, t.b, t.c, far_left(t)]  # MULTIPOINT: c is a hull vertex only when it is right of a -> b


# ---- figures for the constructive kernels: line clip, polygon clip, union, overlay measure, orient_polygons ---------------------------------
#
# A constructive kernel returns geometry, so a wrong sign shows as another SHAPE (parts, rings, coordinates per ring, which input
# coordinate stands where), not as another mask.  tests/test_hard_orient.py holds every figure to: COMPOSITION kept, only the planted
# triple uncertain, transitions apart by the headers' own definition (transition_gap of the references), one shape per exact sign,
# and the shapes of + and - different for every operation.


def rot90(t: Triple) -> Triple:
    """(x, y) -> (-y, x), exact: swap_xy then mirror_x.  Two mirrors: every class AND the kind stay"""
    return mirror_x(swap_xy(t))


def rot180(t: Triple) -> Triple:
    return rot90(rot90(t))


def pass_points(t: Triple):
    """w inside (a, b, r) — and inside the arc of the long ring —, q1 and q2 outside, on the right of a -> b"""
    u = along(t)
    return at(t, u - 0.05, 0.1), at(t, u + 0.05, -0.2), at(t, u - 0.10, -0.2)


def pass_polygon(t: Triple):
    """POLYGON (w, c, q1, q2), stored clockwise: its boundary passes through the vertex c from the inside of A = polygon_row(t) to its
    outside.  c left of a -> b: c is inside A and c -> q1 crosses ab right after c; c right of it: w -> c crosses ab right before c;
    collinear: c is a vertex of B on the open edge ab.  gpk_lineclip.h / gpk_polyclip.h decide it in lp::side_bits at c, in the
    crossing tests of w -> c and c -> q1 against ab, in crossing_type (orient(a, b, q) of the crossing segment's far end) and, walking
    the edge ab of A, in event_before's "(b) against (c)" rule: the vertex c of B against the crossings of B's two edges at c"""
    w, q1, q2 = pass_points(t)
    return [[w, t.c, q1, q2, w]]


def pass_line(t: Triple):
    """LINESTRING w, c, q1: the two edges of pass_polygon that meet at c.  Inside A it is [w, c, x] with a crossing x after c when c is
    left of a -> b, [w, c] when collinear, [w, x] with x before c when right; outside A the rest"""
    w, q1, _q2 = pass_points(t)
    return [w, t.c, q1]


def far_triangle(t: Triple, k: int = 0):
    """a counter-clockwise triangle three edge lengths away from the figure: the first member of the MULTIPOLYGON forms (k = 0 beside
    A, on the left; k = 1 beside B, on the right)"""
    u, v = (3.0, 3.0) if k == 0 else (-2.7, -3.3)  # (no edge of one in line with a vertex of the other)
    p, q, r = at(t, u, v), at(t, u + 0.5, v + 0.1), at(t, u + 0.1, v + 0.5)
    return [[p, q, r, p]]


def far_line(t: Triple):
    return [at(t, -4.1, 2.2), at(t, -4.7, 2.6)]  # the first member of the MULTILINESTRING form: outside everything


def pass_rows(t: Triple, long: bool = False, multi: bool = False):
    """(A, B, line) of the pass figure.  long: A is the 48-coordinate ring; multi: MULTIPOLYGON / MULTILINESTRING rows with the figure
    as the second member"""
    A, B, line = polygon_row(t, long), pass_polygon(t), pass_line(t)
    return ([far_triangle(t, 0), A], [far_triangle(t, 1), B], [far_line(t), line]) if multi else (A, B, line)


SPIKE_X = (0.7, 0.3)  # the far point of the spike ring: 0.7 along the edge, 0.3 off it
LONG_ARC = 300  # arc points of the long spike ring: past SHORT_RING = 256 of gpk_seqedit.hip (the work-group kernel)


def _spike_ring(t: Triple, long: bool):
    side = 1.0 if t.sign >= 0 else -1.0  # (a collinear row: either side gives a ring that touches itself)
    X = at(t, SPIKE_X[0], SPIKE_X[1] * side)
    mid = []
    if long:  # a half ellipse from X to b that bulges away from a
        m, h = ((X[0] + t.b[0]) / 2, (X[1] + t.b[1]) / 2), ((X[0] - t.b[0]) / 2, (X[1] - t.b[1]) / 2)
        o = (0.5 * side * h[1], -0.5 * side * h[0])
        if (m[0] + o[0] - t.a[0]) ** 2 + (m[1] + o[1] - t.a[1]) ** 2 < (m[0] - o[0] - t.a[0]) ** 2 + (m[1] - o[1] - t.a[1]) ** 2:
            o = (-o[0], -o[1])
        th = [math.pi * (j + 1) / (LONG_ARC + 1) for j in range(LONG_ARC)]
        mid = [(m[0] + math.cos(x) * h[0] + math.sin(x) * o[0], m[1] + math.cos(x) * h[1] + math.sin(x) * o[1]) for x in th]
    return [t.a, t.c, X] + mid + [t.b, t.a]


@lru_cache(maxsize=None)
def spike_triple(t: Triple, long: bool = False) -> Triple:
    """t turned by a multiple of 90 degrees (exact; classes and kind stay) so that a is the lexicographically smallest coordinate of
    the spike ring by a margin: the directions from a to every other coordinate span less than 90 degrees, so one of the four quarter
    turns puts them all at a larger x.  tests/test_hard_orient.py asserts the placement with seqedit_ref.ring_turn"""
    for _ in range(4):
        ring = _spike_ring(t, long)
        L = math.hypot(t.b[0] - t.a[0], t.b[1] - t.a[1])
        if min(p[0] for p in ring[1:-1]) > t.a[0] + 0.02 * L:
            return t
        t = rot90(t)
    raise AssertionError(t)


def spike_row(t: Triple, long: bool = False):
    """POLYGON [a, c, X, b, a] around spike_triple(t), X far on c's side of a -> b: the triangle (c, X, b) with the spike a - c, whose
    returning edge b -> a passes c an ulp away.  The turn at the lexicographically smallest coordinate a is orient(b, a, c), the
    planted triple: c left of a -> b gives a clockwise ring, c right a counter-clockwise one, collinear a ring that touches itself
    (s == 0: gpk_orient_polygons copies it unchanged; for the clip an invalid row).  se::ring_turn of gpk_seqedit.h decides
    gpk_orient_polygons, pc::ring_sign of gpk_polyclip.h the sign of the ring when a box that contains it keeps it whole.
    long: LONG_ARC more coordinates between X and b (gpk_orient_polygons only)"""
    return [_spike_ring(spike_triple(t, long), long)]


def box_around(row, margin: float = 1.0):
    """POLYGON: a counter-clockwise box around every coordinate of the row, about `margin` times the row's larger extent away from it
    (another distance on every side: no corner in line with a diagonal of the row's own box)"""
    pts = [p for ring in row for p in ring]
    lo, hi = (min(p[0] for p in pts), min(p[1] for p in pts)), (max(p[0] for p in pts), max(p[1] for p in pts))
    m = margin * max(hi[0] - lo[0], hi[1] - lo[1])
    x0, y0, x1, y1 = lo[0] - m, lo[1] - 1.3 * m, hi[0] + 0.9 * m, hi[1] + 1.1 * m
    return [[(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]]


def nested_triple(t: Triple) -> Triple:
    """t, or t turned by 180 degrees (exact; classes and kind stay), whichever has c on the side of a -> b with the larger x — the
    side hole_row puts the shell on: no row is lost to a hole that lies outside its shell"""
    s = 1 if -(t.b[1] - t.a[1]) > 0 else -1  # +1: hole_row's shell is left of a -> b
    return t if t.sign * s >= 0 else rot180(t)


def nested_row(t: Triple, long: bool = False):
    """POLYGON hole_row(nested_triple(t)): the hole's lowest vertex c lies strictly inside the shell, an ulp from its edge ab (on it
    for a collinear row, which the clip is not given).  Intersected with a box that contains it, both rings are kept whole and the
    result is the row itself, one part of two rings: the hole finds its shell in pc::ring_encloses (gpk_polyclip.h), the crossing
    number of c against the shell, where only the edge ab is in doubt"""
    return hole_row(nested_triple(t), long)


def hinge_rows(t: Triple):
    """(P, Q): P = (a, b, r) and Q = (a, X, c), X far on the right of a -> b, both counter-clockwise and hinged at a.  c right of
    a -> b: they touch at a only; c left of it: X -> c crosses ab right before c and they overlap in the sliver (a, x, c); collinear:
    they share the stretch a - c of ab.  At a four arcs meet: pc::cw_before (gpk_polyclip.h, and the union's stitch in
    gpk_polyunion.h) orders a -> b against a -> c there, and the crossing test of X -> c against ab decides whether there is an overlap
    at all"""
    X = at(t, along(t) - 0.2, -0.5)
    return polygon_row(t), [[t.a, X, t.c, t.a]]


# ---- a fan of disjoint slivers for the point join -------------------------------------------------------------------------------------------
#
# A lean index with chains wants DISJOINT polygons, and a translation would destroy what makes a triple hard: the filter gives up only
# where an edge's extent is comparable with the magnitude of its coordinates (at an offset the differences are exact and the filter
# certain).  So the polygons stand around the origin like a fan: polygon i keeps to the middle half of its own angular sector, its
# planted edge a -> b runs outwards from radius 18 .. 22 to 45 .. 60, its apex r is at 55.  The two other sides are cut into short
# edges: 90 coordinates a ring, 4320 in all, which gives the index a raster of 256 x 256 cells of 0.47 — less than the 0.85 between
# neighbouring polygons at the inner radius, so that cells with two polygons (list cells) stay rare.

FAN_N, FAN_WIDE, FAN_RING = 48, 16.0, 90  # polygons; degrees of the first sector of every quadrant (interior cells); coordinates a ring


def fan_sectors():
    out = []
    per = FAN_N // 4
    narrow = (70.0 - FAN_WIDE) / (per - 1)
    for q in range(4):
        th = 90.0 * q + 10.0
        for j in range(per):
            w = FAN_WIDE if j == 0 else narrow
            out.append((math.radians(th), math.radians(w)))
            th += w
    return out


@lru_cache(maxsize=None)
def fan(seed: int = 104):
    """FAN_N triples with COMPOSITION, triple i inside sector i, and the apex r of its polygon"""
    rng = np.random.default_rng(seed)
    out = []
    for i, (th, w) in enumerate(fan_sectors()):
        want = COMPOSITION[i % len(COMPOSITION)]
        pol = lambda rho, f: (rho * math.cos(th + f * w), rho * math.sin(th + f * w))  # noqa: E731
        r = pol(55.0, 0.75)
        for _ in range(400000):
            a, b = pol(float(rng.uniform(18.0, 22.0)), float(rng.uniform(0.25, 0.4))), pol(float(rng.uniform(45.0, 60.0)), float(rng.uniform(0.25, 0.4)))
            if want == COLLINEAR:  # the wide-mantissa construction between these two ends
                a, b, c = _collinear(a, a, b, b, rng)
            elif want == EASY:  # 1 / 2000 of the edge off it: certain all the same, and still between its polygon's neighbours
                c = at(Triple(a, b, a, EASY), float(rng.uniform(T_LO, T_HI)), float(rng.choice([-0.0005, 0.0005])))
            else:
                c = _near(a, b, rng)
            if kind_of(a, b, c) == want:
                break
        else:
            raise AssertionError((i, want))
        t = Triple(a, b, c, want)
        assert exact(a, b, r) > 0 and only_planted_is_uncertain(t, [r])
        out.append((t, r))
    return tuple(out)


def _cut(p, q, k):
    """the k - 1 points that cut p -> q into k pieces (rounded: the side bends by ulps, the ring stays simple)"""
    return [(p[0] + (q[0] - p[0]) * j / k, p[1] + (q[1] - p[1]) * j / k) for j in range(1, k)]


def fan_polygons():
    """[a, b, 43 points to r, r, 43 points back to a, a]: the planted edge stays one long edge, every other edge is about a unit long"""
    k = (FAN_RING - 4) // 2 + 1
    out = []
    for t, r in fan():
        ring = [t.a, t.b] + _cut(t.b, r, k) + [r] + _cut(r, t.a, k) + [t.a]
        assert len(ring) == FAN_RING
        out.append([ring])
    return out


def fan_points(seed: int = 105):
    """the planted points, each polygon's centroid, and points spread over the fan's box"""
    rng = np.random.default_rng(seed)
    pts = [t.c for t, _ in fan()] + [((t.a[0] + t.b[0] + r[0]) / 3, (t.a[1] + t.b[1] + r[1]) / 3) for t, r in fan()]
    return pts + [tuple(p) for p in rng.uniform(-62.0, 62.0, (400, 2)).tolist()]


# ---- the stage-A sites of csrc ---------------------------------------------------------------------------------------------------------------


class FilterSite(NamedTuple):
    file: str
    function: str  # the function that holds the filter
    exact_arm: str  # what runs when the filter gives up
    reached_by: str  # the kernels that get there
    test: Optional[str]  # the GPU test that takes hard rows through it; None only for an exempt site (then `note` says why)
    note: str = ""
    exempt: bool = False


FILTER_SITES = [
    FilterSite("gpk_device.h", "orient2d", "orient2d_exact", "ring_edge (row-wise point in polygon, the generic walk of the point join), the relation "
               "masks, validity, hull, distance", f"{NEW}::test_rowwise_point_in_polygon",
               "also every relation, validity, hull and distance test of the file"),
    FilterSite("gpk_device.h", "ring_edge_inline", "orient2d_exact_unrolled", "nothing: chain_generic_row<INLINE_EXACT = true> (gpk_pipshared.h) is its "
               "only caller and is instantiated with false everywhere", None,
               "dead code: no kernel of the library contains it, so no input reaches it", exempt=True),
    FilterSite("gpk_device.h", "ring_edge_filtered", "`unsure`: the caller hands the point to the exact walk", "pip_tile_chain_kernel (gpk_join.hip), "
               "chains of more than four edges in the one-launch join", f"{NEW}::test_point_join_chain_kernel"),
    FilterSite("gpk_pipflow.hip", "ring_edge_flat", "`unsure`: flow_exact_pass walks the row", "pip_tile_flow_kernel, the one-launch point join",
               f"{NEW}::test_point_join_one_launch"),
    FilterSite("gpk_triangulate.h", "tri::orient", "tri::orient_exact", "gpk_triangulate on the device and in the host driver",
               f"{NEW}::test_triangulation"),
]


def counted_filter_sites() -> dict:
    """{source file: occurrences of the stage-A constant} over geopolars_amd/csrc, and the set of constants found"""
    out, found = {}, set()
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".h", ".cpp")):
            with open(os.path.join(CSRC, fn)) as f:
                hits = re.findall(r"\b3\.33066907387\d*e-16\b", f.read())
            if hits:
                out[fn] = len(hits)
                found.update(hits)
    return out, found


def inventory_filter_sites() -> dict:
    out = {}
    for s in FILTER_SITES:
        out[s.file] = out.get(s.file, 0) + 1
    return out


# ---- census ------------------------------------------------------------------------------------------------------------------------------------


def census(evaluations) -> dict:
    """{class: count} over (a, b, c) evaluations in the order given"""
    out = {"Z": 0, "F": 0, "U": 0, "W": 0}
    for a, b, c in evaluations:
        out[classify(a, b, c)] += 1
    return out


def ring_evaluations(ring, points):
    """what coord_pos_relative_to_ring evaluates: every edge whose closed y-range holds the point and whose closed x-range holds it"""
    for p in points:
        for s, e in zip(ring[:-1], ring[1:]):
            if min(s[1], e[1]) <= p[1] <= max(s[1], e[1]) and min(s[0], e[0]) <= p[0] <= max(s[0], e[0]) and tuple(s) != tuple(e):
                yield tuple(s), tuple(e), tuple(p)


# ---- rows for the references that work on integers ------------------------------------------------------------------------------------------


def integer_grid_scale(*rows) -> int:
    """the power of two on_integer_grid multiplies these rows by: a reference result on the grid, divided by it, is the result on the
    doubles (polyclip_ref.scaled_back, lineclip_ref.scaled_back)"""
    flat = []

    def walk(r):
        if isinstance(r, tuple) and len(r) == 2 and not isinstance(r[0], (tuple, list)):
            flat.extend(Fraction(float(v)) for v in r)
        else:
            for q in r:
                walk(q)

    for r in rows:
        walk(r)
    return max(f.denominator for f in flat)  # (denominators are powers of two)


def on_integer_grid(*rows):
    """the rows (nested lists of (x, y) doubles) with every coordinate multiplied by one power of two that makes all of them
    integers (Python ints): relation_ref and polyrel_ref take integer coordinates, and a common exact scale changes no relation"""
    den = integer_grid_scale(*rows)

    def conv(r):
        if isinstance(r, tuple) and len(r) == 2 and not isinstance(r[0], (tuple, list)):
            return (int(Fraction(float(r[0])) * den), int(Fraction(float(r[1])) * den))
        return [conv(q) for q in r]

    return [conv(r) for r in rows]
