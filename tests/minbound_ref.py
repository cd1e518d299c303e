"""Exact reference of gpk_minimum_rotated_rectangle and gpk_minimum_bounding_circle (include/geopolars_hip.h)
and the rows of their fixture tests/golden/minbound_lattice.npz.

A row's float coordinates are dyadic rationals: they are scaled by one power of two to Python integers, and everything — the hull
(monotone chain on exact orientations), the per-edge extents s = u . d and t = d x u, the areas A / L2, the smallest circle — is
integer or `fractions.Fraction` arithmetic on them.  The extents of an edge are vectorised in int64 where they fit; the three extremes
are then taken as Python ints."""
import functools
import math
import os
import random
from fractions import Fraction

import numpy as np

from tests import interior_ref as I

PT, MPT, LS, MLS, PG, MPG = I.PT, I.MPT, I.LS, I.MLS, I.PG, I.MPG
FAMILIES = I.FAMILIES
PLACEMENTS = I.PLACEMENTS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "minbound_lattice.npz")
REL_TOL = 1e-9
# csrc/gpk_minbound.h
G, SMALL_HULL, BIG_THREADS, BIG_BLOCKS, LDS_HULL = 16, 128, 256, 1024, 4096
CIRCLE_ITERS = 64  # include/geopolars_hip.h


# ---- exact geometry on integers -------------------------------------------------------------------------------------------------------
def scaled_ints(coords):
    """float (x, y) pairs -> (integer pairs, scale): x = X / scale exactly, scale a power of two"""
    scale = 1
    for p in coords:
        for v in p:
            scale = max(scale, Fraction(float(v)).denominator)
    return [(int(Fraction(float(x)) * scale), int(Fraction(float(y)) * scale)) for x, y in coords], scale


def hull_ring(pts):
    """the hull of integer points as gpk_convex_hull writes it: counter-clockwise from the lexicographically smallest vertex, no collinear
    vertices, closing vertex dropped (one distinct point: [p]; collinear: [p, q])"""
    p = sorted(set(pts))
    if len(p) <= 2:
        return p

    def half(seq):
        out = []
        for c in seq:
            while len(out) >= 2 and (out[-1][0] - out[-2][0]) * (c[1] - out[-2][1]) - (out[-1][1] - out[-2][1]) * (c[0] - out[-2][0]) <= 0:
                out.pop()
            out.append(c)
        return out

    lo, up = half(p), half(p[::-1])
    return lo[:-1] + up[:-1]


def edge_extents(h):
    """per edge i of the hull ring h (h >= 3 integer vertices): (smin, smax, tmax, L2) as Python ints"""
    n = len(h)
    span = max(max(abs(x - h[0][0]), abs(y - h[0][1])) for x, y in h)
    out = []
    if 16 * span * span < 2**62:  # every product and sum below fits int64
        v = np.array(h, dtype=np.int64)
        for i in range(n):
            a, d = v[i], v[(i + 1) % n] - v[i]
            u = v - a
            s = u[:, 0] * d[0] + u[:, 1] * d[1]
            t = d[0] * u[:, 1] - d[1] * u[:, 0]
            out.append((int(s.min()), int(s.max()), int(t.max()), int(d[0]) ** 2 + int(d[1]) ** 2))
    else:
        for i in range(n):
            (ax, ay), (bx, by) = h[i], h[(i + 1) % n]
            dx, dy = bx - ax, by - ay
            s = [(x - ax) * dx + (y - ay) * dy for x, y in h]
            t = [dx * (y - ay) - dy * (x - ax) for x, y in h]
            out.append((min(s), max(s), max(t), dx * dx + dy * dy))
    return out


def edge_rectangle(h, i, ext, scale):
    """the exact corners [(x, y)] * 4 (Fractions, unscaled) of the rectangle on edge i"""
    (ax, ay), (bx, by) = h[i], h[(i + 1) % len(h)]
    dx, dy = bx - ax, by - ay
    smin, smax, tmax, L2 = ext
    lo, hi, up = Fraction(smin, L2), Fraction(smax, L2), Fraction(tmax, L2)
    c0 = (ax + lo * dx, ay + lo * dy)
    c1 = (ax + hi * dx, ay + hi * dy)
    c2 = (c1[0] - up * dy, c1[1] + up * dx)
    c3 = (c0[0] - up * dy, c0[1] + up * dx)
    return [(x / scale, y / scale) for x, y in (c0, c1, c2, c3)]


# circles on integers: centre (X / D, Y / D), squared radius R / D^2, D > 0
def _c1(p):
    return (p[0], p[1], 1, 0)


def _c2(p, q):
    return (p[0] + q[0], p[1] + q[1], 2, (p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2)


def _c3(a, b, c):
    ex, ey, fx, fy = b[0] - a[0], b[1] - a[1], c[0] - a[0], c[1] - a[1]
    D = 2 * (ex * fy - ey * fx)
    if D == 0:
        return None
    e2, f2 = ex * ex + ey * ey, fx * fx + fy * fy
    nx, ny = fy * e2 - ey * f2, ex * f2 - fx * e2
    if D < 0:
        D, nx, ny = -D, -nx, -ny
    return (a[0] * D + nx, a[1] * D + ny, D, nx * nx + ny * ny)


def _inside(c, p):
    X, Y, D, R = c
    return (p[0] * D - X) ** 2 + (p[1] * D - Y) ** 2 <= R


def _r2(c):
    return Fraction(c[3], c[2] * c[2])


def smallest_circle(pts):
    """Welzl's randomized incremental algorithm with move-to-front on the outer level, exact: (X, Y, D, R) of the smallest circle of
    the integer points (the order is a seeded shuffle: the circle is unique, the order only decides the running time)"""
    P = list(dict.fromkeys(pts))
    random.Random(12345).shuffle(P)
    c = None
    for i in range(len(P)):
        p = P[i]
        if c is not None and _inside(c, p):
            continue
        c = _c1(p)
        for j in range(i):
            q = P[j]
            if _inside(c, q):
                continue
            c = _c2(p, q)
            for k in range(j):
                r = P[k]
                if not _inside(c, r):
                    c = _c3(p, q, r)
        P.insert(0, P.pop(i))  # move to front: a point that decided once tends to decide again
    return c


def smallest_circle_brute(pts):
    """the smallest among the circles on one, two or three of the points that contain all of them (a cross-check for few points)"""
    P = list(dict.fromkeys(pts))
    cands = [_c1(p) for p in P] + [_c2(p, q) for i, p in enumerate(P) for q in P[:i]]
    cands += [c for i, p in enumerate(P) for j, q in enumerate(P[:i]) for r in P[:j] for c in [_c3(p, q, r)] if c is not None]
    ok = [c for c in cands if all(_inside(c, p) for p in P)]
    return min(ok, key=_r2)


def exact_sqrt(fr: Fraction) -> Fraction:
    """sqrt of a non-negative Fraction to 2^-100 relative"""
    if fr == 0:
        return Fraction(0)
    k = 200 + 2 * max(0, fr.denominator.bit_length() - fr.numerator.bit_length())
    return Fraction(math.isqrt((fr.numerator << k) // fr.denominator), 1 << (k // 2))


# ---- one row ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _row_reference(coords):
    pts, scale = scaled_ints(coords)
    h = hull_ring(pts)
    ref = {"scale": scale, "hull": h}
    if len(h) >= 3:
        ext = edge_extents(h)
        areas = [Fraction((smax - smin) * tmax, L2) / (scale * scale) for smin, smax, tmax, L2 in ext]
        ref.update(ext=ext, areas=areas, min_area=min(areas), best_edge=areas.index(min(areas)))
    c = smallest_circle(h)
    if len(h) <= 12:
        assert _r2(c) == _r2(smallest_circle_brute(h)) and (c[0] * smallest_circle_brute(h)[2], c[1] * smallest_circle_brute(h)[2]) == (
            smallest_circle_brute(h)[0] * c[2], smallest_circle_brute(h)[1] * c[2]), "Welzl and brute force disagree"
    assert all(_inside(c, p) for p in h)
    ref["centre"] = (Fraction(c[0], c[2]) / scale, Fraction(c[1], c[2]) / scale)
    ref["r2"] = _r2(c) / (scale * scale)
    ref["radius"] = exact_sqrt(ref["r2"])
    return ref


def row_reference(coords):
    """the exact verdict on a row's float coordinates [(x, y)] (at least one, all finite): {'hull': integer ring, 'scale', 'ext',
    'areas' (Fractions, per edge), 'min_area', 'best_edge' (lowest index of the least area), 'centre', 'r2', 'radius'}"""
    return _row_reference(tuple(sorted({(float(x), float(y)) for x, y in coords})))  # (a row is its set of coordinates)


def tolerance(coords) -> float:
    """1e-9 * (row box diagonal) + 4 ulp(max |coordinate| of the row): the project's bound for representative_point"""
    c = np.array(coords, dtype=np.float64).reshape(-1, 2)
    return REL_TOL * float(math.hypot(*(c.max(axis=0) - c.min(axis=0)))) + 4 * I.ulp(float(np.abs(c).max()))


def ring_signed_area2(ring) -> Fraction:
    r = [(Fraction(float(x)), Fraction(float(y))) for x, y in ring]
    return sum(r[k][0] * r[k + 1][1] - r[k + 1][0] * r[k][1] for k in range(len(r) - 1))


def check_rectangle(coords, ring) -> float:
    """the acceptance of one rectangle answer `ring` (5 float pairs) for the row `coords`; returns the corner error as a share of tol"""
    ring = [(float(x), float(y)) for x, y in ring]
    assert len(ring) == 5 and ring[4] == ring[0], ("the fifth coordinate is the first bit for bit", ring)
    assert ring_signed_area2(ring) >= 0, ("the ring is counter-clockwise", ring)
    ref = row_reference(coords)
    h, scale = ref["hull"], ref["scale"]
    if len(h) <= 2:
        p, q = (h[0][0] / scale, h[0][1] / scale), (h[-1][0] / scale, h[-1][1] / scale)
        assert ring == [p, q, q, p, p], ("degenerate row", ring, [p, q, q, p, p])
        return 0.0
    tol = Fraction(tolerance(coords))
    got = [(Fraction(x), Fraction(y)) for x, y in ring[:4]]
    best = None
    for j, area in enumerate(ref["areas"]):
        smin, smax, tmax, L2 = ref["ext"][j]
        perimeter = Fraction(2 * ((smax - smin) + tmax) / math.sqrt(L2)) / scale
        if area > ref["min_area"] * (1 + Fraction(REL_TOL)) + tol * perimeter:
            continue
        want = edge_rectangle(h, j, ref["ext"][j], scale)
        err2 = max((g[0] - w[0]) ** 2 + (g[1] - w[1]) ** 2 for g, w in zip(got, want))
        if best is None or err2 < best:
            best = err2
    assert best is not None and best <= tol * tol, ("no edge of (nearly) least area has its rectangle within tol of the answer", ring,
                                                    None if best is None else math.sqrt(float(best)), float(tol))
    return math.sqrt(float(best)) / float(tol)


def check_circle(coords, cx, cy, radius) -> float:
    """the acceptance of one circle answer; returns the worst of the centre and radius errors as a share of tol (cx, cy None: radius only)"""
    ref = row_reference(coords)
    tol = Fraction(tolerance(coords))
    err = abs(Fraction(float(radius)) - ref["radius"])
    if cx is not None:
        err = max(err, abs(Fraction(float(cx)) - ref["centre"][0]), abs(Fraction(float(cy)) - ref["centre"][1]))
        reach = (Fraction(float(radius)) + tol) ** 2
        for x, y in ref["hull"]:  # (the hull vertices are the row's farthest coordinates from any centre)
            d2 = (Fraction(x, ref["scale"]) - Fraction(float(cx))) ** 2 + (Fraction(y, ref["scale"]) - Fraction(float(cy))) ** 2
            assert d2 <= reach, ("a coordinate of the row lies outside radius + tol", (x / ref["scale"], y / ref["scale"]))
    assert err <= tol, ("centre or radius off the exact circle", (cx, cy, radius), [float(v) for v in ref["centre"]], float(ref["radius"]), float(tol))
    return float(err / tol)


def row_coords(kind, row):
    return I.row_coords(kind, row)


def has_answer(kind, row) -> bool:
    c = row_coords(kind, row)
    return len(c) > 0 and bool(np.isfinite(np.array(c, dtype=np.float64)).all())


# ---- the fixture's point sets (integer lattice) ---------------------------------------------------------------------------------------------
def parabola(n):
    """n lattice points in convex position, exact"""
    return [(i, i * i) for i in range(n)]


CIRCLE5 = [(5, 0), (4, 3), (3, 4), (0, 5), (-3, 4), (-4, 3), (-5, 0), (-4, -3), (-3, -4), (0, -5), (3, -4), (4, -3)]
IN_TRIANGLE = [(0, 0), (1000, 0), (0, 1000)] + [((i * 37) % 300 + 1, (i * 53) % 300 + 1) for i in range(597)]
CONVEX_SIZES = (G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 64, 65, 127, 128, 129, 257, 600, LDS_HULL + 1)


def point_sets():
    """(name, points): the rows every family with several coordinates holds"""
    sets = [
        ("rect_axis", [(0, 0), (6, 0), (6, 3), (0, 3)]), ("diamond", [(0, 2), (2, 0), (4, 2), (2, 4)]),
        ("triangle_acute", [(0, 0), (4, 0), (1, 3)]), ("triangle_obtuse", [(0, 0), (6, 0), (1, 1)]), ("triangle_right", [(0, 0), (4, 0), (0, 3)]),
        ("square_interior", [(0, 0), (4, 0), (4, 4), (0, 4), (1, 1), (2, 3), (3, 2), (2, 2)]), ("circle5", CIRCLE5),
        ("sliver", [(0, 0), (997, 1), (2000, 3), (1003, 2)]), ("collinear", [(0, 0), (2, 2), (4, 4), (1, 1)]), ("two_points", [(1, 2), (7, 10)]),
        ("single", [(3, 4)]), ("repeated", [(5, 5), (5, 5), (5, 5)]), ("start_not_min", [(4, 3), (1, 5), (0, 0), (4, 0)]),
        ("in_triangle_600", IN_TRIANGLE),
    ]
    sets += [(f"convex_{n}", parabola(n)) for n in CONVEX_SIZES]
    return sets


def closed(pts):
    return list(pts) + [pts[0]]


def family_rows(fam):
    """(names, rows, validity) of a family's column: the point sets in the family's form, the family's own rows, an empty row, then a null
    copy of the first row"""
    if fam == "pt":
        named = [("a", (1, 2)), ("b", (-7, 30)), ("empty", None)]
    else:
        named = []
        for name, pts in point_sets():
            k = (len(pts) + 1) // 2
            if fam in ("mpt", "ls"):
                row = list(pts)
            elif fam == "mls":
                row = [pts[:k], [], pts[k:]] if len(pts) > 1 else [pts, []]
            elif fam == "pg":
                row = [closed(pts)]
            else:
                row = [[closed(pts[:k])], [], [closed(pts[k:])]] if len(pts) > 1 else [[closed(pts)], []]
            named.append((name, row))
        if fam == "pg":
            # the duplicate closing vertex is the lexicographic minimum; a hole wider than nothing contributes only points
            named.append(("closing_is_min", [[(0, 0), (4, 0), (4, 3), (1, 5), (0, 0)]]))
            named.append(("holed", [I.rect(0, 0, 10, 8), I.rect(2, 2, 8, 6, cw=True)]))
        if fam == "mpg":
            named.append(("holed_and_empty", [[I.rect(0, 0, 10, 8), I.rect(2, 2, 8, 6, cw=True)], [], [[(20, 1), (23, 1), (21, 9), (20, 1)]]]))
            named.append(("only_empty_members", [[], [[]]]))
        if fam == "mls":
            named.append(("only_empty_members", [[], []]))
        named.append(("empty", []))
    names = [n for n, _ in named] + ["null"]
    rows = [r for _, r in named] + [named[0][1]]
    return names, rows, [True] * len(named) + [False]


def build_arrays():
    """every array of tests/golden/minbound_lattice.npz: per family the column, its validity, the row names and — at the lattice
    placement — the reference's verdict (hull size, the lowest edge of least area, the least area, the circle's centre and radius as the
    floats nearest to the exact values; -1 / NaN for a row without an answer)"""
    from tests import exact_ref as X

    out = {}
    for fam, kind in FAMILIES.items():
        names, rows, valid = family_rows(fam)
        col = X.column(kind, rows)
        out[f"{fam}_xy"] = col.xy
        for name in ("geom_offsets", "part_offsets", "ring_offsets"):
            v = getattr(col, name)
            out[f"{fam}_{name}"] = np.zeros(0, dtype=np.int32) if v is None else np.asarray(v, dtype=np.int32)
        out[f"{fam}_valid"] = np.array(valid, dtype=bool)
        out[f"{fam}_names"] = np.array(names)
        hull, edge, area, circle = [], [], [], []
        for row, ok in zip(I.column_rows(col), valid):
            if not ok or not has_answer(kind, row):
                hull.append(-1), edge.append(-1), area.append(np.nan), circle.append((np.nan, np.nan, np.nan))
                continue
            ref = row_reference(row_coords(kind, row))
            hull.append(len(ref["hull"]))
            edge.append(ref.get("best_edge", -1))
            area.append(float(ref.get("min_area", 0)))
            circle.append((float(ref["centre"][0]), float(ref["centre"][1]), float(ref["radius"])))
        out[f"{fam}_hull_size"] = np.array(hull, dtype=np.int32)
        out[f"{fam}_best_edge"] = np.array(edge, dtype=np.int32)
        out[f"{fam}_min_area"] = np.array(area, dtype=np.float64)
        out[f"{fam}_circle"] = np.array(circle, dtype=np.float64).reshape(-1, 3)
    return out


npz_bytes = I.npz_bytes
fixture_column = I.fixture_column
column_rows = I.column_rows


def hull_floats(coords):
    """the exact hull ring of float coordinates, as floats (hull vertices are input coordinates: the conversion back is exact)"""
    ref = row_reference(coords)
    return [(x / ref["scale"], y / ref["scale"]) for x, y in ref["hull"]]


def driver_records(col) -> bytes:
    """the rows of a column as input records of tests/minbound_host_driver.cpp: int32 n_coords (-1: a null row), the coordinates,
    int32 h, the exact hull ring (h = 0 for a row without an answer)"""
    import io

    buf = io.BytesIO()
    for ok, row in zip(col.is_valid(), column_rows(col)):
        c = np.array(row_coords(col.geom_type, row), dtype=np.float64).reshape(-1, 2)
        buf.write(np.int32(len(c) if ok else -1).tobytes())
        if ok:
            buf.write(c.tobytes())
        hull = hull_floats([tuple(p) for p in c]) if ok and len(c) and np.isfinite(c).all() else []
        buf.write(np.int32(len(hull)).tobytes())
        buf.write(np.array(hull, dtype=np.float64).reshape(-1, 2).tobytes())
    return buf.getvalue()


def sweep_rows(n_rows=2000, seed=20240611):
    """the random sweep: rows of 3 .. 40 points, doubles not integers, at the georeferenced placement"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n_rows):
        k = int(rng.integers(3, 41))
        scale = 10.0 ** rng.uniform(-2, 3)
        pts = rng.normal(size=(k, 2)) * scale * np.array([1.0, 10.0 ** rng.uniform(-1.5, 0)]) + np.array(I.OFFSET)
        rows.append([(float(x), float(y)) for x, y in pts])
    return rows


def hard_rows():
    """(name, row) of double rows whose hull has more than 128 vertices and is no parabola — they take the work-group kernel:
    ulp_circle_*   300 random points on the circle of radius 100 about the origin, each followed by 0 .. 3 copies moved one ulp on along the
                   tangent: neighbouring hull vertices whose projections round to the same value (hulls of about 300 vertices: two
                   edges a thread, the calipers advance across the ulp-adjacent vertices); *_wide: 900 points, four edges a thread;
    ellipse_*      rotated ellipses of 200 and 700 points, translated;
    arcs           a scalene acute triangle on a circle and 300 points on a concentric circle of 0.97 of its radius: the smallest circle
                   has the triangle as its three-point support and is reached after at least two steps."""
    rows = []
    for seed, n in [(s, 300) for s in range(10)] + [(100, 900), (101, 900)]:
        rng = np.random.default_rng(seed)
        pts = []
        for t in np.sort(rng.uniform(0, 2 * np.pi, n)):
            x, y = 100.0 * math.cos(t), 100.0 * math.sin(t)
            pts.append((x, y))
            for _ in range(int(rng.integers(0, 4))):
                x, y = float(np.nextafter(x, x - math.sin(t) * 1e9)), float(np.nextafter(y, y + math.cos(t) * 1e9))
                pts.append((x, y))
        rows.append((f"ulp_circle_{seed}" + ("_wide" if n > 300 else ""), pts))
    for name, n, a, b, rot, off in (("ellipse_200", 200, 31.7, 12.9, 0.4, (3.25, -7.5)), ("ellipse_700", 700, 1234.5, 77.7, 2.1, I.OFFSET)):
        t = 2 * np.pi * (np.arange(n) + 0.123) / n
        x, y = a * np.cos(t), b * np.sin(t)
        rows.append((name, [(float(u), float(v)) for u, v in zip(off[0] + x * math.cos(rot) - y * math.sin(rot), off[1] + x * math.sin(rot) + y * math.cos(rot))]))
    cx, cy, R = 3.0, -2.0, 50.0
    tri = [(cx + R * math.cos(t), cy + R * math.sin(t)) for t in (0.3, 2.2, 4.4)]
    ring = [(cx + 0.97 * R * math.cos(t), cy + 0.97 * R * math.sin(t)) for t in 2 * np.pi * np.arange(300) / 300]
    rows.append(("arcs", tri + [(float(x), float(y)) for x, y in ring]))
    return rows
