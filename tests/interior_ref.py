"""Exact reference of gpk_representative_point (include/geopolars_hip.h) and the rows of its fixture
tests/golden/interior_lattice.npz.

Polygonal rows: scanY is a float computed by the stated rule (comparisons and one average of floats); the crossings, the sections and
their widths are `fractions.Fraction` values of the float coordinates.  Lineal and puntal rows: the centroid is the length-weighted one
(square roots carried to 50 digits, then taken as fractions: 1e-50 against a tolerance of 1e-9) or the exact mean, the squared distance
of every candidate vertex to it is a Fraction."""
import io
import math
import os
import zipfile
from fractions import Fraction

import numpy as np

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from tests import exact_ref as X

PT, MPT, LS, MLS, PG, MPG = (_abi.GEOM_POINT, _abi.GEOM_MULTIPOINT, _abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON,
                             _abi.GEOM_MULTIPOLYGON)
FAMILIES = {"pt": PT, "mpt": MPT, "ls": LS, "mls": MLS, "pg": PG, "mpg": MPG}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interior_lattice.npz")
OFFSET = (500000.0, 4500000.0)  # the georeferenced placement
PLACEMENTS = {"lattice": (0.0, 0.0), "georeferenced": OFFSET}
# csrc/gpk_interior.h
G_SMALL, G_LARGE, G_MEAN, BLOCK_COORDS, SLICE, LDS_CROSSINGS = 4, 16, 32.0, 512, 32, 2048
REL_TOL = 1e-9
MIN_REL_WIDTH = 1e-6  # rows whose exact widest width is at least this fraction of the diagonal carry the interior guarantee


# ---- the rules, exactly ----------------------------------------------------------------------------------------------------------------
def scan_y(rings) -> float:
    ys = [float(p[1]) for r in rings for p in r]
    lo, hi = min(ys), max(ys)
    centre = (lo + hi) / 2
    for y in ys:
        if y <= centre:
            if y > lo:
                lo = y
        elif y < hi:
            hi = y
    return (lo + hi) / 2


def member_sections(rings):
    """one non-empty member: {'scan': float, 'crossings': [(x, edge)], 'sections': [(x0, x1, width)]}, x exact"""
    scan = scan_y(rings)
    s = Fraction(scan)
    cross, e = [], 0
    for r in rings:
        for i in range(len(r) - 1):
            (x0, y0), (x1, y1) = (float(r[i][0]), float(r[i][1])), (float(r[i + 1][0]), float(r[i + 1][1]))
            counts = y0 != y1 and min(y0, y1) <= scan <= max(y0, y1) and not (y0 == scan and y1 < scan) and not (y1 == scan and y0 < scan)
            if counts:
                x = Fraction(x0) if x0 == x1 else Fraction(x0) + (s - Fraction(y0)) * (Fraction(x1) - Fraction(x0)) / (Fraction(y1) - Fraction(y0))
                cross.append((x, e + i))
        e += len(r)
    cross.sort()
    sections = [(cross[k][0], cross[k + 1][0], cross[k + 1][0] - cross[k][0]) for k in range(0, len(cross) - 1, 2)]
    return {"scan": scan, "crossings": cross, "sections": sections}


def live_members(kind, row):
    """the members of a polygonal row that count: with rings and a non-empty shell"""
    return [p for p in X.row_polys(kind, row) if len(p) and len(p[0])]


def polygon_row(kind, row):
    """{'members': [member_sections], 'max_width': Fraction, 'first': (x, y) floats or None (no coordinate), 'choice': (member, section)
    of the rule in exact arithmetic or None (degenerate)}"""
    members = [member_sections(p) for p in live_members(kind, row)]
    first = None
    for p in live_members(kind, row):
        first = (float(p[0][0][0]), float(p[0][0][1]))
        break
    best, choice = Fraction(0), None
    for m, mem in enumerate(members):
        for k, (_, _, w) in enumerate(mem["sections"]):
            if w > best:
                best, choice = w, (m, k)
    return {"members": members, "max_width": best, "first": first, "choice": choice}


def row_coords(kind, row):
    if kind == PT:
        return [] if row is None else [row]
    return [c for s in X.row_seqs(kind, row) for c in s]


def diagonal(kind, row) -> float:
    c = np.array(row_coords(kind, row), dtype=np.float64).reshape(-1, 2)
    return float(math.hypot(*(c.max(axis=0) - c.min(axis=0)))) if len(c) else 0.0


def ulp(v: float) -> float:
    return float(np.spacing(abs(v)))


def tolerance(kind, row) -> float:
    """1e-9 * (row box diagonal) + 4 ulp(max |x| of the row): the project's rule plus the rounding of the final addition at the
    coordinate's magnitude"""
    c = np.array(row_coords(kind, row), dtype=np.float64).reshape(-1, 2)
    return REL_TOL * diagonal(kind, row) + 4 * ulp(float(np.abs(c[:, 0]).max()))


def vertex_row(kind, row):
    """a lineal or puntal row: {'centroid': (Fraction, Fraction), 'candidates': [(x, y, d2)] in storage order — the interior vertices,
    the member end points when there is none, every member of a multipoint}; None for a row without a coordinate"""
    if kind in (PT, MPT):
        pts = row_coords(kind, row)
        if not pts:
            return None
        cx = sum(Fraction(float(p[0])) for p in pts) / len(pts)
        cy = sum(Fraction(float(p[1])) for p in pts) / len(pts)
        cand = pts
    else:
        seqs = [s for s in X.row_seqs(kind, row) if len(s)]
        if not seqs:
            return None
        tot = mx = my = 0
        for s in seqs:
            for a, b in zip(s[:-1], s[1:]):
                L = Fraction(X.segment_length(a, b))
                tot += L
                mx += L * (Fraction(float(a[0])) + Fraction(float(b[0]))) / 2
                my += L * (Fraction(float(a[1])) + Fraction(float(b[1]))) / 2
        if tot:
            cx, cy = mx / tot, my / tot
        else:  # every segment degenerate: geo's dimension-0 case, the start of every segment (a member of one coordinate: that one)
            k = [max(len(s) - 1, 1) for s in seqs]
            cx = sum(Fraction(float(s[0][0])) * w for s, w in zip(seqs, k)) / sum(k)
            cy = sum(Fraction(float(s[0][1])) * w for s, w in zip(seqs, k)) / sum(k)
        cand = [c for s in seqs for c in s[1:-1]] or [c for s in seqs for c in (s[0], s[-1])]
    out = [(float(x), float(y), (Fraction(float(x)) - cx) ** 2 + (Fraction(float(y)) - cy) ** 2) for x, y in cand]
    return {"centroid": (cx, cy), "candidates": out}


def finite_row(kind, row) -> bool:
    return bool(np.isfinite(np.array(row_coords(kind, row), dtype=np.float64)).all())


# ---- the checks every consumer of the fixture makes ---------------------------------------------------------------------------------------
def check_polygon_answer(kind, row, x, y, width=None):
    """the point (x, y) [and out_width] of a polygonal row with coordinates against the rules; returns the error as a fraction of tol
    (0.0 for a degenerate row, whose answer is bit-exact)"""
    ref = polygon_row(kind, row)
    if ref["choice"] is None:
        assert (x, y) == ref["first"], ("degenerate row: first coordinate", (x, y), ref["first"])
        assert width is None or width == 0.0, width
        return 0.0
    tol = Fraction(tolerance(kind, row))
    best = None
    for mem in ref["members"]:
        if y != mem["scan"]:
            continue
        for x0, x1, w in mem["sections"]:
            if w >= ref["max_width"] - tol:
                err = abs(Fraction(x) - (x0 + x1) / 2)
                werr = abs(Fraction(width) - w) if width is not None else Fraction(0)
                if werr <= 2 * tol and (best is None or err < best):
                    best = err
    assert best is not None, ("y is no member's scan line, or no widest section there", (x, y, width), [m["scan"] for m in ref["members"]])
    assert best <= tol, ("x off the midpoint of every widest section", float(best), float(tol))
    return float(best / tol)


def check_vertex_answer(kind, row, x, y):
    ref = vertex_row(kind, row)
    d2 = [d for cx, cy, d in ref["candidates"] if (cx, cy) == (x, y)]
    assert d2, ("not a candidate coordinate of the row (an interior vertex whenever one exists)", (x, y))
    bound = min(d for _, _, d in ref["candidates"]) + Fraction(REL_TOL * diagonal(kind, row) ** 2)
    assert min(d2) <= bound, ("not the nearest candidate", (x, y), float(min(d2)), float(bound))


# ---- shapes on the integer lattice (rings closed, as stored) ----------------------------------------------------------------------------------
def rect(x0, y0, x1, y1, cw=False):
    r = [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]
    return r[::-1] if cw else r


def comb(k, n_coords=None, wide=None):
    """a comb of k teeth standing on a base: the scan line crosses 2k edges.  Teeth are 1 wide (tooth `wide`: 2) and 2 apart; the ring
    runs along the base and back over the teeth from the right, so storage order is not x order.  n_coords: pad with vertices on the
    base to exactly that many coordinates."""
    xs, x = [], 0
    for t in range(k):
        w = 2 if t == wide else 1
        xs.append((x, x + w))
        x += w + 2
    W = xs[-1][1]
    ring = [(0, 0)]
    if n_coords is not None:
        pad = n_coords - (4 * k + 1)
        assert 0 <= pad < W, (k, n_coords)
        ring += [(i, 0) for i in range(1, pad + 1)]
    ring.append((W, 0))
    for t in range(k - 1, -1, -1):
        a, b = xs[t]
        ring += [(b, 10), (a, 10)] if t == k - 1 else [(b, 1), (b, 10), (a, 10)]
        if t > 0:
            ring.append((a, 1))
    ring.append((0, 0))
    assert n_coords is None or len(ring) == n_coords, (len(ring), n_coords)
    return ring


def pad_base(ring, n_coords):
    """the ring with vertices added on its first edge, which must be horizontal and lie at the ring's lowest ordinate (so that neither
    the scan line nor a crossing changes), up to exactly n_coords coordinates; the added abscissae are dyadic fractions"""
    (x0, y0), (x1, y1) = ring[0], ring[1]
    pad = n_coords - len(ring)
    assert y0 == y1 == min(p[1] for p in ring) and x0 != x1 and pad >= 0
    m = 1
    while m <= pad:
        m *= 2
    return [ring[0]] + [(x0 + (x1 - x0) * j / m, y0) for j in range(1, pad + 1)] + list(ring[1:])


TRI = [(0, 0), (4, 0), (0, 3), (0, 0)]
L_SHAPE = [(0, 0), (6, 0), (6, 2), (2, 2), (2, 6), (0, 6), (0, 0)]
U_SHAPE = [(0, 0), (6, 0), (6, 6), (4, 6), (4, 2), (2, 2), (2, 6), (0, 6), (0, 0)]
RING_SHAPE = [rect(0, 0, 10, 10), rect(3, 3, 7, 7, cw=True)]
COMB_TEETH = (1, 2, 3, 4, 8, 15, 16, 17, 31, 32, 33)  # around G / 2, G, and (2k and k) around the slice of 32
UP = 2.0**-30  # one ulp of the georeferenced ordinate 4500001


def holed(*holes):
    return [rect(0, 0, 20, 10)] + [rect(a, 2, b, 8, cw=True) for a, b in holes]


def polygon_rows():
    """(name, row) of the POLYGON column"""
    rows = [
        ("triangle", [TRI]), ("triangle_cw", [[(1, 1), (1, 5), (7, 1), (1, 1)]]),
        ("l_shape", [L_SHAPE]), ("u_shape", [U_SHAPE]), ("ring_shape", RING_SHAPE),
        ("hole1_widest_first", holed((12, 15))), ("hole1_widest_last", holed((3, 6))), ("hole2_widest_middle", holed((2, 4), (15, 17))),
        ("hole2_widest_first", holed((10, 12), (14, 16))), ("hole2_widest_last", holed((2, 4), (6, 8))),
        ("hole3_widest_last", holed((2, 3), (5, 6), (8, 9))), ("hole3_widest_middle", holed((2, 3), (12, 13), (16, 17))),
        ("hole3_widest_first", holed((9, 10), (12, 13), (16, 17))),
        ("vertex_at_centre", [[(0, 0), (4, 2), (0, 4), (-4, 2), (0, 0)]]),
        ("horizontal_at_centre", [[(0, 0), (6, 0), (6, 2), (4, 2), (4, 4), (0, 4), (0, 0)]]),
        ("adjacent_lattice", [[(0, 0), (6, 1), (3, 2), (-1, float(np.nextafter(1.0, 2.0))), (0, 0)]]),
        ("adjacent_georeferenced", [[(0, 0), (6, 1), (3, 2), (-1, 1 + UP), (0, 0)]]),
        ("flat_diagonal", [[(0, 0), (2, 2), (4, 4), (0, 0)]]), ("flat_horizontal", [[(0, 0), (5, 0), (2, 0), (0, 0)]]),
        ("flat_point", [[(1, 1), (1, 1), (1, 1), (1, 1)]]), ("flat_vertical", [[(3, 0), (3, 7), (3, 2), (3, 0)]]),
        ("empty", []),
    ]
    rows += [(f"comb_{k}", [comb(k)]) for k in COMB_TEETH]
    rows += [("comb_wide_17", [comb(17, wide=9)]), ("comb_wide_3", [comb(3, wide=2)])]
    rows += [("comb_513", [comb(100, n_coords=BLOCK_COORDS + 1, wide=40)]), ("comb_2048", [comb(400, n_coords=2048, wide=333)]),
             ("comb_512", [comb(100, n_coords=BLOCK_COORDS)])]
    # few crossings in many coordinates: the lane-group kernel ranks them at 512 coordinates, the work-group kernel sorts them beyond
    rows += [("u_shape_512", [pad_base(U_SHAPE, BLOCK_COORDS)]), ("u_shape_513", [pad_base(U_SHAPE, BLOCK_COORDS + 1)]),
             ("ring_shape_700", [pad_base(RING_SHAPE[0], 695), RING_SHAPE[1]])]
    return rows


def multipolygon_rows():
    sq = lambda x, w: [rect(x, 0, x + w, 4)]  # noqa: E731
    return [
        ("widest_first", [sq(0, 9), [], sq(20, 3), sq(30, 5)]), ("widest_middle", [sq(0, 2), [], sq(20, 8), [[]], sq(30, 5)]),
        ("widest_last", [[], sq(0, 2), sq(20, 3), [], sq(30, 7)]), ("equal_first_wins", [sq(0, 5), sq(20, 5)]),
        ("equal_after_narrow", [sq(0, 2), sq(10, 5), [], sq(20, 5)]), ("single", [[L_SHAPE]]), ("ring_and_comb", [RING_SHAPE, [comb(17)]]),
        ("comb_then_wide", [[comb(33)], sq(200, 3)]), ("flat_then_square", [[[(0, 0), (2, 2), (4, 4), (0, 0)]], sq(10, 2)]),
        ("only_empty_members", [[], [[]]]), ("empty", []), ("holed_members", [holed((3, 6)), [[(p[0] + 30, p[1]) for p in r] for r in holed((12, 15))]]),
        ("big_member", [sq(-20, 4), [comb(100, n_coords=600)]]),
    ]


def line_rows():
    return [
        ("two_point", [(0, 0), (4, 3)]), ("two_point_flat", [(2, 2), (2, 2)]), ("equidistant_first_wins", [(0, 0), (0, 2), (4, 2), (4, 0)]),
        ("closed", [(0, 0), (4, 0), (4, 4), (0, 4), (0, 0)]), ("zigzag", [(0, 0), (1, 5), (2, 0), (3, 5), (9, 0), (10, 5)]),
        ("hook", [(0, 0), (10, 0), (10, 1), (0, 1)]), ("long", [(i, (i * 7) % 5) for i in range(40)]),
        ("big", [(i, (i * 7) % 11) for i in range(BLOCK_COORDS + 88)]), ("empty", []),
        ("flat_three", [(3, 1), (3, 1), (3, 1)]),
    ]


def multiline_rows():
    return [
        ("no_interior", [[(0, 0), (1, 0)], [], [(5, 5), (6, 5)]]), ("interior_in_last", [[(0, 0), (10, 0)], [], [(0, 5), (3, 5), (10, 5)]]),
        ("interior_in_both", [[(0, 0), (2, 1), (4, 0)], [(0, 5), (2, 4), (4, 5)]]), ("single", [[(0, 0), (1, 1), (2, 0)]]),
        ("only_empty_members", [[], []]), ("empty", []), ("closed_and_open", [[(0, 0), (4, 0), (4, 4), (0, 0)], [(10, 10), (12, 10)]]),
        ("flat_members", [[(0, 0), (0, 0), (0, 0), (0, 0)], [], [(10, 0), (10, 0), (10, 0)], [(7, 7)]]),
        ("flat_member_ignored", [[(100, 100), (100, 100), (100, 100)], [(0, 0), (2, 0), (4, 0)]]),
    ]


def multipoint_rows():
    return [
        ("single", [(3, 4)]), ("duplicates", [(0, 0), (4, 0), (4, 0), (10, 10)]), ("tie_first_wins", [(0, 0), (2, 0), (0, 2), (2, 2)]),
        ("many", [((i * 37) % 101, (i * 53) % 89) for i in range(70)]), ("empty", []), ("all_equal", [(5, 5), (5, 5), (5, 5)]),
    ]


def point_rows():
    return [("a", (1, 2)), ("b", (-7, 30)), ("empty", None)]


ROWS = {"pg": polygon_rows, "mpg": multipolygon_rows, "ls": line_rows, "mls": multiline_rows, "mpt": multipoint_rows, "pt": point_rows}


def family_rows(fam):
    """(names, rows, validity) of a family's column: the rows above, then a null copy of the first row"""
    named = ROWS[fam]()
    names = [n for n, _ in named] + ["null"]
    rows = [r for _, r in named] + [named[0][1]]
    return names, rows, [True] * len(named) + [False]


# ---- columns <-> rows ------------------------------------------------------------------------------------------------------------------------
def column_rows(col: GeoArrowArray):
    """the rows of a column as nested lists of (x, y) float tuples"""
    xy = [tuple(map(float, p)) for p in col.xy]
    g, p, r, k = col.geom_offsets, col.part_offsets, col.ring_offsets, col.geom_type
    if k == PT:
        return [None if math.isnan(q[0]) else q for q in xy]
    if k in (MPT, LS):
        return [xy[g[i]:g[i + 1]] for i in range(col.n_geoms)]
    if k in (MLS, PG):
        return [[xy[r[j]:r[j + 1]] for j in range(g[i], g[i + 1])] for i in range(col.n_geoms)]
    return [[[xy[r[j]:r[j + 1]] for j in range(p[m], p[m + 1])] for m in range(g[i], g[i + 1])] for i in range(col.n_geoms)]


def fixture_column(z, fam, offset=(0.0, 0.0)) -> GeoArrowArray:
    """a family's column of the fixture, translated by `offset`, with its validity"""
    off = {name: (z[f"{fam}_{name}"] if len(z[f"{fam}_{name}"]) else None) for name in ("geom_offsets", "part_offsets", "ring_offsets")}
    valid = z[f"{fam}_valid"]
    return GeoArrowArray(FAMILIES[fam], z[f"{fam}_xy"] + np.asarray(offset, dtype=np.float64), validity=np.packbits(valid, bitorder="little"), **off)


def build_arrays():
    """every array of tests/golden/interior_lattice.npz: per family the column, its validity, the row names and — at the lattice
    placement — the reference's verdict (polygonal: scan line of the first member, crossings of the first member, the exact widest width
    as a float; others: the first nearest candidate)"""
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
        rows = column_rows(col)
        if kind in (PG, MPG):
            refs = [polygon_row(kind, r) for r in rows]
            out[f"{fam}_scan"] = np.array([ref["members"][0]["scan"] if ref["members"] else np.nan for ref in refs])
            out[f"{fam}_crossings"] = np.array([len(ref["members"][0]["crossings"]) if ref["members"] else -1 for ref in refs], dtype=np.int32)
            out[f"{fam}_width"] = np.array([float(ref["max_width"]) for ref in refs])
        else:
            ans = []
            for r in rows:
                ref = vertex_row(kind, r)
                if ref is None:
                    ans.append((np.nan, np.nan))
                else:
                    d = min(c[2] for c in ref["candidates"])
                    ans.append(next((c[0], c[1]) for c in ref["candidates"] if c[2] == d))
            out[f"{fam}_nearest"] = np.array(ans, dtype=np.float64).reshape(-1, 2)
    return out


def npz_bytes(arrays) -> bytes:
    """an .npz with fixed member dates: the same arrays give the same bytes"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as zf:
        for name in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, b.getvalue())
    return buf.getvalue()


def driver_records(col: GeoArrowArray) -> bytes:
    """the valid rows of a column as input records of tests/interior_host_driver.cpp: int32 kind, int32 n_parts, per part int32 n_seqs,
    per sequence int32 n_coords and the coordinates (a puntal or lineal row: one part; a point: one sequence of one coordinate)"""
    buf = io.BytesIO()
    k = col.geom_type
    for row in column_rows(col):
        if k == PT:
            parts = [[[] if row is None else [row]]]
        elif k in (MPT, LS):
            parts = [[row]]
        elif k in (MLS, PG):
            parts = [row]
        else:
            parts = row
        buf.write(np.int32(k).tobytes())
        buf.write(np.int32(len(parts)).tobytes())
        for seqs in parts:
            buf.write(np.int32(len(seqs)).tobytes())
            for s in seqs:
                buf.write(np.int32(len(s)).tobytes())
                buf.write(np.array(s, dtype=np.float64).reshape(-1, 2).tobytes())
    return buf.getvalue()
