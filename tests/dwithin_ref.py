"""Exact reference of the within-distance join (gpk_dwithin_join / gpk_dwithin_rowwise) and the fixtures its GPU tests use.

Rows are described as in exact_ref: (kind, rows, validity).  A pair (l, r) is within t iff both rows are usable (valid, at least one
coordinate, no NaN coordinate) and the exact squared distance, a Fraction, is <= t^2.  The exact distance of a pair comes from
exact_ref.exact_row_distance2 when a side is a POINT and from pair_distance_ref.distance2 otherwise.

`classify` also reports, per threshold, the pairs that are "too close to call": pairs whose exact distance d lies within the distance
routines' a-priori bound (exact_ref.distance_bound(d, lmax) = the bound of pair_distance_ref.check) of the threshold.  Two non-point
rows are never too close to t = 0 (`exact_zero`): their distance contract returns 0.0 exactly when the closed sets meet and a positive
double when they do not.  The point kernels restate geo's tolerance on "the point lies on the line", so a point within the bound of a
line counts as too close like any other pair.  The GPU tests rely on that list being empty for every committed fixture and threshold
(tests/test_dwithin_ref.py proves it), so they compare pair sets exactly and leave nothing out."""
from fractions import Fraction

import numpy as np

from geopolars_amd import _abi
from tests import exact_ref as X
from tests import pair_distance_ref as R

PT = _abi.GEOM_POINT
MP, LS, MLS, PG, MPG = _abi.GEOM_MULTIPOINT, _abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON
NONPOINT = [MP, LS, MLS, PG, MPG]
LARGE_COST = 1 << 16  # gpk_pairdist.h PD_LARGE_COST


def row_usable(kind, row, valid=True) -> bool:
    """valid, with a coordinate, and — POINT rows — without a NaN coordinate"""
    if not valid or row is None:
        return False
    if kind == PT:
        return not (np.isnan(row[0]) or np.isnan(row[1]))
    return sum(len(s) for s in X.row_seqs(kind, row)) > 0


def pair_distance2(ka, ra, kb, rb):
    """(exact squared distance as a Fraction, longest segment of the pair) of two usable rows of any two families"""
    if ka == PT:
        d2, _ = X.exact_row_distance2(ra, kb, rb)
        return d2, X.row_lmax(kb, rb)
    if kb == PT:
        d2, _ = X.exact_row_distance2(rb, ka, ra)
        return d2, X.row_lmax(ka, ra)
    return R.distance2(ka, ra, kb, rb), max(R.lmax(ka, ra), R.lmax(kb, rb))


def exact_table(left, right):
    """{(l, r): (d2 Fraction, lmax)} for every pair of usable rows — brute force"""
    ka, rows_a, va = left
    kb, rows_b, vb = right
    ua = [row_usable(ka, r, va is None or va[i]) for i, r in enumerate(rows_a)]
    ub = [row_usable(kb, r, vb is None or vb[j]) for j, r in enumerate(rows_b)]
    return {(l, r): pair_distance2(ka, rows_a[l], kb, rows_b[r]) for l in range(len(rows_a)) if ua[l] for r in range(len(rows_b)) if ub[r]}


def classify(table, t: float, exact_zero: bool = False):
    """(sorted pairs within t, pairs too close to call) from an exact_table; exact_zero: the table is of two non-point columns"""
    t2 = Fraction(float(t)) ** 2
    within, close = [], []
    for key, (d2, lmax) in table.items():
        if d2 <= t2:
            within.append(key)
        if d2 != 0 and not (exact_zero and t == 0):
            d = X.dec_sqrt(d2)
            if X.abs_err(float(t), d) <= X.distance_bound(float(d), lmax):
                close.append(key)
    return sorted(within), close


def dwithin_exact(left, right, t: float):
    """sorted (l, r) pairs of the exact within-distance join"""
    return classify(exact_table(left, right), t)[0]


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
# Thresholds of the exact comparison are fixed numbers (the CPU test must know them); DOMAIN is 1000 for the point fixtures and the
# non-point fixtures spread over a few hundred units.
THRESHOLDS = [0.0, 7.5, 60.0, 400.0]
N_POINTS_LEFT, N_ROWS_RIGHT = 24, 40  # point x family: the first rows of exact_ref.instance_fixture
N_ROWS_LEFT, N_POINTS_RIGHT = 20, 30  # family x point


def point_fixture(family: str, G: int, point_left: bool):
    """(left, right) columns as (kind, rows, validity): the POINT side from the instance fixture's query points, the other side its
    first rows (null, empty, dyadic and duplicated rows included)"""
    fx = X.instance_fixture(family, G)
    pts = [tuple(map(float, p)) for p in fx["left"][:140]]  # (the uniform ones)
    n = min(N_ROWS_RIGHT if point_left else N_ROWS_LEFT, len(fx["rows"]))
    # queries aimed at the kept rows first: vertices, hole centres and points exactly on dyadic edges (the fixture's queries one ulp off
    # a vertex are left out: they are within the bound of threshold 0 by construction)
    aimed = [tuple(map(float, fx["queries"][i])) for i in range(n) if i % 6 in (1, 2)]
    aimed += [tuple(map(float, fx["meta"][i]["edge"])) for i in range(n) if fx["meta"][i]["edge"] is not None and fx["usable"][i]]
    if point_left:
        return (PT, (aimed + pts)[:N_POINTS_LEFT], None), (fx["kind"], fx["rows"][:n], fx["validity"][:n])
    return (fx["kind"], fx["rows"][:n], fx["validity"][:n]), (PT, (aimed + pts)[:N_POINTS_RIGHT], None)


POINT_FIXTURES = [(f, g, pl) for f, g in X.INSTANCES for pl in (True, False) if not (f == "point" and not pl)]


def _make_row(kind, rng, cx, cy, size, nv):
    """a row of `kind` with about nv coordinates around (cx, cy) of extent ~size (the generator style of test_gpu_distance_pairs)"""
    if kind == MP:
        return [tuple(p) for p in np.stack([cx + rng.uniform(-size, size, nv) / 2, cy + rng.uniform(-size, size, nv) / 2], axis=1)]
    if kind == LS:
        t = np.linspace(-0.5, 0.5, nv)
        return [tuple(p) for p in np.stack([cx + size * t, cy + size * 0.3 * np.sin(7 * t) + rng.uniform(-0.02, 0.02, nv) * size], axis=1)]
    if kind == MLS:
        return [_make_row(LS, rng, cx + (i - 0.5) * size * 0.2, cy + (i - 0.5) * size * 0.3, size * 0.8, max(1, nv // 2)) for i in range(2)]
    if kind == PG:
        return [X._star(rng, cx, cy, size, max(3, nv - 6)), X._star(rng, cx, cy, size * 0.15, 4, cw=True)]
    return [_make_row(PG, rng, cx - size * 0.3, cy, size * 0.5, max(4, nv // 2)), [X._star(rng, cx + size * 0.4, cy, size * 0.3, max(3, nv // 2 - 1))]]


PAIR_SIZES = {"g8": (12, 9, 9, 11), "g32": (160, 140, 5, 6), "large": (320, 280, 3, 4)}  # coordinates per row (a, b), rows (left, right)


def pair_fixture(ka: int, kb: int, size: str, seed: int = 0):
    """(left, right) non-point columns: rows scattered over a square a few row sizes wide — overlapping, near and far pairs — with a
    null and an empty row on each side"""
    nva, nvb, nl, nr = PAIR_SIZES[size]
    rng = np.random.default_rng(1234 + seed + 97 * ka + 13 * kb + nva)
    span, rsize = 260.0, 40.0
    ra = [_make_row(ka, rng, *rng.uniform(0, span, 2), rsize, nva) for _ in range(nl)]
    rb = [_make_row(kb, rng, *rng.uniform(0, span, 2), rsize, nvb) for _ in range(nr)]
    va, vb = [True] * nl, [True] * nr
    if size == "g8":
        ra[2], va[4] = [], False
        rb[3], vb[1] = [], False
    return (ka, ra, va), (kb, rb, vb)


# every ordered pair of non-point families at every size: the 8-lane and 32-lane group kernels and the work-group schedule
PAIR_INSTANCES = [(ka, kb, s) for s in PAIR_SIZES for ka in NONPOINT for kb in NONPOINT]
PAIR_FIXTURES = PAIR_INSTANCES  # all of them are held against the exact reference too


def margin_cases(n: int = 6, t: float = 4.1, seed: int = 5):
    """(t, [(a, b)]): doubles with fl(b - a) == t although fl(a + t) < b — a is negative and b lies in a lower binade than t, so the
    difference rounds down onto t while the sum rounds below b.  A pair of geometries whose nearest coordinates are a and b on one axis
    has the computed distance t, and a left box grown by exactly t stops one ulp short of the right box."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        a = float(-rng.uniform(2.2, 3.0))
        b = float(np.nextafter(a + t, np.inf))
        if a + t < b < 2.0 and b - t > a and b - a == t and Fraction(b) - Fraction(a) > Fraction(t):
            out.append((a, b))
    return t, out

_TABLES = {}


def fixture_table(key):
    """exact_table of a POINT_FIXTURES / PAIR_FIXTURES entry, cached per process"""
    if key not in _TABLES:
        left, right = point_fixture(*key) if isinstance(key[0], str) else pair_fixture(*key)
        _TABLES[key] = exact_table(left, right)
    return _TABLES[key]


def columns(left, right):
    return X.column(*left), X.column(*right)
