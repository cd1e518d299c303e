"""The HIP path at georeferenced magnitudes against exact answers (tests/exact_ref.py).

Near the origin a kernel that drops the shift of geo's area / centroid sums (every ring shifted by its first coordinate), or borrows
a neighbouring ring's, stays within 1e-9 of the oracle; at UTM / Web Mercator magnitudes with metre-scale features it breaks the
a-priori error bounds of exact_ref by orders of magnitude (test_oracle_georeferenced.py shows the bounds separate the two on every
fixture).  Here every shift site is held to those bounds:

  * area / signed area / length / bounds through both forms (GPK_RING_STREAM=1, =0 and the product's choice, each its own
    interpreter): every size class, the 8192-coordinate chunks, rings across 512-coordinate windows and 1024-coordinate strips, a
    column of exactly 2048 coordinates that ends in empty and null rows with an empty geometry at a strip base; integer rings of
    every class length at +-2^30 (area bit for bit the untranslated one);
  * centroid: every class, long chunks, multipolygons with holes (the bound relative to the feature's extent), zero-area rings;
  * row-wise distance (per-row and the grouped row-map schedule) and contains / within / intersects for points on edges, on
    vertices and 1 - 2 ulps off them; the point-in-polygon join (one-launch flow and GPK_TILE_KERNEL=chain), the polygon x polygon
    joins on the lattice goldens; hulls of near-collinear sets; the nearest join with exact ties on a binary grid;
  * exact power-of-two scaling of every op, 2^k for k in +-7, +-30, +-60, +-100 (inside the range stated in
    include/geopolars_hip.h)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries

from . import exact_ref as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_FORMS_PROG = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from oracle import pyoracle as oracle
from tests import exact_ref as X
oracle.build(); oracle.lib()

def rel_close(got, exp, name):
    m = ~np.isnan(exp)
    assert np.array_equal(np.isnan(got), np.isnan(exp)), name
    bad = np.abs(got[m] - exp[m]) > 1e-9 * np.maximum(np.abs(exp[m]), 1e-300)
    assert not bad.any(), (name, np.nonzero(bad)[0][:5])

fx = X.area_fixtures()
fx["buildings_polygon"] = ([g[:1] for g in fx["buildings"][0]], None)
for name, (geoms, valid) in fx.items():
    a = X.to_polygon_array(geoms) if name.endswith("_polygon") else X.to_array(geoms, valid)
    s = GeoSeries(a)
    for signed in (False, True):
        got = np.asarray(s.signed_area() if signed else s.area())
        rel_close(got, oracle.area(a, signed=signed), (name, signed))
        ex, bd = X.exact_areas(geoms, valid, signed=signed)
        for i, (e, b) in enumerate(zip(ex, bd)):
            if e is None:
                continue
            err = X.abs_err(got[i], e)
            assert err <= b, (name, "signed" if signed else "area", i, err, b)
    ln = np.asarray(s.euclidean_length())
    rel_close(ln, oracle.euclidean_length(a), (name, "length"))
    for i, g in enumerate(geoms):
        if valid is None or valid[i]:
            ext = [p[0] for p in g]
            e = X.exact_length(ext)
            assert X.abs_err(ln[i], e) <= X.length_bound(ext, float(e)), (name, "length", i)
    assert np.array_equal(s.bounds(), oracle.bounds(a), equal_nan=True), (name, "bounds")
# integer rings of every class length at +-2^30: the area is the untranslated one, bit for bit
rng = np.random.default_rng(9)
rings = []
for n in (4, 5, 16, 17, 128, 129, 512, 513, 8191, 8192, 8193, 20000):
    t = 2 * np.pi * np.arange(n - 1) / (n - 1)
    r = np.round(rng.uniform(50, 4000) * (1 + 0.2 * np.sin(3 * t)))
    xy = np.stack([np.round(r * np.cos(t)), np.round(r * np.sin(t))], axis=1)
    rings.append(np.concatenate([xy, xy[:1]]))
base = GeoArrowArray.from_polygons([[r.tolist()] for r in rings], close=False)
a0 = np.asarray(GeoSeries(base).signed_area())
assert np.array_equal(a0, [float(X.ring_area2(r) / 2) for r in rings])
for t in ((2.0**30, -(2.0**30)), (-(2.0**30), 2.0**30), (2.0**30, 2.0**30)):
    moved = X.translated_exactly(base, t)
    assert np.array_equal(np.asarray(GeoSeries(moved).signed_area()), a0), t
    assert np.array_equal(np.asarray(GeoSeries(moved).euclidean_length()), np.asarray(GeoSeries(base).euclidean_length())), t
# the ops lattice golden at the lattice offsets: area bit for bit
import numpy as _np
z = _np.load(os.path.join(os.getcwd(), "tests", "golden", "ops_lattice.npz"))
polys = GeoArrowArray(_abi.GEOM_POLYGON, z["xy"], geom_offsets=z["geom_offsets"], ring_offsets=z["ring_offsets"])
for t in X.LATTICE_OFFSETS:
    assert np.array_equal(np.asarray(GeoSeries(X.translated_exactly(polys, t)).area()), z["area"]), t
print("GEOREF_FORMS_OK")
"""


@pytest.mark.parametrize("mode", ["1", "0", None])
def test_area_length_bounds_both_forms(mode):
    env = dict(os.environ)
    env.pop("GPK_RING_STREAM", None)
    if mode is not None:
        env["GPK_RING_STREAM"] = mode
    r = subprocess.run([sys.executable, "-c", _FORMS_PROG], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0 and "GEOREF_FORMS_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def _centroid_rows(geoms, valid):
    for i, g in enumerate(geoms):
        if valid is None or valid[i]:
            ec = X.exact_centroid(g)
            if ec is not None:
                yield i, ec


@pytest.mark.parametrize("name", list(X.area_fixtures()))
def test_centroid_within_extent_relative_bound(gpk, oracle, name):
    geoms, valid = X.area_fixtures()[name]
    a = X.to_array(geoms, valid)
    c = GeoSeries(a).centroid().array.xy
    n = 0
    for i, ec in _centroid_rows(geoms, valid):
        b = X.centroid_bound(geoms[i], ec)
        for ax in (0, 1):
            assert X.abs_err(c[i, ax], ec[ax]) <= b[ax], (name, i, ax, X.abs_err(c[i, ax], ec[ax]), b[ax])
        n += 1
    assert n >= len(geoms) // 2


def test_centroid_of_zero_area_rings_at_offsets(gpk, oracle):
    """dyadic collinear rings (every shifted term exactly 0, so the area is exactly 0 in f64 too): the length-weighted centroid
    of the ring, every class length; positive weights, so gamma(n + 6) of the coordinate plus the exact value's rounding"""
    rings = []
    for i, n in enumerate((3, 5, 15, 17, 129, 513, 8193, 17001)):  # a line of m points out and back: 2 m - 1 coordinates
        px, py = X.PLACEMENTS[i % len(X.PLACEMENTS)]
        k = np.arange((n + 1) // 2)
        line = np.stack([np.round(px) + 0.25 * k, np.round(py) + 0.75 * k], axis=1)
        rings.append(np.concatenate([line, line[-2::-1]]))
    a = GeoArrowArray.from_polygons([[r.tolist()] for r in rings], close=False)
    s = GeoSeries(a)
    assert np.array_equal(np.asarray(s.area()), np.zeros(len(rings)))
    c = s.centroid().array.xy
    exp, _ = oracle.centroid(a)
    assert np.allclose(c, exp, rtol=1e-9, atol=0)
    for i, r in enumerate(rings):
        e = X.linestring_centroid_exact(r)
        for ax in (0, 1):
            assert X.abs_err(c[i, ax], e[ax]) <= X.gamma(len(r) + 6) * abs(float(e[ax])) * 1.01, (i, ax)


def _probes():
    geoms = X.buildings(150, seed=11) + X.dyadic_buildings(120)
    pts, rows = X.probe_points(geoms)
    return geoms, X.to_array(geoms), pts, rows


def test_distance_and_predicates_near_edges(gpk, oracle):
    geoms, a, pts, rows = _probes()
    P = GeoArrowArray.from_points(pts)
    d = GeoSeries(P).distance(GeoSeries(a), rows)
    assert np.array_equal(d == 0, oracle.distance_rowwise(P, a, rows) == 0)
    take = X.to_array([geoms[r] for r in rows])
    S, Q = GeoSeries(take), GeoSeries(P)
    contains, within, inter = S.contains(Q), Q.within(S), Q.intersects(S)
    for i, (p, r) in enumerate(zip(pts, rows)):
        pos = X.geom_position(p, geoms[r])
        assert contains[i] == (pos > 0) and within[i] == (pos > 0) and inter[i] == (pos >= 0), (i, pos)
        e, b = X.exact_distance(p, geoms[r])
        if e == 0:
            assert d[i] == 0.0, i
        else:
            assert X.abs_err(d[i], e) <= b, (i, d[i], e, b)


def _lines_and_probes():
    """linestrings (building exteriors) and 24 probes a line: the grouped row-map schedule takes targets with >= 8 rows each"""
    geoms = X.buildings(60, seed=12, holes=False, multi=False) + X.dyadic_buildings(40, seed=13)
    lines = [g[0][0] for g in geoms]
    pts, rows = X.probe_points([[[l]] for l in lines] * 2, seed=14)
    rows = rows % len(lines)
    return lines, GeoArrowArray.from_linestrings([l.tolist() for l in lines]), pts, rows.astype(np.uint32)


def test_distance_to_linestrings_per_row_and_grouped(gpk, oracle):
    from geopolars_amd.geoseries import RowMap

    lines, L, pts, rows = _lines_and_probes()
    P = GeoArrowArray.from_points(pts)
    exp = oracle.distance_rowwise(P, L, rows)
    got = GeoSeries(P).distance(GeoSeries(L), rows)  # >= 8 rows per target: the grouped schedule
    rm = RowMap(GeoSeries(L), rows)
    got_map = GeoSeries(P).distance(GeoSeries(L), row_map=rm)
    rm.free()
    for g in (got, got_map):
        assert np.array_equal(g == 0, exp == 0)  # geo's EPSILON rule for points on linestrings, as the oracle applies it
        for i, (p, r) in enumerate(zip(pts, rows)):
            d2, lmax = X.point_seqs_dist2(p, [lines[r]])
            e = X.dec_sqrt(d2)
            if e == 0:
                assert g[i] == 0.0, i
            elif exp[i] != 0:
                assert X.abs_err(g[i], e) <= X.distance_bound(float(e), lmax), (i, g[i], e)


def _pip_pairs(left, right):
    from geopolars_amd.spatial_index import join_pairs

    pairs, counts = join_pairs(GeoSeries(left), GeoSeries(right), "intersects")
    return pairs, counts


def test_point_in_polygon_join_near_edges(gpk, oracle):
    geoms, a, pts, rows = _probes()
    P = GeoArrowArray.from_points(pts)
    pairs, counts = _pip_pairs(P, a)
    exp, exp_counts, _ = oracle.spatial_join(P, a, "intersects", mode=1)
    assert np.array_equal(pairs, exp) and np.array_equal(counts, exp_counts)
    prog = (
        "import os, sys, numpy as np\nsys.path.insert(0, os.getcwd())\n"
        "from tests import exact_ref as X\nfrom tests.test_gpu_georeferenced import _probes, _pip_pairs\n"
        "from geopolars_amd.geoarrow import GeoArrowArray\nfrom oracle import pyoracle as oracle\noracle.build(); oracle.lib()\n"
        "geoms, a, pts, rows = _probes()\nP = GeoArrowArray.from_points(pts)\npairs, counts = _pip_pairs(P, a)\n"
        "exp, exp_counts, _ = oracle.spatial_join(P, a, 'intersects', mode=1)\n"
        "assert np.array_equal(pairs, exp) and np.array_equal(counts, exp_counts)\nprint('CHAIN_OK')\n"
    )
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, GPK_TILE_KERNEL="chain"))
    assert r.returncode == 0 and "CHAIN_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def _npz(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name))


@pytest.mark.parametrize("t", X.LATTICE_OFFSETS)
def test_joins_on_translated_lattice_goldens(gpk, t):
    from geopolars_amd.spatial_index import join_pairs

    z = _npz("join_lattice.npz")
    polys = X.translated_exactly(GeoArrowArray(_abi.GEOM_POLYGON, z["xy"], geom_offsets=z["geom_offsets"], ring_offsets=z["ring_offsets"]), t)
    pts = X.translated_exactly(GeoArrowArray.from_points(z["points"]), t)
    exp = z["pairs"]
    pairs, _ = join_pairs(GeoSeries(pts), GeoSeries(polys), "intersects")
    assert np.array_equal(pairs, exp)
    back, _ = join_pairs(GeoSeries(polys), GeoSeries(pts), "contains")
    assert np.array_equal(back[np.lexsort((back[:, 0], back[:, 1]))][:, ::-1], exp)


@pytest.mark.parametrize("k", [30, -60])
def test_polygon_joins_on_scaled_contains_lattice(gpk, oracle, k):
    """polygon x polygon (C4) intersects and contains joins: the nudged contains lattice moves by powers of two only (no
    translation keeps its 2^-50 nudges exact); 600 polygons a side against the oracle's brute force"""
    from geopolars_amd.spatial_index import join_pairs

    from .lattice import load_contains_golden

    a, b, _ = load_contains_golden()
    a, b = X.polygon_geoms(a)[:600], X.polygon_geoms(b)[:600]
    a, b = X.to_polygon_array(a), X.to_polygon_array(b)
    sa, sb = X.scaled(a, k), X.scaled(b, k)
    for pred in ("intersects", "contains"):
        exp, _, _ = oracle.spatial_join(a, b, pred, mode=0)
        got, _ = join_pairs(GeoSeries(sa), GeoSeries(sb), pred)
        assert np.array_equal(got, exp), pred


def test_convex_hull_of_near_collinear_sets(gpk, oracle):
    sets = X.near_collinear_sets()
    a = GeoArrowArray(_abi.GEOM_MULTIPOINT, np.concatenate(sets), geom_offsets=np.cumsum([0] + [len(s) for s in sets]).astype(np.int32))
    hx, ho = oracle.convex_hull(a)
    h = GeoSeries(a).convex_hull().array
    assert np.array_equal(h.ring_offsets, ho)
    for i, s in enumerate(sets):
        got = X.canon(h.xy[ho[i] : ho[i + 1]])
        assert np.array_equal(got, X.canon(hx[ho[i] : ho[i + 1]])), i
        assert np.array_equal(got, X.canon(X.exact_hull(s))), i


def _nearest_setup(seed=15):
    """right: dyadic buildings (vertices on multiples of 2^-4) around two placements; left: queries on a 2^-3 grid around them, so
    that exact ties (a query equidistant from two vertices or edges) are common and fall on index cell borders"""
    rng = np.random.default_rng(seed)
    geoms = []
    for i in range(120):
        px, py = X.PLACEMENTS[(i % 2) * 1]
        cx, cy = np.round(px) + 16 * int(rng.integers(0, 12)), np.round(py) + 16 * int(rng.integers(0, 12))
        w, h = [float(rng.integers(2, 64)) / 8 for _ in range(2)]
        geoms.append([[np.array([(cx, cy), (cx + w, cy), (cx + w, cy + h), (cx, cy + h), (cx, cy)])]])
    right = X.to_array(geoms)
    q = []
    for j in range(400):
        px, py = X.PLACEMENTS[(j % 2) * 1]
        q.append((np.round(px) + int(rng.integers(-16, 210)) / 8, np.round(py) + int(rng.integers(-16, 210)) / 8))
    return GeoArrowArray.from_points(np.array(q)), right


def test_nearest_join_at_offsets_with_exact_ties(gpk, oracle):
    from geopolars_amd.spatial_index import nearest_pairs

    from .test_gpu_nearest import _check_against_oracle, _oracle_matrix

    left, right = _nearest_setup()
    pairs, counts, dist = nearest_pairs(GeoSeries(left), GeoSeries(right))
    D = _oracle_matrix(oracle, left, right)
    _check_against_oracle(D, pairs, counts, dist)
    # tie sets complete: every right row at exactly the row's minimum distance, decided in exact arithmetic among the rows the
    # oracle puts within 1e-6 of it (geo's formula rounds an exact tie between a vertex and an edge differently; the kernel's
    # squared-distance fractions of these dyadic inputs are exact, so exact ties are equal doubles there)
    starts = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    geoms = X.polygon_geoms(right)
    n_ties = 0
    for l in range(len(left)):
        p = left.xy[l]
        cand = np.nonzero(D[l] <= D[l].min() * (1 + 1e-6))[0]
        d2 = {int(r): (0 if X.geom_position(p, geoms[r]) >= 0 else X.point_seqs_dist2(p, [g for rings in geoms[r] for g in rings])[0]) for r in cand}
        m = min(d2.values())
        exp = sorted(r for r, v in d2.items() if v == m)
        assert pairs[starts[l] : starts[l + 1], 1].tolist() == exp, (l, exp)
        n_ties += len(exp) > 1
    assert n_ties >= 20


# ---- exact power-of-two scaling -----------------------------------------------------------------------------------------------

SCALES = [7, -7, 30, -30, 60, -60, 100, -100]


def _ops_of(polys, lines, P, rows, eps):
    from geopolars_amd.spatial_index import join_pairs, nearest_pairs

    s, l, p = GeoSeries(polys), GeoSeries(lines), GeoSeries(P)
    h = s.convex_hull().array
    simp = l.simplify(eps).array
    return {
        "area": np.asarray(s.area()), "signed": np.asarray(s.signed_area()), "length": np.asarray(s.euclidean_length()),
        "llength": np.asarray(l.euclidean_length()), "centroid": s.centroid().array.xy, "lcentroid": l.centroid().array.xy,
        "bounds": s.bounds(), "hull": (h.xy, h.ring_offsets), "simplify": (simp.xy, simp.geom_offsets),
        "dist": p.distance(s, rows), "ldist": p.distance(l, rows % len(lines)),
        "contains": s.contains(GeoSeries(GeoArrowArray.from_points(P.xy[: len(polys)]))),
        "join": join_pairs(p, s, "intersects"), "near": nearest_pairs(p, s), "lnear": nearest_pairs(p, l),
    }


def _bits(x):
    return np.asarray(x).view(np.uint64)


@pytest.mark.parametrize("k", SCALES)
def test_every_op_scales_exactly_by_powers_of_two(gpk, k):
    geoms = X.buildings(200, seed=16)
    polys = X.to_array(geoms)
    ls = [r for g in geoms[:80] for r in g[0]]
    lines = GeoArrowArray.from_linestrings([np.concatenate([r, r[:3] + 0.37]).tolist() for r in ls])
    pts, rows = X.probe_points(geoms, seed=17)
    P = GeoArrowArray.from_points(pts)
    eps = 0.05
    base = _ops_of(polys, lines, P, rows, eps)
    got = _ops_of(X.scaled(polys, k), X.scaled(lines, k), X.scaled(P, k), rows, np.ldexp(eps, k))
    for name in ("area", "signed"):
        assert np.array_equal(_bits(got[name]), _bits(np.ldexp(base[name], 2 * k))), name
    for name in ("length", "llength", "centroid", "lcentroid", "bounds", "dist", "ldist"):
        assert np.array_equal(_bits(got[name]), _bits(np.ldexp(base[name], k))), name
    for name in ("hull", "simplify"):
        assert np.array_equal(got[name][1], base[name][1]) and np.array_equal(_bits(got[name][0]), _bits(np.ldexp(base[name][0], k))), name
    assert np.array_equal(got["contains"], base["contains"])
    for name in ("join", "near", "lnear"):
        for g, b in zip(got[name][:2], base[name][:2]):
            assert np.array_equal(g, b), name
    for name in ("near", "lnear"):
        assert np.array_equal(_bits(got[name][2]), _bits(np.ldexp(base[name][2], k))), name
