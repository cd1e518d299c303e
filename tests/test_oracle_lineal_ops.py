"""CPU: the oracle's geodesic_length and simplify restatements (oracle/gpk_oracle.c) against what exists OUTSIDE this repository
for them: the values geo's own documentation states, Vincenty's published test line, and — for Douglas-Peucker — an
independent pure-Python recursion on exact rationals plus hand-checked cases of the rules that are particular to geo 0.27
(last farthest point among equals, the INITIAL_MIN floor of 4 for rings)."""
import math
from fractions import Fraction as F

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from tests import simplify_ref as R


def _dms(d, m, s):
    return d + m / 60.0 + s / 3600.0


def test_geodesic_lengths_reproduce_published_values(oracle):
    nyc_london = GeoArrowArray.from_linestrings([[(-74.006, 40.7128), (-0.1278, 51.5074)]])
    # the examples of geo's HaversineLength / VincentyLength docs (New York City -> London), rounded to metres there
    assert round(float(oracle.geodesic_length(nyc_london, "haversine")[0])) == 5_570_230
    assert round(float(oracle.geodesic_length(nyc_london, "vincenty")[0])) == 5_585_234
    # T. Vincenty (1975), the line Flinders Peak -> Buninyong: 54 972.271 m
    fb = GeoArrowArray.from_linestrings([[(_dms(144, 25, 29.52440), -_dms(37, 57, 3.72030)), (_dms(143, 55, 35.38390), -_dms(37, 39, 10.15610))]])
    assert abs(float(oracle.geodesic_length(fb, "vincenty")[0]) - 54972.271) < 1e-3
    # coincident points: 0; antipodal points: upstream's FailedToConverge -> NaN; a polygon counts its exterior ring only
    z = GeoArrowArray.from_linestrings([[(10.0, 20.0), (10.0, 20.0)], [(0.0, 0.0), (180.0, 0.0)], []])
    v = oracle.geodesic_length(z, "vincenty")
    assert v[0] == 0.0 and np.isnan(v[1]) and v[2] == 0.0
    poly = GeoArrowArray.from_polygons([[[(0, 0), (1, 0), (1, 1), (0, 1)], [(0.2, 0.2), (0.2, 0.4), (0.4, 0.4), (0.4, 0.2)]]])
    ring = GeoArrowArray.from_linestrings([[(0, 0), (1, 0), (1, 1), (0, 1), (0, 0)]])
    assert oracle.geodesic_length(poly, "haversine")[0] == oracle.geodesic_length(ring, "haversine")[0]


def test_karney_geodesic_reproduces_published_lines(oracle):
    """"geodesic" = geo 0.27 GeodesicLength = Karney's inverse problem (geographiclib-rs): the values geo's documentation and
    GeographicLib publish.  (lon, lat) order, like every geodesic method of the surface."""

    def line(*pts):
        return float(oracle.geodesic_length(GeoArrowArray.from_linestrings([list(pts)]), "geodesic")[0])

    # geo's GeodesicDistance / GeodesicLength doc examples (rounded to metres there)
    assert round(line((-74.006, 40.7128), (-0.1278, 51.5074))) == 5_585_234
    assert round(line((-74.006, 40.7128), (-0.1278, 51.5074), (135.5244559, 34.687455))) == 15_109_158
    # GeographicLib's documentation: Wellington (41.32S 174.81E) -> Salamanca (40.96N 5.50W), s12 = 19959679.267 m
    assert abs(line((174.81, -41.32), (-5.50, 40.96)) - 19959679.26735382) < 1e-5
    # GeodSolve's example: JFK (40.6N 73.8W) -> LHR (51.6N 0.5W), 5551759.400 m
    assert abs(line((-73.8, 40.6), (-0.5, 51.6)) - 5551759.4003186841) < 1e-5
    # the first line of GeographicLib's GeodTest set
    assert abs(line((-139.44815, 35.60777), (-69.95921, -11.17491)) - 8935244.5604818305) < 1e-6
    # Karney 2013, the nearly antipodal example: (0, 0) -> (0.5N, 179.5E), 19936288.579 m
    assert abs(line((0.0, 0.0), (179.5, 0.5)) - 19936288.578965) < 1e-3
    # closed forms on WGS84: a quarter of the equator, a quarter meridian (10001965.729 m), antipodes over the pole
    a = 6378137.0
    assert abs(line((0.0, 0.0), (90.0, 0.0)) - a * np.pi / 2) < 1e-6
    assert abs(line((0.0, 0.0), (0.0, 90.0)) - 10001965.729313) < 1e-4
    assert abs(line((0.0, 0.0), (180.0, 0.0)) - 2 * 10001965.729313) < 1e-3  # (Vincenty's iteration fails here)
    assert line((10.0, 20.0), (10.0, 20.0)) == 0.0
    # symmetric, and in step with Vincenty's formula where that converges (sub-millimetre on 20 000 random lines)
    rng = np.random.default_rng(2)
    p = np.stack([rng.uniform(-180, 180, 20_000), rng.uniform(-89, 89, 20_000)], axis=1)
    q = np.stack([rng.uniform(-180, 180, 20_000), rng.uniform(-89, 89, 20_000)], axis=1)
    off = np.arange(0, 40_001, 2, dtype=np.int32)
    fwd = GeoArrowArray(_abi.GEOM_LINESTRING, np.stack([p, q], axis=1).reshape(-1, 2), geom_offsets=off)
    bwd = GeoArrowArray(_abi.GEOM_LINESTRING, np.stack([q, p], axis=1).reshape(-1, 2), geom_offsets=off)
    kf, kb, vf = oracle.geodesic_length(fwd, "geodesic"), oracle.geodesic_length(bwd, "geodesic"), oracle.geodesic_length(fwd, "vincenty")
    assert np.all(np.abs(kf - kb) <= 1e-8)
    ok = ~np.isnan(vf) & (kf < 1.9e7)  # (Vincenty's series loses accuracy towards the antipode)
    assert ok.sum() > 15_000 and np.all(np.abs(kf[ok] - vf[ok]) < 1e-3)


def _rdp_rational(pts, eps, min_pts):
    """geo 0.27 compute_rdp on exact rationals (tests/simplify_ref.py: squared distances compared, so no rounding anywhere)"""
    return [p for p, k in zip(pts, R.rdp_exact(pts, float(eps), min_pts).keep) if k]


@pytest.mark.parametrize("seed", range(6))
def test_simplify_matches_the_rational_recursion_on_lattice_lines(oracle, seed):
    rng = np.random.default_rng(seed)
    lines = []
    for _ in range(40):
        n = int(rng.integers(2, 60))
        walk = np.cumsum(rng.integers(-4, 5, (n, 2)), axis=0)
        lines.append([tuple(int(v) for v in p) for p in walk])
    a = GeoArrowArray.from_linestrings(lines)
    for eps in (F(1, 2), F(3), F(7)):  # distances of lattice data are never within an ulp of these: float == rational decisions
        xy, off = oracle.simplify(a, float(eps))
        for i, line in enumerate(lines):
            exp = _rdp_rational(line, eps, 2)
            assert xy[off[i] : off[i + 1]].tolist() == [[float(x), float(y)] for x, y in exp], (seed, i, eps)


def test_simplify_rules_particular_to_geo(oracle):
    # geo's doc example: [(0,0),(5,4),(11,5.5),(17.3,3.2),(27.8,0.1)] with epsilon 1.0 -> [(0,0),(5,4),(11,5.5),(27.8,0.1)]
    ls = GeoArrowArray.from_linestrings([[(0.0, 0.0), (5.0, 4.0), (11.0, 5.5), (17.3, 3.2), (27.8, 0.1)]])
    xy, off = oracle.simplify(ls, 1.0)
    assert xy.tolist() == [[0.0, 0.0], [5.0, 4.0], [11.0, 5.5], [27.8, 0.1]] and off.tolist() == [0, 4]
    # polygons: a ring never drops below 4 coordinates (INITIAL_MIN = 4) — a thin sliver keeps a closed triangle
    poly = GeoArrowArray.from_polygons([[[(0, 0), (10, 0), (10, 0.1), (5, 0.2), (0, 0.1)]]])
    xy, off = oracle.simplify(poly, 5.0)
    assert off[-1] >= 4 and xy[0].tolist() == xy[-1].tolist()
    # the doc example of Polygon::simplify: [(0,0),(0,10),(5,11),(10,10),(10,0),(0,0)] with epsilon 2 drops (5, 11)
    poly = GeoArrowArray.from_polygons([[[(0, 0), (0, 10), (5, 11), (10, 10), (10, 0)]]])
    xy, off = oracle.simplify(poly, 2.0)
    assert xy.tolist() == [[0, 0], [0, 10], [10, 10], [10, 0], [0, 0]]
    # ties: two interior points equally far from the chord -> the split happens at the LAST one
    ls = GeoArrowArray.from_linestrings([[(0, 0), (2, 3), (4, 3), (6, 0)]])
    xy, _ = oracle.simplify(ls, 1.0)
    assert xy.tolist() == [[0, 0], [2, 3], [4, 3], [6, 0]]
    # epsilon <= 0 and short sequences come back unchanged
    xy, off = oracle.simplify(ls, 0.0)
    assert len(xy) == 4
    two = GeoArrowArray.from_linestrings([[(0, 0), (1, 1)], [(5, 5)], []])
    xy, off = oracle.simplify(two, 10.0)
    assert off.tolist() == [0, 2, 3, 3]


def test_karney_restatement_against_an_independent_solver(oracle):
    """oracle/gpk_oracle.c's Karney restatement (series + Newton, the algorithm of the HIP kernel written a second time) against
    oracle/geodesic_quadrature.py: the same geodesic problem solved by Gauss-Legendre quadrature of Bessel's integrals and a
    bisection on the azimuth — a different derivation, so the two cannot share a bug.  The independent solver itself is first
    held against the values GeographicLib publishes."""
    from oracle import geodesic_quadrature as gq

    published = [  # (lon1, lat1, lon2, lat2, metres): GeographicLib's documentation / GeodTest line 1 / Karney 2013 / closed forms
        (174.81, -41.32, -5.50, 40.96, 19959679.26735382),
        (-73.8, 40.6, -0.5, 51.6, 5551759.4003186841),
        (-139.44815, 35.60777, -69.95921, -11.17491, 8935244.5604818305),
        (0.0, 0.0, 179.5, 0.5, 19936288.578965),
        (0.0, 0.0, 90.0, 0.0, 6378137.0 * np.pi / 2),
        (0.0, 0.0, 0.0, 90.0, 10001965.729313),
        (0.0, 0.0, 180.0, 0.0, 2 * 10001965.729313),
    ]
    for l1, p1, l2, p2, metres in published:
        assert abs(float(gq.inverse_distance([l1], [p1], [l2], [p2])[0]) - metres) < 2e-6

    def c_oracle(l1, p1, l2, p2):
        n = len(l1)
        xy = np.empty((2 * n, 2))
        xy[0::2, 0], xy[0::2, 1], xy[1::2, 0], xy[1::2, 1] = l1, p1, l2, p2
        return oracle.geodesic_length(GeoArrowArray(_abi.GEOM_LINESTRING, xy, geom_offsets=np.arange(0, 2 * n + 1, 2, dtype=np.int32)), "geodesic")

    rng = np.random.default_rng(40)
    n = 12_000
    sets = [(rng.uniform(-180, 180, n), rng.uniform(-90, 90, n), rng.uniform(-180, 180, n), rng.uniform(-90, 90, n))]
    for spread in (0.5, 0.01, 1e-4):
        m = 3_000
        p1, l1 = rng.uniform(-75, 75, m), rng.uniform(-180, 180, m)
        sets.append((l1, p1, l1 + 180.0 + rng.normal(0, spread, m), -p1 + rng.normal(0, spread, m)))
    m = 2_000
    p1, l1 = rng.uniform(-89, 89, m), rng.uniform(-180, 180, m)
    sets.append((l1, p1, l1 + rng.normal(0, 1e-3, m), p1 + rng.normal(0, 1e-3, m)))
    sets.append((l1, p1, l1, rng.uniform(-90, 90, m)))
    sets.append((l1, p1, l1 + 180.0, rng.uniform(-90, 90, m)))
    sets.append((l1, np.zeros(m), rng.uniform(-180, 180, m), np.zeros(m)))
    sets.append((l1, np.full(m, 90.0), rng.uniform(-180, 180, m), rng.uniform(-90, 90, m)))
    for l1, p1, l2, p2 in sets:
        p2 = np.clip(p2, -90.0, 90.0)
        got, exp = c_oracle(l1, p1, l2, p2), gq.inverse_distance(l1, p1, l2, p2)
        assert np.all(np.abs(got - exp) <= 1e-9 * exp + 2e-8)


def _pair_lines(l1, p1, l2, p2):
    n = len(l1)
    xy = np.empty((2 * n, 2))
    xy[0::2, 0], xy[0::2, 1], xy[1::2, 0], xy[1::2, 1] = l1, p1, l2, p2
    return GeoArrowArray(_abi.GEOM_LINESTRING, xy, geom_offsets=np.arange(0, 2 * n + 1, 2, dtype=np.int32))


def test_haversine_against_a_high_precision_evaluation(oracle):
    """the oracle's f64 half-angle formula against the same great-circle distance at 50 digits: its error per regime is what
    tests/geodesic_ref.py records (the GPU test allows the kernel 4 times as much)"""
    pytest.importorskip("mpmath")
    from tests import geodesic_ref as Gd

    for regime, q in Gd.haversine_pairs().items():
        err = Gd.haversine_errors_m(oracle.geodesic_length(_pair_lines(*q), "haversine"), Gd.haversine_mp(*q))
        print(f"haversine {regime}: largest error {err.max():.3e} m")
        assert err.max() <= Gd.HAVERSINE_ERR_M[regime], (regime, err.max())


def test_vincenty_restatement_and_the_pairs_far_from_the_iteration_limit(oracle):
    from tests import geodesic_ref as Gd

    l1, p1, l2, p2, is_nan, drawn = Gd.nearly_antipodal_pairs()
    assert len(l1) == 1533 and drawn == 1600 and is_nan.sum() == 688  # pairs kept / drawn / failing to converge
    v = oracle.geodesic_length(_pair_lines(l1, p1, l2, p2), "vincenty")
    assert np.array_equal(np.isnan(v), is_nan)
    mine = np.array([Gd.vincenty_py(*(float(x) for x in q))[0] for q in zip(l1, p1, l2, p2)])
    assert np.all(np.abs(mine[~is_nan] - v[~is_nan]) <= 1e-12 * v[~is_nan])
    assert math.isnan(Gd.vincenty_py(0.0, 0.0, 180.0, 0.0)[0]) and Gd.vincenty_py(10.0, 20.0, 10.0, 20.0)[0] == 0.0
    assert [Gd.geodesic_group_size(c, s) for c, s in ((0, 0), (24, 1), (25, 1), (240, 10), (241, 10))] == [0, 4, 16, 4, 16]
