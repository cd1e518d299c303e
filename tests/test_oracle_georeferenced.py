"""The CPU oracle at georeferenced magnitudes (UTM, Web Mercator) against exact answers (tests/exact_ref.py): every f64 result
within the a-priori error bound of geo's formula, predicates / hull / join exactly; and the bounds are sharp enough to matter —
geo's shifted sums with the shift dropped or borrowed from the previous ring break them by >= 100x on every fixture, so the
GPU tests that hold the HIP kernels to the same bounds (test_gpu_georeferenced.py) catch such a kernel.

The lattice goldens translated by exact binary offsets: integer coordinates stay integers, so area, length and distance are the
untranslated doubles bit for bit, hulls and bounds move by exactly the offset, predicates and pairs do not change."""
import os

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray

from . import exact_ref as X

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = X.area_fixtures()


def _rows(geoms, valid):
    return [i for i in range(len(geoms)) if valid is None or valid[i]]


@pytest.mark.parametrize("name", list(FIXTURES))
def test_area_within_bound_and_wrong_shifts_break_it(oracle, name):
    geoms, valid = FIXTURES[name]
    a = X.to_array(geoms, valid)
    for signed in (False, True):
        got = oracle.area(a, signed=signed)
        ex, bd = X.exact_areas(geoms, valid, signed=signed)
        assert np.array_equal(np.isnan(got), [e is None for e in ex])
        m0, mp = X.mutant_areas(geoms, "zero", signed), X.mutant_areas(geoms, "prev", signed)
        for i in _rows(geoms, valid):
            err = X.abs_err(got[i], ex[i])
            assert err <= bd[i], (name, signed, i, err, bd[i])
            if ex[i] == 0:
                assert got[i] == 0.0, (name, i)
                continue
            for kind, m in (("zero", m0), ("prev", mp)):
                assert X.abs_err(m[i], ex[i]) >= 100 * bd[i], (name, signed, i, kind, X.abs_err(m[i], ex[i]), bd[i])


@pytest.mark.parametrize("name", list(FIXTURES))
def test_centroid_within_bound_and_wrong_shifts_break_it(oracle, name):
    geoms, valid = FIXTURES[name]
    a = X.to_array(geoms, valid)
    c, ok = oracle.centroid(a)
    m0, mp = X.mutant_centroids(geoms, "zero"), X.mutant_centroids(geoms, "prev")
    checked = 0
    for i in _rows(geoms, valid):
        ec = X.exact_centroid(geoms[i])
        if ec is None:
            continue
        b = X.centroid_bound(geoms[i], ec)
        for ax in (0, 1):
            err = X.abs_err(c[i, ax], ec[ax])
            assert err <= b[ax], (name, i, ax, err, b[ax])
            for kind, m in (("zero", m0), ("prev", mp)):
                assert X.abs_err(m[i, ax], ec[ax]) >= 100 * b[ax], (name, i, ax, kind)
        checked += 1
    assert checked >= len(geoms) // 2


@pytest.mark.parametrize("name", list(FIXTURES))
def test_length_and_bounds_exact(oracle, name):
    geoms, valid = FIXTURES[name]
    a = X.to_array(geoms, valid)
    ln, bb = oracle.euclidean_length(a), oracle.bounds(a)
    for i in _rows(geoms, valid):
        exteriors = [p[0] for p in geoms[i]]
        e = X.exact_length(exteriors)
        assert X.abs_err(ln[i], e) <= X.length_bound(exteriors, float(e)), (name, i)
        if geoms[i]:
            allxy = np.concatenate([r for p in geoms[i] for r in p])
            assert np.array_equal(bb[i], [allxy[:, 0].min(), allxy[:, 1].min(), allxy[:, 0].max(), allxy[:, 1].max()])


def _probe_setup():
    geoms = X.buildings(150, seed=11) + X.dyadic_buildings(120)
    pts, rows = X.probe_points(geoms)
    return geoms, X.to_array(geoms), pts, rows


def test_distance_and_predicates_near_edges_at_offsets(oracle):
    geoms, a, pts, rows = _probe_setup()
    P = GeoArrowArray.from_points(pts)
    d = oracle.distance_rowwise(P, a, rows)
    take = X.to_array([geoms[r] for r in rows])
    contains = oracle.predicate_rowwise(take, P, "contains").astype(bool)
    within = oracle.predicate_rowwise(P, take, "within").astype(bool)
    inter = oracle.predicate_rowwise(P, take, "intersects").astype(bool)
    n_on = 0
    for i, (p, r) in enumerate(zip(pts, rows)):
        pos = X.geom_position(p, geoms[r])
        n_on += pos == 0
        assert contains[i] == (pos > 0) and within[i] == (pos > 0) and inter[i] == (pos >= 0), (i, pos)
        e, b = X.exact_distance(p, geoms[r])
        if e == 0:
            assert d[i] == 0.0, i
        else:
            assert X.abs_err(d[i], e) <= b, (i, d[i], e, b)
    assert n_on >= 300  # vertices and exact midpoints of the dyadic rows


def test_point_in_polygon_join_near_edges_is_exact(oracle):
    geoms, a, pts, rows = _probe_setup()
    P = GeoArrowArray.from_points(pts)
    pairs, counts, _ = oracle.spatial_join(P, a, "intersects", mode=1)
    got = set(map(tuple, pairs.tolist()))
    # only the probe's own geometry and its neighbours can hold it; every pair the join returns is checked too
    exp = set()
    for i, (p, r) in enumerate(zip(pts, rows)):
        for g in {int(r)} | {int(q) for (l, q) in got if l == i}:
            if X.geom_position(p, geoms[g]) > 0:  # the join's intersects rejects points on a boundary (KA-1)
                exp.add((i, g))
    assert got == exp


def test_convex_hull_of_near_collinear_sets_is_exact(oracle):
    sets = X.near_collinear_sets()
    a = GeoArrowArray(_abi.GEOM_MULTIPOINT, np.concatenate(sets), geom_offsets=np.cumsum([0] + [len(s) for s in sets]).astype(np.int32))
    hx, ho = oracle.convex_hull(a)
    for i, s in enumerate(sets):
        assert np.array_equal(X.canon(hx[ho[i] : ho[i + 1]]), X.canon(X.exact_hull(s))), i


# ---- the lattice goldens, translated ------------------------------------------------------------------------------------------


def _npz(name):
    return np.load(os.path.join(HERE, "golden", name))


def _ops(t):
    z = _npz("ops_lattice.npz")
    polys = GeoArrowArray(_abi.GEOM_POLYGON, z["xy"], geom_offsets=z["geom_offsets"], ring_offsets=z["ring_offsets"])
    return z, X.translated_exactly(polys, t), X.translated_exactly(GeoArrowArray.from_points(z["points"]), t)


@pytest.mark.parametrize("t", X.LATTICE_OFFSETS)
def test_translated_ops_lattice(oracle, t):
    z, polys, pts = _ops(t)
    _, p0, q0 = _ops((0.0, 0.0))
    assert np.array_equal(oracle.area(polys), z["area"])  # bit for bit
    assert np.array_equal(oracle.distance_rowwise(pts, polys), oracle.distance_rowwise(q0, p0))
    assert np.array_equal(oracle.euclidean_length(polys), oracle.euclidean_length(p0))
    hx, ho = oracle.convex_hull(polys)
    assert np.array_equal(ho, z["hull_offsets"])
    for g in range(len(ho) - 1):
        assert np.array_equal(X.canon(hx[ho[g] : ho[g + 1]]), X.canon(z["hull_xy"][ho[g] : ho[g + 1]] + t)), g
    b0 = oracle.bounds(p0)
    assert np.array_equal(oracle.bounds(polys), b0 + [t[0], t[1], t[0], t[1]])
    pos = z["position"]
    assert np.array_equal(oracle.predicate_rowwise(polys, pts, "contains").astype(bool), pos > 0)
    assert np.array_equal(oracle.predicate_rowwise(pts, polys, "intersects").astype(bool), pos >= 0)
    c, _ = oracle.centroid(polys)
    geoms = X.polygon_geoms(polys)
    for g in range(len(geoms)):
        ec = X.exact_centroid(geoms[g])
        b = X.centroid_bound(geoms[g], ec)
        for ax in (0, 1):
            assert X.abs_err(c[g, ax], ec[ax]) <= b[ax] + np.spacing(abs(t[ax])), (g, ax)


@pytest.mark.parametrize("t", X.LATTICE_OFFSETS)
def test_translated_lines_lattice(oracle, t):
    z = _npz("lines_lattice.npz")
    l0 = GeoArrowArray(_abi.GEOM_LINESTRING, z["xy"], geom_offsets=z["geom_offsets"])
    q0 = GeoArrowArray.from_points(z["points"])
    lines, pts = X.translated_exactly(l0, t), X.translated_exactly(q0, t)
    assert np.array_equal(oracle.euclidean_length(lines), oracle.euclidean_length(l0))
    assert np.array_equal(oracle.distance_rowwise(pts, lines), oracle.distance_rowwise(q0, l0))
    assert np.array_equal(oracle.bounds(lines), z["bounds"] + [t[0], t[1], t[0], t[1]], equal_nan=True)
    assert np.array_equal(oracle.predicate_rowwise(lines, pts, "contains").astype(bool), z["contains"])
    c, ok = oracle.centroid(lines)
    assert np.array_equal(ok, z["centroid_valid"])
    # sum(mid * len) / sum(len): positive weights, nothing cancels, so the error is gamma(n + 4) of the centroid's magnitude
    # (a few ulps of T) plus the golden's own rounding of the exact value
    n = np.diff(z["geom_offsets"])[ok][:, None]
    tol = X.gamma(1) * (n + 4) * np.abs(c[ok]) + 1e-12 * 64
    assert np.all(np.abs(c[ok] - (z["centroid"][ok] + t)) <= tol)


@pytest.mark.parametrize("t", X.LATTICE_OFFSETS)
def test_translated_join_lattice(oracle, t):
    z = _npz("join_lattice.npz")
    polys = X.translated_exactly(GeoArrowArray(_abi.GEOM_POLYGON, z["xy"], geom_offsets=z["geom_offsets"], ring_offsets=z["ring_offsets"]), t)
    pts = X.translated_exactly(GeoArrowArray.from_points(z["points"]), t)
    for mode in (0, 1):
        pairs, _, _ = oracle.spatial_join(pts, polys, "intersects", mode=mode)
        assert np.array_equal(pairs, z["pairs"])


@pytest.mark.parametrize("k", [-60, 30, 100])
def test_scaled_contains_lattice(oracle, k):
    """contains_lattice's coordinates are nudged by 2^-50 (tests/lattice.py `nudged`): no translation keeps them exact, a power
    of two does"""
    from .lattice import load_contains_golden

    a, b, exp = load_contains_golden()
    exp_i = load_contains_golden(key="intersects")[2]
    a, b = X.scaled(a, k), X.scaled(b, k)
    assert np.array_equal(oracle.predicate_rowwise(a, b, "contains").astype(bool), exp)
    assert np.array_equal(oracle.predicate_rowwise(a, b, "intersects").astype(bool), exp_i)
