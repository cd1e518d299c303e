"""GPU: linear referencing (gpk_closest_point_rowwise, gpk_line_locate_point, gpk_line_interpolate_point) against the exact
reference of tests/linref_ref.py: hand-made cases for all six right-side families, exact ties on lattice inputs for each lane-group
size, random columns, consistency with the distance and the nearest join, exact scaling by powers of two, device buffers."""
import ctypes as C

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import nearest_pairs
from tests import exact_ref as X
from tests import linref_ref as R

pytestmark = pytest.mark.gpu

PT, MP, LS, MLS, PG, MPG = (_abi.GEOM_POINT, _abi.GEOM_MULTIPOINT, _abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON,
                            _abi.GEOM_MULTIPOLYGON)
NAN = float("nan")


def _pts(xy, validity=None):
    bits = None if validity is None else np.packbits(np.asarray(validity, dtype=bool), bitorder="little")
    return GeoSeries(GeoArrowArray.from_points(np.asarray(xy, dtype=np.float64).reshape(-1, 2), validity=bits))


def _closest(points: GeoSeries, right: GeoSeries, rows=None):
    q, seg = points.closest_point(right, other_rows=rows, return_segment=True)
    return q.array.xy, seg, q.array.is_valid()


def check_closest(pts, col: GeoArrowArray, rows_of=None, validity=None, max_ambiguous=None, what=""):
    """closest_point (and, for lineal columns, project) of point i against row rows_of[i] of col, against the exact reference"""
    kind, rows = R.rows_of(col)
    right = GeoSeries(col)
    n = len(pts)
    idx = np.arange(n) if rows_of is None else np.asarray(rows_of)
    q, seg, ok = _closest(_pts(pts), right, None if rows_of is None else idx.astype(np.uint32))
    lineal = kind in (LS, MLS)
    if lineal:
        m = right.project(_pts(pts), rows=None if rows_of is None else idx.astype(np.uint32))
        mn = right.project(_pts(pts), normalized=True, rows=None if rows_of is None else idx.astype(np.uint32))
    n_amb = 0
    for i in range(n):
        j = int(idx[i])
        p = (float(pts[i][0]), float(pts[i][1]))
        usable = j < len(rows) and (validity is None or validity[j]) and not (np.isnan(p[0]) or np.isnan(p[1]))
        ex = R.closest(p, kind, rows[j]) if usable else None
        if ex is None:
            assert np.isnan(q[i]).all() and seg[i] == -1 and not ok[i], (what, i, q[i], seg[i])
            if lineal:
                assert np.isnan(m[i]) and np.isnan(mn[i]), (what, i)
            continue
        assert ok[i], (what, i)
        if ex["inside"]:
            assert seg[i] == -1 and q[i, 0] == p[0] and q[i, 1] == p[1], (what, i, q[i], seg[i])
            continue
        base = R.coord_base(col, j)
        if R.ambiguous(p, ex):
            n_amb += 1
            tol = R.Q_REL * max(abs(p[0]), abs(p[1]), max(abs(c) for sg in R.segments(kind, rows[j]) for c in (*sg[2], *sg[3])))
            assert R.on_some_segment((float(q[i, 0]), float(q[i, 1])), kind, rows[j], tol), (what, i, q[i])
            d = float(np.hypot(q[i, 0] - p[0], q[i, 1] - p[1]))
            e = float(R.dec_sqrt(ex["d2"]))
            assert abs(d - e) <= 1e-9 * e, (what, i, d, e)
            continue
        assert seg[i] == base + ex["seg"], (what, i, seg[i], base, ex["seg"])
        b = R.q_bound(p, ex["s"], ex["e"])
        assert R.dec_err(q[i, 0], ex["q"][0]) <= b and R.dec_err(q[i, 1], ex["q"][1]) <= b, (what, i, q[i], ex["q"], b)
        if ex["t"] == 0:
            assert tuple(q[i]) == ex["s"], (what, i)
        if ex["t"] == 1:
            assert tuple(q[i]) == ex["e"], (what, i)
        if lineal:
            L = float(R.total_length(kind, rows[j]))
            assert R.dec_err(m[i], R.measure(kind, rows[j], ex)) <= R.M_REL * L, (what, i, m[i])
            if L > 0:
                assert R.dec_err(mn[i], R.measure(kind, rows[j], ex, normalized=True)) <= R.M_REL, (what, i, mn[i])
            else:
                assert mn[i] == 0.0, (what, i)
    if max_ambiguous is not None:
        assert n_amb <= max_ambiguous, (what, n_amb, n)
    return q, seg


# ---- hand-made cases ------------------------------------------------------------------------------------------------------------

RING = [(0.0, 0.0), (8.0, 0.0), (8.0, 8.0), (0.0, 8.0), (0.0, 0.0)]
HOLE = [(2.0, 2.0), (2.0, 6.0), (6.0, 6.0), (6.0, 2.0), (2.0, 2.0)]
FAR = [(14.0, 0.0), (20.0, 0.0), (20.0, 8.0), (14.0, 8.0), (14.0, 0.0)]
HAND = {
    PT: [(3.0, 4.0), None, (1.0, 1.0), (-2.0, 5.0)],
    MP: [[(3.0, 4.0), (-3.0, 4.0), (1.0, 1.0)], [], [(5.0, 5.0)], [(3.0, 4.0), (-3.0, 4.0)]],
    LS: [[(0.0, 0.0), (10.0, 0.0), (10.0, 10.0)], [], [(1.0, 2.0), (1.0, 2.0)], [(0.0, 0.0), (3.0, 4.0), (6.0, 0.0)], [(7.0, 7.0)], RING],
    MLS: [[[(0.0, 0.0), (3.0, 0.0)], [], [(100.0, 0.0), (100.0, 4.0)], [(7.0, 7.0)], [(200.0, 0.0), (203.0, 4.0)]], [], [[], []],
          [[(1.0, 2.0)], [(5.0, 5.0)]], [RING, HOLE]],
    PG: [[RING, HOLE], [], [RING], [FAR, [(15.0, 1.0), (15.0, 3.0), (17.0, 3.0), (17.0, 1.0), (15.0, 1.0)]]],
    MPG: [[[RING, HOLE], [FAR]], [], [[RING]], [[FAR], [RING, HOLE]]],
}
PROBES = [(3.0, 4.0), (4.0, 3.0), (1.0, 1.0), (8.0, 3.0), (2.0, 3.0), (11.0, 4.0), (-3.0, -4.0), (9.0, -4.0), (101.0, 1.0), (7.0, 8.0),
          (204.0, 5.0), (16.0, 2.0), (0.0, 0.0), (13.0, 6.0), (NAN, 1.0), (1.0, NAN), (5.5, -1.0), (4.0, 4.0), (15.0, 2.0), (0.5, 7.5)]


@pytest.mark.parametrize("kind", [PT, MP, LS, MLS, PG, MPG])
def test_hand_made_cases_every_family(gpk, kind):
    rows = HAND[kind]
    validity = [True] * len(rows)
    validity[-1] = False  # a null row that keeps its coordinates
    rows = rows + [rows[0]]
    validity = validity + [True]
    col = X.column(kind, rows, validity)
    n = len(rows)
    pts = [p for p in PROBES for _ in range(n)]
    rows_of = [j for _ in PROBES for j in range(n)]
    # out-of-range row numbers behave like null rows
    pts += [(1.0, 1.0)] * 3
    rows_of += [n, n + 7, 0xFFFFFFFF]
    q, seg = check_closest(np.array(pts), col, rows_of=np.array(rows_of, dtype=np.int64).clip(0, None), validity=validity, what=f"hand {kind}")
    assert np.isnan(q[-3:]).all() and (seg[-3:] == -1).all()
    # a null point
    qq, ss, ok = _closest(_pts([(1.0, 1.0)] * n, validity=[False] * n), GeoSeries(col))
    assert np.isnan(qq).all() and (ss == -1).all() and not ok.any()


def test_hand_made_interpolate(gpk):
    cases = {
        LS: (HAND[LS], [0.0, 2.5, 5.0, 8.0, -3.0, -11.0, -40.0, 11.0, 1e9, 20.0, 10.0, NAN, np.inf, -np.inf, -0.0]),
        MLS: (HAND[MLS], [0.0, 3.0, 3.5, 7.0, 9.5, 12.0, 13.0, -5.0, -12.0, 32.0, 40.0, NAN, np.inf]),
    }
    for kind, (rows, ds) in cases.items():
        validity = [True] * len(rows)
        validity[-1] = False
        rows = rows + [rows[-1]]
        validity = validity + [True]
        s = GeoSeries(X.column(kind, rows, validity))
        for normalized in (False, True):
            for d in ds + [0.25, 0.5, 1.0, -0.25, 1.5]:
                out = s.interpolate(d, normalized=normalized)
                arr = s.interpolate(np.full(len(rows), d), normalized=normalized)
                assert np.array_equal(out.array.xy.view(np.uint64), arr.array.xy.view(np.uint64)), (kind, d)  # scalar == array form
                assert np.array_equal(out.array.is_valid(), arr.array.is_valid())
                for j, row in enumerate(rows):
                    ex = R.interpolate(kind, row, d, normalized) if validity[j] else None
                    g = out.array.xy[j]
                    if ex is None:
                        assert np.isnan(g).all() and not out.array.is_valid()[j], (kind, d, j, g)
                        continue
                    assert out.array.is_valid()[j]
                    L = float(R.total_length(kind, row))
                    assert R.dec_err(g[0], ex[0]) <= R.M_REL * L and R.dec_err(g[1], ex[1]) <= R.M_REL * L, (kind, normalized, d, j, g, ex)
    # a measure that lands exactly on a vertex returns that vertex bit for bit; a member boundary gives the end of the earlier member
    s = GeoSeries(X.column(MLS, [HAND[MLS][0]] * 4))
    got = s.interpolate([3.0, 7.0, 12.0, 0.0]).array.xy
    assert got.tolist() == [[3.0, 0.0], [100.0, 4.0], [203.0, 4.0], [0.0, 0.0]]
    # a per-row distance array with nulls
    s = GeoSeries(X.column(LS, [HAND[LS][3]] * 3))
    out = s.interpolate([2.5, NAN, -2.5])
    assert out.array.is_valid().tolist() == [True, False, True] and out.array.xy[0].tolist() == [1.5, 2.0] and out.array.xy[2].tolist() == [4.5, 2.0]


def test_shortest_line(gpk):
    col = X.column(PG, [[RING, HOLE], [], [RING]])
    s = _pts([(11.0, 4.0), (1.0, 1.0), (1.0, 1.0)]).shortest_line(GeoSeries(col))
    a = s.array
    assert a.geom_type == LS and a.geom_offsets.tolist() == [0, 2, 4, 6] and a.is_valid().tolist() == [True, False, True]
    assert a.xy[:2].tolist() == [[11.0, 4.0], [8.0, 4.0]] and a.xy[4:].tolist() == [[1.0, 1.0], [1.0, 1.0]]


# ---- exact ties on lattice inputs, one column per lane-group size --------------------------------------------------------------
# Coordinates are integers of magnitude <= 64: differences < 2^8, cross^2 < 2^32, d2 < 2^16, so every product of frac_less is an exact
# double and f64 ties are exactly the rational ties.  Every sequence is laid out twice (and parts are repeated), so every minimum
# is tied between segments that fall to different lanes: the lowest coordinate index must win for G = 1, 8 and 32.


def _lattice_walk(rng, n):
    xy = np.clip(np.cumsum(rng.integers(-6, 7, (n, 2)), axis=0) + rng.integers(-20, 21, 2), -60, 60)
    return [(float(x), float(y)) for x, y in xy]


def _lattice_row(rng, kind, k):
    if kind == MP:
        w = _lattice_walk(rng, max(1, k // 2))
        return w + w
    if kind == LS:
        w = _lattice_walk(rng, max(2, k // 2))
        return w + w
    if kind == MLS:
        w = _lattice_walk(rng, max(2, k // 3))
        return [w, [w[0]], w, w[::-1]]
    ring = _lattice_walk(rng, max(3, k // 2 - 1))
    ring = ring + ring[:1]
    if kind == PG:
        return [ring, ring]  # (the "hole" repeats the exterior: every point not outside it is on it or in it)
    return [[ring], [ring]]


@pytest.mark.parametrize("G", [1, 8, 32])
@pytest.mark.parametrize("kind", [MP, LS, MLS, PG, MPG])
def test_exact_ties_take_the_lowest_index_in_every_instance(gpk, kind, G):
    rng = np.random.default_rng(1000 * kind + G)
    lo, hi = X._VERTS[G]
    n = {1: 120, 8: 60, 32: 30}[G]
    rows = [_lattice_row(rng, kind, int(rng.integers(lo, hi + 1))) for _ in range(n)]
    col = X.column(kind, rows)
    assert X.group_size_of(col) == G  # the instance that runs (gpk_distance.h distance_group_size, restated in exact_ref)
    pts = rng.integers(-64, 65, (3 * n, 2)).astype(np.float64)
    rows_of = np.tile(np.arange(n), 3)
    right = GeoSeries(col)
    q, seg, ok = _closest(_pts(pts), right, rows_of.astype(np.uint32))
    _, rr = R.rows_of(col)
    tied = 0
    for i in range(len(pts)):
        p = (float(pts[i, 0]), float(pts[i, 1]))
        ex = R.closest(p, kind, rr[rows_of[i]])
        if ex["inside"]:
            assert seg[i] == -1 and tuple(q[i]) == p, (i, seg[i])
            continue
        tied += sum(1 for s, d2, _ in ex["near"] if d2 == ex["d2"]) > 1
        assert seg[i] == R.coord_base(col, int(rows_of[i])) + ex["seg"], (kind, G, i, seg[i], ex["seg"])
        b = R.q_bound(p, ex["s"], ex["e"])
        assert R.dec_err(q[i, 0], ex["q"][0]) <= b and R.dec_err(q[i, 1], ex["q"][1]) <= b
    assert tied >= len(pts) // 4  # the ties are really there
    if kind in (LS, MLS):
        m = right.project(_pts(pts), rows=rows_of.astype(np.uint32))
        for i in range(len(pts)):
            ex = R.closest((float(pts[i, 0]), float(pts[i, 1])), kind, rr[rows_of[i]])
            L = float(R.total_length(kind, rr[rows_of[i]]))
            assert R.dec_err(m[i], R.measure(kind, rr[rows_of[i]], ex)) <= R.M_REL * L, (kind, G, i)


# ---- random columns --------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["linestrings", "multilinestrings", "star_polygons", "clustered_polygons", "powerlaw_multipolygons"])
def test_random_columns_against_the_exact_reference(gpk, name):
    col, pts = R.random_columns()[name]
    check_closest(pts, col, max_ambiguous=0.01 * len(pts), what=name)


def test_random_multipoints_against_the_exact_reference(gpk):
    rng = np.random.default_rng(5)
    rows = [[tuple(c) for c in rng.uniform(0, 1000, (int(rng.integers(1, 40)), 2))] for _ in range(150)]
    rows[7] = []
    check_closest(rng.uniform(0, 1000, (150, 2)), X.column(MP, rows), max_ambiguous=1, what="multipoints")


# ---- consistency ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["linestrings", "multilinestrings", "clustered_polygons", "powerlaw_multipolygons"])
def test_closest_point_lies_at_the_rowwise_distance(gpk, name):
    col, pts = R.random_columns()[name]
    P, S = _pts(pts), GeoSeries(col)
    q, seg, ok = _closest(P, S)
    d = P.distance(S)
    h = np.hypot(q[:, 0] - pts[:, 0], q[:, 1] - pts[:, 1])
    nz = d > 0
    assert nz.any() and np.all(np.abs(h[nz] - d[nz]) <= 1e-9 * d[nz])
    assert np.all(h[(d == 0) & ok] <= 1e-9 * np.abs(pts[(d == 0) & ok]).max(axis=1))  # on the geometry (a linestring's EPSILON rule)


def test_closest_point_of_the_nearest_join_lies_at_the_joins_distance(gpk):
    col, _ = R.random_columns()["linestrings"]
    pts = np.random.default_rng(3).uniform(0, 1000, (500, 2))
    P, S = _pts(pts), GeoSeries(col)
    pairs, counts, dist = nearest_pairs(P, S)
    l, r = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.uint32)
    q, seg, ok = _closest(_pts(pts[l]), S, r)
    h = np.hypot(q[:, 0] - pts[l, 0], q[:, 1] - pts[l, 1])
    assert len(l) >= 500 and ok.all() and np.all(np.abs(h - dist) <= 1e-9 * dist)
    m = S.project(_pts(pts[l]), rows=r)  # the chain of the worked example: nearest_pairs -> closest_point -> project
    length = S.euclidean_length()[r]
    assert np.all((m >= 0) & (m <= length * (1 + 1e-12)))


@pytest.mark.parametrize("name", ["linestrings", "multilinestrings"])
def test_interpolate_of_project_is_the_closest_point(gpk, name):
    col, pts = R.random_columns()[name]
    kind, rows = R.rows_of(col)
    P, S = _pts(pts), GeoSeries(col)
    q, seg, ok = _closest(P, S)
    L = S.euclidean_length()
    # The measure is not one-to-one at a member boundary of a MULTILINESTRING: the end of a member and the start of the next one
    # share a measure (the gap has no length).  interpolate answers that measure with the end of the EARLIER member, and a measure
    # one rounding above it with the start of the later one.  locate sums the lengths in another order than interpolate (strided
    # lanes and a group sum against chunk prefixes: the summation order is free), so its measure of a point ON the boundary is the
    # boundary measure up to a rounding in either direction, far inside the 1e-9 L of its contract.  Where the closest point is the
    # end vertex of a member that has a successor, or the start vertex of a member that has a predecessor, the round trip may
    # therefore land on either side of the gap: both ends of the gap are accepted there, each within the bound, and nowhere else.
    # Members are contiguous in the coordinate buffer and none of these columns has an empty member: the gap after coordinate c
    # is (c, c + 1).
    starts = set() if kind == LS else set(int(c) for c in col.ring_offsets[:-1]) - set(R.coord_base(col, j) for j in range(len(col)))
    other = q.copy()
    at_gap = np.zeros(len(S), dtype=bool)
    for i in range(len(S)):
        sg = int(seg[i])
        if sg in starts and tuple(q[i]) == tuple(col.xy[sg]):  # the start of a later member: the earlier one ends at sg - 1
            at_gap[i], other[i] = True, col.xy[sg - 1]
        elif sg >= 0 and sg + 2 in starts and tuple(q[i]) == tuple(col.xy[sg + 1]):  # the end of a member: the next starts at sg + 2
            at_gap[i], other[i] = True, col.xy[sg + 2]
    for normalized in (False, True):
        back = S.interpolate(S.project(P, normalized=normalized), normalized=normalized).array.xy
        # the measure carries 1e-9 L (locate) and the point another 1e-9 L (interpolate)
        tol = 2 * R.M_REL * L + R.Q_REL * np.abs(q).max(axis=1)
        good = (np.abs(back - q).max(axis=1) <= tol) | (np.abs(back - other).max(axis=1) <= tol)
        assert good.all(), (name, normalized, np.flatnonzero(~good)[:5])
    assert kind == LS or at_gap.any()
    # scalar and array forms agree bit for bit
    for d in (0.0, 3.25, -7.5, 1e6):
        a, b = S.interpolate(d).array.xy, S.interpolate(np.full(len(S), d)).array.xy
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # random measures against the exact interpolate
    rng = np.random.default_rng(9)
    d = rng.uniform(-0.2, 1.2, len(S)) * L * rng.choice([1.0, -1.0], len(S))
    got = S.interpolate(d).array.xy
    for j in range(0, len(S), 3):
        ex = R.interpolate(kind, rows[j], float(d[j]))
        assert R.dec_err(got[j, 0], ex[0]) <= R.M_REL * L[j] and R.dec_err(got[j, 1], ex[1]) <= R.M_REL * L[j], (name, j)


# ---- exact scaling by powers of two at georeferenced placements ------------------------------------------------------------------


@pytest.mark.parametrize("k", [-100, -20, 20, 100])
def test_results_scale_exactly_by_powers_of_two(gpk, k):
    geoms = X.buildings(200, seed=16)  # UTM- and Web-Mercator-placed features
    polys = X.to_array(geoms)
    ls = [r for g in geoms[:80] for r in g[0]]
    lines = GeoArrowArray.from_linestrings([np.concatenate([r, r[:3] + 0.37]).tolist() for r in ls])
    mls = R.grouped_lines(lines, 4)
    pts, rows = X.probe_points(geoms, seed=17)
    P = GeoArrowArray.from_points(pts)

    def ops(polys, lines, mls, P):
        p = GeoSeries(P)
        out = {}
        for name, col in (("polys", polys), ("lines", lines), ("mls", mls)):
            s = GeoSeries(col)
            r = (rows % len(col)).astype(np.uint32)
            q, seg = p.closest_point(s, other_rows=r, return_segment=True)
            out[name] = (q.array.xy, seg)
            if name != "polys":
                out[name + "_m"] = s.project(p, rows=r)
                out[name + "_mn"] = s.project(p, normalized=True, rows=r)
                out[name + "_i"] = s.interpolate(0.37, normalized=True).array.xy
        return out

    base = ops(polys, lines, mls, P)
    got = ops(X.scaled(polys, k), X.scaled(lines, k), X.scaled(mls, k), X.scaled(P, k))
    for name in ("polys", "lines", "mls"):
        assert np.array_equal(got[name][1], base[name][1]), name
        assert np.array_equal(got[name][0], np.ldexp(base[name][0], k), equal_nan=True), name
    for name in ("lines", "mls"):
        assert np.array_equal(got[name + "_m"], np.ldexp(base[name + "_m"], k), equal_nan=True), name
        assert np.array_equal(got[name + "_mn"], base[name + "_mn"], equal_nan=True), name
        assert np.array_equal(got[name + "_i"], np.ldexp(base[name + "_i"], k), equal_nan=True), name
    assert (base["polys"][1] >= 0).any() and np.isfinite(base["lines_m"]).all()


# ---- device buffers ------------------------------------------------------------------------------------------------------------


def test_device_buffers_give_the_bytes_of_host_buffers(gpk):
    import torch

    lib = _abi.lib()
    col, pts = R.random_columns()["multilinestrings"]
    n = len(col)
    rng = np.random.default_rng(2)
    rows = rng.integers(0, n + 3, n).astype(np.uint32)  # (some out of range)
    P, S = _pts(pts), GeoSeries(col)
    hq, hseg, _ = _closest(P, S, rows)
    hm = S.project(P, rows=rows)
    dist = rng.uniform(-50, 300, n)
    hi, hs = S.interpolate(dist), S.interpolate(12.5, normalized=False)
    dev = "cuda:0"
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    t_rows = torch.from_numpy(rows.view(np.int32)).to(dev)
    xy = torch.full((n, 2), -1.0, dtype=torch.float64, device=dev)
    seg = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _abi.check(lib.gpk_closest_point_rowwise(P.device().handle, S.device().handle, ptr(t_rows), ptr(xy), ptr(seg), _abi.MEM_DEVICE, stream))
    torch.cuda.synchronize()
    assert np.array_equal(xy.cpu().numpy(), hq, equal_nan=True) and np.array_equal(seg.cpu().numpy(), hseg)
    _abi.check(lib.gpk_closest_point_rowwise(P.device().handle, S.device().handle, ptr(t_rows), ptr(xy), None, _abi.MEM_DEVICE, stream))  # no segments asked
    m = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    _abi.check(lib.gpk_line_locate_point(P.device().handle, S.device().handle, ptr(t_rows), 0, ptr(m), _abi.MEM_DEVICE, stream))
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy(), hm, equal_nan=True)
    valid = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    t_dist = torch.from_numpy(dist).to(dev)
    _abi.check(lib.gpk_line_interpolate_point(S.device().handle, ptr(t_dist), n, 0, ptr(xy), ptr(valid), _abi.MEM_DEVICE, stream))
    torch.cuda.synchronize()
    assert np.array_equal(xy.cpu().numpy(), hi.array.xy, equal_nan=True) and np.array_equal(valid.cpu().numpy().astype(bool), hi.array.is_valid())
    one = torch.tensor([12.5], dtype=torch.float64, device=dev)  # one device value for every row: read in place
    _abi.check(lib.gpk_line_interpolate_point(S.device().handle, ptr(one), 1, 0, ptr(xy), None, _abi.MEM_DEVICE, stream))
    torch.cuda.synchronize()
    assert np.array_equal(xy.cpu().numpy(), hs.array.xy, equal_nan=True)


def test_abi_refusals(gpk):
    lib = _abi.lib()
    P, S = _pts([(0.0, 0.0), (1.0, 1.0)]), GeoSeries(X.column(LS, [HAND[LS][0], HAND[LS][3]]))
    out = np.empty(4)
    d = np.zeros(3)
    assert lib.gpk_line_interpolate_point(S.device().handle, d.ctypes.data, 3, 0, out.ctypes.data, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    assert lib.gpk_line_interpolate_point(P.device().handle, d.ctypes.data, 1, 0, out.ctypes.data, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    assert lib.gpk_closest_point_rowwise(S.device().handle, P.device().handle, None, out.ctypes.data, None, _abi.MEM_HOST, None) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    assert lib.gpk_line_locate_point(P.device().handle, P.device().handle, None, 0, out.ctypes.data, _abi.MEM_HOST, None) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    one = GeoSeries(X.column(LS, [HAND[LS][0]]))
    assert lib.gpk_line_locate_point(P.device().handle, one.device().handle, None, 0, out.ctypes.data, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
