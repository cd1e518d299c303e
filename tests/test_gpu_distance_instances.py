"""GPU: every (family, G) instance of the point -> geometry distance kernels against exact answers.

Row-wise distance (distance_kernel<G, KIND>) and the nearest join (nearest_best_kernel / nearest_emit_kernel<G, KIND>) are compiled
once per right-side family and lane-group size G (1 / 8 / 32, from the right column's mean vertex count; POINT: 1).  Each fixture of
tests/exact_ref.py selects one instance (test_exact_distance_ref.py checks which).  Row-wise results must be within distance_bound
of the exact distance and agree with the oracle; the nearest join must return, bit for bit, the tie set that the per-row kernel's
own distances define: for left point l, every usable right row r with d[l, r] == min d[l, :], where d[l, :] is
gpk_distance_rowwise of n_right copies of l against the right column (b_rows NULL: never the grouped schedule)."""
import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries, RowMap
from geopolars_amd.spatial_index import SpatialIndex, nearest_pairs
from tests import exact_ref as X

pytestmark = pytest.mark.gpu


def _pts(xy):
    return GeoSeries(GeoArrowArray.from_points(np.asarray(xy, dtype=np.float64).reshape(-1, 2)))


def _check_rowwise(got, od, exact, what, grouped=False):
    """got (GPU), od (oracle), exact [(Decimal or None, bound)] of the same pairs.  The per-row kernel is within 1e-9 of the oracle
    relative; the grouped schedule evaluates a segment with other roundings, so for distances of a few ulps of the feature's extent
    (a point one ulp off a vertex) it is held to the exact bound instead: max(1e-9 |oracle|, twice the bound)."""
    assert len(got) == len(od) == len(exact)
    for i, (d, b) in enumerate(exact):
        if np.isnan(od[i]) or d is None:  # null or empty row: the oracle's convention, exactly
            assert (np.isnan(got[i]) and np.isnan(od[i])) or got[i] == od[i], (what, i, got[i], od[i])
            continue
        assert X.abs_err(got[i], d) <= b, (what, i, got[i], d, b)
        assert (got[i] == 0.0) == (od[i] == 0.0), (what, i, got[i], od[i])
        assert abs(got[i] - od[i]) <= max(1e-9 * abs(od[i]), 2 * b if grouped else 0.0), (what, i, got[i], od[i])


def _right(fx):
    if "series" not in fx:
        fx["series"] = GeoSeries(fx["array"])
    return fx["series"]


# ---- row-wise ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("family,G", X.INSTANCES)
def test_rowwise_instance_against_exact_distances(gpk, oracle, family, G):
    fx = X.instance_fixture(family, G)
    right, q = _right(fx), fx["queries"]
    n = len(q)
    exact = X.exact_rowwise(fx)
    got = _pts(q).distance(right)
    _check_rowwise(got, oracle.distance_rowwise(GeoArrowArray.from_points(q), fx["array"]), exact, "identity")
    # shuffled b_rows, with out-of-range entries: NaN
    rng = np.random.default_rng(G + 17 * fx["kind"])
    perm = rng.permutation(n)
    rows = np.concatenate([perm, [n, n + 5, 0xFFFFFFFF]]).astype(np.uint32)
    ql = np.concatenate([q[perm], rng.uniform(0, X.DOMAIN, (3, 2))])
    gs = _pts(ql).distance(right, other_rows=rows)
    assert np.isnan(gs[n:]).all()
    assert np.array_equal(gs[:n].view(np.uint64), got[perm].view(np.uint64))
    _check_rowwise(gs[:n], oracle.distance_rowwise(GeoArrowArray.from_points(q[perm]), fx["array"], b_rows=perm.astype(np.uint32)),
                   [exact[i] for i in perm], "shuffled")
    # mirrored: the geometry on the left
    gm = right.distance(_pts(q))
    assert np.array_equal(gm.view(np.uint64), got.view(np.uint64))


@pytest.mark.parametrize("G", [1, 8, 32])
def test_linestring_grouped_schedule_and_row_map(gpk, oracle, G):
    """8 rows per target: gpk_distance_rowwise takes the grouped schedule; gpk_distance_rowmap with a prepared map gives its bits"""
    fx = X.instance_fixture("linestring", G)
    right = _right(fx)
    n = len(fx["rows"])
    rng = np.random.default_rng(G)
    rows_of = rng.permutation(np.repeat(np.arange(n), 8)).astype(np.uint32)
    q = np.array([X._query(rng, fx["kind"], fx["rows"][j], fx["meta"][j], int(rng.integers(0, 6))) for j in rows_of])
    exact = X.exact_rowwise(fx, q, rows_of)
    got = _pts(q).distance(right, other_rows=rows_of)
    _check_rowwise(got, oracle.distance_rowwise(GeoArrowArray.from_points(q), fx["array"], b_rows=rows_of), exact, "grouped", grouped=True)
    rm = RowMap(right, rows_of)
    try:
        gr = _pts(q).distance(right, row_map=rm)
    finally:
        rm.free()
    assert np.array_equal(gr.view(np.uint64), got.view(np.uint64))


# ---- nearest join -------------------------------------------------------------------------------------------------------------------


def tie_reference(left_xy, right: GeoSeries, usable) -> np.ndarray:
    """d[l, r] from gpk_distance_rowwise's per-row kernel (n_right copies of l, b_rows NULL); inf for null and empty rows"""
    nr = len(usable)
    D = np.empty((len(left_xy), nr))
    for l, p in enumerate(np.asarray(left_xy, dtype=np.float64)):
        D[l] = _pts(np.repeat(p[None], nr, axis=0)).distance(right)
    D[:, ~np.asarray(usable, dtype=bool)] = np.inf
    return D


def expected_pairs(D, max_distance=np.inf):
    mins = D.min(axis=1)
    pairs, dist, counts = [], [], np.zeros(len(D), np.int64)
    for l in range(len(D)):
        if not (np.isfinite(mins[l]) and mins[l] <= max_distance):
            continue
        rs = np.flatnonzero(D[l] == mins[l])
        counts[l] = len(rs)
        pairs += [(l, int(r)) for r in rs]
        dist += [mins[l]] * len(rs)
    return np.array(pairs, np.int64).reshape(-1, 2), counts, np.array(dist, np.float64)


def assert_same_pairs(got, exp, what):
    (gp, gc, gd), (ep, ec, ed) = got, exp
    assert np.array_equal(gc.astype(np.int64), ec), (what, np.flatnonzero(gc.astype(np.int64) != ec)[:5])
    assert np.array_equal(gp.astype(np.int64), ep), what
    assert np.array_equal(gd.view(np.uint64), ed.view(np.uint64)), what


def check_nearest(left_xy, right: GeoSeries, usable, exact_min, indexes, D=None, max_distances=True):
    """every index gives the per-row kernel's tie set bit for bit; the minima are within bound of the exact minima; with max_distance
    at a row's own minimum the row is kept, one ulp below it dropped.  Returns D."""
    D = tie_reference(left_xy, right, usable) if D is None else D
    mins = D.min(axis=1)
    for l, (d, b) in enumerate(exact_min):
        if d is None:
            assert not np.isfinite(mins[l]), l
        else:
            assert X.abs_err(mins[l], d) <= b, (l, mins[l], d, b)
    left = _pts(left_xy)
    exp = expected_pairs(D)
    for name, ix in indexes.items():
        assert_same_pairs(nearest_pairs(left, right, r_index=ix), exp, name)
    if max_distances:
        pos = np.sort(mins[np.isfinite(mins) & (mins > 0)])
        if len(pos):
            md = float(pos[len(pos) // 2])
            for m in (md, float(np.nextafter(md, 0.0))):
                e = expected_pairs(D, m)
                assert (e[1][np.flatnonzero(mins == md)] > 0).all() == (m == md)
                assert_same_pairs(nearest_pairs(left, right, r_index=indexes.get("for_points=False"), max_distance=m), e, ("max_distance", m))
    return D


def _indexes(right: GeoSeries, kind: int):
    ix = {"none": None, "for_points=False": SpatialIndex(right, for_points=False)}
    if kind in X.POLYGONAL:
        ix["default"] = SpatialIndex(right)
        ix["full"] = SpatialIndex(right, full=True)
    return ix


@pytest.mark.parametrize("family,G", X.INSTANCES)
def test_nearest_instance_gives_the_rowwise_tie_set(gpk, family, G):
    fx = X.instance_fixture(family, G)
    right = _right(fx)
    D = check_nearest(fx["left"], right, fx["usable"], X.exact_nearest_minima(fx), _indexes(right, fx["kind"]))
    counts = (D == D.min(axis=1)[:, None]).sum(axis=1)
    assert (counts > 1).sum() >= 10, "the fixture has exact ties"


# ---- the search's edge cases ---------------------------------------------------------------------------------------------------------


def _fixture(kind, rows, validity=None):
    validity = [True] * len(rows) if validity is None else validity
    usable = np.array([v and not X.row_is_empty(kind, r) for r, v in zip(rows, validity)])
    return {"kind": kind, "rows": rows, "validity": validity, "usable": usable, "array": X.column(kind, rows, validity)}


def _run_edge_case(fx, left, G, exact_rows=None):
    """exact_rows: evaluate the exact minimum over these rows only (a column of identical rows)"""
    a = fx["array"]
    assert X.group_size_of(a) == G
    right = GeoSeries(a)
    left = np.asarray(left, dtype=np.float64)
    if exact_rows is None:
        exact_min = X.exact_nearest_minima(fx, left)
    else:
        sub = {"kind": fx["kind"], "rows": [fx["rows"][j] for j in exact_rows], "usable": fx["usable"][exact_rows]}
        exact_min = X.exact_nearest_minima(sub, left)
    return check_nearest(left, right, fx["usable"], exact_min, _indexes(right, fx["kind"]))


# Cell borders.  16 rows -> gdim = ceil(2 sqrt(16)) = 8 cells a side (gpk_index_build_ex); an extent of 8 * 4 puts every border on a
# multiple of 4: exact doubles, and (v - x0) * inv_w is exact, so a point on a border is exactly at a cell's edge.
X0, Y0, CW = 64.0, 32.0, 4.0


def _border_queries(rng):
    b = [X0 + CW * i for i in range(9)], [Y0 + CW * i for i in range(9)]
    q = [(x, y) for x in b[0] for y in b[1][::2]]  # cell corners, the max edges included
    q += [(x, float(rng.uniform(Y0, Y0 + 8 * CW))) for x in b[0]] + [(float(rng.uniform(X0, X0 + 8 * CW)), y) for y in b[1]]
    q += [(X0 + 8 * CW, Y0 + 8 * CW + 3.0), (X0 + 8 * CW + 2.5, Y0 + 4 * CW), (X0 - 1.0, Y0 - 1.0), (X0 + 8 * CW, Y0 - 7.0)]
    q += [tuple(rng.uniform((X0 - 4, Y0 - 4), (X0 + 8 * CW + 4, Y0 + 8 * CW + 4))) for _ in range(40)]
    return q


def _border_boxes(rng, n=16):
    """n boxes on cell borders (cells a0..a1 x b0..b1), the first two spanning the extent's corners"""
    out = [(0, 0, 2, 3), (5, 6, 8, 8)]
    while len(out) < n:
        a0, b0 = rng.integers(0, 7, 2)
        out.append((int(a0), int(b0), int(a0 + rng.integers(1, 9 - a0)), int(b0 + rng.integers(1, 9 - b0))))
    return [(X0 + CW * a0, Y0 + CW * b0, X0 + CW * a1, Y0 + CW * b1) for a0, b0, a1, b1 in out]


def test_cell_borders_linestring_g1(gpk):
    rng = np.random.default_rng(1)
    rows = [[(x0, y0), (x1, (y0 + y1) / 2), (x0, y1)] if k % 2 else [(x0, y0), (x1, y1)] for k, (x0, y0, x1, y1) in enumerate(_border_boxes(rng))]
    _run_edge_case(_fixture(_abi.GEOM_LINESTRING, rows), _border_queries(rng), 1)


def test_cell_borders_polygon_g8(gpk):
    rng = np.random.default_rng(2)
    rows = []
    for x0, y0, x1, y1 in _border_boxes(rng):
        m = 5  # 20 vertices a ring: G = 8
        ring = [(x0 + (x1 - x0) * i / m, y0) for i in range(m)] + [(x1, y0 + (y1 - y0) * i / m) for i in range(m)]
        ring += [(x1 - (x1 - x0) * i / m, y1) for i in range(m)] + [(x0, y1 - (y1 - y0) * i / m) for i in range(m)]
        rows.append([np.array(ring + ring[:1])])
    _run_edge_case(_fixture(_abi.GEOM_POLYGON, rows), _border_queries(rng), 8)


def test_cell_borders_multipoint_g32(gpk):
    rng = np.random.default_rng(3)
    rows = []
    for x0, y0, x1, y1 in _border_boxes(rng):
        pts = [(x0, y0), (x1, y1)] + [tuple(np.round(rng.uniform((x0, y0), (x1, y1)) * 4) / 4) for _ in range(198)]
        rows.append(pts)
    _run_edge_case(_fixture(_abi.GEOM_MULTIPOINT, rows), _border_queries(rng), 32)


# Degenerate axes: an extent of zero width or height has inv_w / inv_h = 0 and one usable column / row (NearGrid::ex / ey = 1).


def test_all_boxes_on_one_vertical_line(gpk):
    rng = np.random.default_rng(4)
    ys = rng.uniform(0, 500, 300)
    q = [(50.0, float(y)) for y in rng.uniform(-50, 550, 40)] + [tuple(rng.uniform((-100, -100), (200, 600))) for _ in range(80)]
    _run_edge_case(_fixture(_abi.GEOM_POINT, [(50.0, float(y)) for y in ys]), q, 1)
    rows = [[(50.0, float(y + 0.25 * k)) for k in range(40)] for y in ys[:100]]
    _run_edge_case(_fixture(_abi.GEOM_LINESTRING, rows), q, 8)


def test_all_boxes_on_one_horizontal_line(gpk):
    rng = np.random.default_rng(5)
    rows = [[(float(x), 20.0) for x in rng.uniform(0, 400, 200)] for _ in range(40)]
    q = [(float(x), 20.0) for x in rng.uniform(-50, 450, 30)] + [tuple(rng.uniform((-100, -300), (500, 300))) for _ in range(60)]
    _run_edge_case(_fixture(_abi.GEOM_MULTIPOINT, rows), q, 32)


def test_all_rows_identical_sorts_a_long_tie_slice(gpk):
    """3000 copies of one 200-vertex polygon: a point outside ties with all of them (lane 0's shell sort of 3000 right ids); so does
    every point of a column of 2500 identical points (both axes degenerate)"""
    rng = np.random.default_rng(6)
    ring = X._star(rng, 100.0, 100.0, 50.0, 200)
    rows = [[ring]] * 3000
    q = [tuple(rng.uniform(40, 160, 2)) for _ in range(24)] + [(100.0, 100.0), tuple(ring[7]), (100.0, 400.0), (-1e5, 3.0)]
    fx = _fixture(_abi.GEOM_POLYGON, rows)
    D = _run_edge_case(fx, q, 32, exact_rows=[0])
    outside = D.min(axis=1) > 0
    assert outside.sum() >= 3 and ((D == D.min(axis=1)[:, None]).sum(axis=1)[outside] == 3000).all()
    fx = _fixture(_abi.GEOM_POINT, [(3.5, -2.25)] * 2500)
    _run_edge_case(fx, [(3.5, -2.25), (0.0, 0.0), (1e6, 1e6)], 1, exact_rows=[0])


# Far queries: far outside the extent in all eight compass directions, with and without max_distance (check_nearest sets one).
@pytest.mark.parametrize("family,G", [("linestring", 8), ("polygon", 32), ("multipoint", 1), ("multipolygon", 8)])
def test_far_queries_in_all_eight_directions(gpk, family, G):
    fx = X.instance_fixture(family, G)
    c = X.DOMAIN / 2
    q = []
    for far in (3 * X.DOMAIN, 1e6 * X.DOMAIN):
        q += [(c + far * dx, c + far * dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if dx or dy]
        q += [(-far, 0.0), (far, X.DOMAIN), (0.0, -far), (X.DOMAIN, far)]
    _run_edge_case(fx, q, G)
    right = _right(fx)
    none = nearest_pairs(_pts(q), right, max_distance=X.DOMAIN)
    assert len(none[0]) == 0 and not none[1].any()


# Crowded cells: every cell lists more rows than G (rows spanning the extent), null rows (with coordinates: listed) and empty rows among
# them, so the candidate loop runs with partial groups; long rows are listed in many cells and must be evaluated once per query.


def _crowded(kind, G, rng, n=160):
    rows = []
    for i in range(n):
        a, b = rng.uniform(0, 200, 2), rng.uniform(800, 1000, 2)
        if i % 3 == 0:
            a, b = a, np.array([b[0], a[1] + 1000 * (i % 2)])  # diagonals and horizontals across the extent
        if kind == _abi.GEOM_MULTIPOINT:
            rows.append([tuple(a), tuple(b)] + [tuple(rng.uniform(0, 1000, 2)) for _ in range(int(rng.integers(0, 6)))])
        elif kind == _abi.GEOM_LINESTRING:
            t = np.linspace(0, 1, 40)[:, None]
            rows.append([tuple(c) for c in a + t * (b - a) + rng.normal(0, 3, (40, 2))])
        else:
            rows.append([X._star(rng, 500 + rng.uniform(-100, 100), 500 + rng.uniform(-100, 100), float(rng.uniform(600, 1200)), 200)])
        if i % 11 == 5:
            rows[-1] = []
    validity = [i % 7 != 2 for i in range(n)]
    return _fixture(kind, rows, validity)


@pytest.mark.parametrize("kind,G", [(_abi.GEOM_MULTIPOINT, 1), (_abi.GEOM_LINESTRING, 8), (_abi.GEOM_POLYGON, 32)])
def test_crowded_cells(gpk, kind, G):
    rng = np.random.default_rng(kind + G)
    fx = _crowded(kind, G, rng)
    q = [tuple(rng.uniform(-50, 1050, 2)) for _ in range(150)]
    good = np.flatnonzero(fx["usable"])
    for j in good[:40]:
        v = X._vertices(kind, fx["rows"][j])
        q.append(tuple(v[int(rng.integers(0, len(v)))]))
    spans = [np.ptp(np.asarray(X._vertices(kind, r)), axis=0).min() > 500 for r in fx["rows"] if len(r)]
    assert sum(spans) > 2 * G, "rows listed in many cells: more than G entries per cell"
    _run_edge_case(fx, q, G)
