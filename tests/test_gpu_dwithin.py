"""GPU: within-distance join and row-wise dwithin (gpk_dwithin_join / gpk_dwithin_rowwise, csrc/gpk_dwithin.hip) — exact, no tolerances.

  1. against the library's own distance, bit for bit: the matrix D[l, r] from gpk_distance_rowwise's per-row kernels (rotated row maps;
     n_left < 8 * n_right, so the LINESTRING grouped schedule is never chosen) and, per threshold, pairs == {D <= t}, counts, distances;
  2. against the exact reference (tests/dwithin_ref.py) on the same fixtures: tests/test_dwithin_ref.py proves that no pair is within
     the distance bound of a threshold, so the sets are compared exactly;
  3. closedness on exactly representable distances; 4. candidate superset (boxes exactly t apart, georeferenced placements, grown boxes
     against the grid's border, a degenerate grid axis, wide right rows, the three candidate regimes); 5. rules (null / empty / NaN rows,
     empty columns, out-of-range b_rows, symmetry, table joins); 6. relations to the nearest join and the intersects join; 7. determinism."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest
import torch

from geopolars_amd import _abi
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import (
    SpatialIndex,
    SpatialJoinDWithinArgs,
    dwithin_pairs,
    dwithin_pairs_device,
    join_indices,
    join_pairs,
    nearest_pairs,
    spatial_join_dwithin,
    take_column,
)
from tests import dwithin_ref as W
from tests import exact_ref as X

pytestmark = pytest.mark.gpu

PT, MP, LS, MLS, PG, MPG = W.PT, W.MP, W.LS, W.MLS, W.PG, W.MPG


def _sq(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]


def series(col):
    return GeoSeries(X.column(*col))


def usable(col):
    kind, rows, v = col
    return np.array([W.row_usable(kind, r, v is None or v[i]) for i, r in enumerate(rows)])


def distance_matrix(left, right, sl=None, sr=None):
    """D[l, r] of gpk_distance_rowwise's per-row kernels (NaN where a row is null, empty or a NaN point)"""
    sl, sr = sl or series(left), sr or series(right)
    nl, nr = len(left[1]), len(right[1])
    D = np.full((nl, nr), np.nan)
    if left[0] != PT and right[0] == PT:  # b_rows needs the POINT column on the left: the mirrored call
        assert nr < 8 * nl
        for k in range(nl):
            rows = ((np.arange(nr) + k) % nl).astype(np.uint32)
            D[rows, np.arange(nr)] = sr.distance(sl, other_rows=rows)
    else:
        assert nl < 8 * nr
        for k in range(nr):
            rows = ((np.arange(nl) + k) % nr).astype(np.uint32)
            D[np.arange(nl), rows] = sl.distance(sr, other_rows=rows)
    D[~usable(left), :] = np.nan  # (the point kernels give 0.0 against an empty linestring: never matched)
    D[:, ~usable(right)] = np.nan
    return D


def expected(D, t):
    ll, rr = np.nonzero(D <= t)  # (row-major: sorted by (l, r); NaN compares false)
    return np.stack([ll, rr], axis=1).astype(np.uint32), np.bincount(ll, minlength=D.shape[0]).astype(np.uint32), D[ll, rr]


def check_against_matrix(left, right, D, sl, sr, thresholds):
    idx = SpatialIndex(sr, for_points=False)
    lib = _abi.lib()
    for t in thresholds:
        p0, c0, d0 = expected(D, t)
        for ix in (None, idx):
            pairs, counts, dist = dwithin_pairs(sl, sr, t, r_index=ix)
            assert np.array_equal(pairs, p0), (t, len(pairs), len(p0))
            assert np.array_equal(counts, c0), t
            assert dist.tobytes() == d0.tobytes(), t
    # device outputs, count-only, capacity error and left_row_base at the median threshold
    t = thresholds[2]
    p0, c0, d0 = expected(D, t)
    n = C.c_int64(-1)
    assert lib.gpk_dwithin_join(sl.device().handle, sr.device().handle, idx.handle, t, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_OK
    assert n.value == len(p0)
    counts = torch.full((len(c0),), -1, dtype=torch.int32, device="cuda:0")
    assert dwithin_pairs_device(sl.device(), sr.device(), None, t, counts, None) == len(p0)
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy().astype(np.uint32), c0)
    pairs = torch.zeros((len(p0) + 3, 2), dtype=torch.int32, device="cuda:0")
    dist = torch.zeros(len(p0) + 3, dtype=torch.float64, device="cuda:0")
    assert dwithin_pairs_device(sl.device(), sr.device(), idx, t, counts, pairs, dist, left_row_base=1000) == len(p0)
    torch.cuda.synchronize()
    got = pairs.cpu().numpy().astype(np.uint32)[: len(p0)]
    assert np.array_equal(got, p0 + np.array([1000, 0], dtype=np.uint32))
    assert dist.cpu().numpy()[: len(p0)].tobytes() == d0.tobytes()
    if len(p0) > 1:
        small = np.zeros((len(p0) - 1, 2), dtype=np.uint32)
        n = C.c_int64(-1)
        rc = lib.gpk_dwithin_join(sl.device().handle, sr.device().handle, None, t, 0, None, small.ctypes.data, None, len(small), C.byref(n), _abi.MEM_HOST, None)
        assert rc == _abi.GPK_ERR_CAPACITY and n.value == len(p0)
    idx.free()


def quantile_thresholds(D):
    fin = D[np.isfinite(D)]
    assert len(fin) > 10
    return [0.0, float(np.quantile(fin, 0.1, method="lower")), float(np.quantile(fin, 0.5, method="lower")), float(np.quantile(fin, 0.9, method="lower")), float(fin.max())]


# ---- 1 + 2: every ordered pair of families, every kernel instance ----------------------------------------------------------------


@pytest.mark.parametrize("key", W.POINT_FIXTURES, ids=lambda k: f"{k[0]}-G{k[1]}-{'pl' if k[2] else 'pr'}")
def test_point_pairs_against_own_distance_and_exact_reference(gpk, key):
    left, right = W.point_fixture(*key)
    sl, sr = series(left), series(right)
    assert X.group_size_of((sr if key[2] else sl).array) == key[1]
    D = distance_matrix(left, right, sl, sr)
    check_against_matrix(left, right, D, sl, sr, quantile_thresholds(D))
    table = W.fixture_table(key)
    for t in W.THRESHOLDS:
        within, close = W.classify(table, t)
        assert close == []
        pairs, counts, _ = dwithin_pairs(sl, sr, t)
        assert [tuple(p) for p in pairs.tolist()] == within, (key, t)
        assert int(counts.sum()) == len(within)


@pytest.mark.parametrize("key", W.PAIR_INSTANCES, ids=lambda k: f"{k[0]}x{k[1]}-{k[2]}")
def test_non_point_pairs_against_own_distance(gpk, key):
    left, right = W.pair_fixture(*key)
    sl, sr = series(left), series(right)
    D = distance_matrix(left, right, sl, sr)
    check_against_matrix(left, right, D, sl, sr, quantile_thresholds(D))


@pytest.mark.parametrize("key", W.PAIR_FIXTURES, ids=lambda k: f"{k[0]}x{k[1]}-{k[2]}")
def test_non_point_pairs_against_exact_reference(gpk, key):
    left, right = W.pair_fixture(*key)
    sl, sr = series(left), series(right)
    table = W.fixture_table(key)
    for t in W.THRESHOLDS:
        within, close = W.classify(table, t, exact_zero=True)
        assert close == []
        pairs, _, _ = dwithin_pairs(sl, sr, t)
        assert [tuple(p) for p in pairs.tolist()] == within, (key, t)


# ---- 3: closedness on exactly representable distances ----------------------------------------------------------------------------

# (name, left column, right column, exact distance of pair (0, 0)): 3-4-5 vertex gaps and axis-parallel gaps against segments of
# power-of-two length
CLOSED = [
    ("pt_pt", (PT, [(0.0, 0.0)], None), (PT, [(3.0, 4.0)], None), 5.0),
    ("pt_mp", (PT, [(1.0, 1.0)], None), (MP, [[(40.0, 40.0), (4.0, 5.0)]], None), 5.0),
    ("pt_ls", (PT, [(1.0, 3.0)], None), (LS, [[(0.0, 0.0), (4.0, 0.0)]], None), 3.0),
    ("ls_pt", (LS, [[(0.0, 0.0), (4.0, 0.0)]], None), (PT, [(7.0, 4.0)], None), 5.0),
    ("pt_pg", (PT, [(-2.0, 1.0)], None), (PG, [[_sq(0.0, 0.0, 2.0, 2.0)]], None), 2.0),
    ("mpg_pt", (MPG, [[[_sq(0.0, 0.0, 2.0, 2.0)], [_sq(10.0, 0.0, 12.0, 2.0)]]], None), (PT, [(6.0, 1.0)], None), 4.0),
    ("ls_ls", (LS, [[(0.0, 0.0), (8.0, 0.0)]], None), (LS, [[(2.0, 1.5), (6.0, 1.5)]], None), 1.5),
    ("mls_pg", (MLS, [[[(0.0, 0.0), (0.0, 2.0)], [(100.0, 0.0), (100.0, 1.0)]]], None), (PG, [[_sq(3.0, 6.0, 5.0, 8.0)]], None), 5.0),
    ("pg_mpg", (PG, [[_sq(0.0, 0.0, 4.0, 4.0)]], None), (MPG, [[[_sq(4.75, 1.0, 6.0, 2.0)]]], None), 0.75),
    ("mp_ls", (MP, [[(0.0, 0.0), (20.0, 20.0)]], None), (LS, [[(23.0, 24.0), (30.0, 30.0)]], None), 5.0),
]


@pytest.mark.parametrize("case", CLOSED, ids=[c[0] for c in CLOSED])
def test_threshold_is_closed(gpk, case):
    _, left, right, d = case
    sl, sr = series(left), series(right)
    assert distance_matrix(left, right, sl, sr)[0, 0] == d  # the distance itself is exact here
    assert W.exact_table(left, right)[(0, 0)][0] == d * d
    for a, b in ((sl, sr), (sr, sl)):
        pairs, counts, dist = dwithin_pairs(a, b, d)
        assert pairs.tolist() == [[0, 0]] and counts.tolist() == [1] and dist.tolist() == [d]
        pairs, counts, _ = dwithin_pairs(a, b, float(np.nextafter(d, 0.0)))
        assert len(pairs) == 0 and counts.tolist() == [0]
        assert a.dwithin(b, d).tolist() == [True] and a.dwithin(b, float(np.nextafter(d, 0.0))).tolist() == [False]


def test_zero_distance_is_touching_crossing_or_contained(gpk):
    ulp_y = float(np.nextafter(1.0, 2.0))
    left = (LS, [[(1.0, 1.0), (1.0, 5.0)], [(1.0, ulp_y), (1.0, 5.0)], [(2.0, 2.0), (3.0, 3.0)], [(0.0, 9.0), (9.0, 0.0)]], None)
    right = (PG, [[_sq(0.0, -1.0, 4.0, 1.0)], [_sq(1.5, 1.5, 8.0, 8.0), _sq(1.75, 1.75, 3.5, 3.5)[::-1]]], None)
    want = W.dwithin_exact(left, right, 0.0)
    assert want == [(0, 0), (3, 1)]  # touching an edge; crossing.  One ulp above the edge and inside the hole: not returned
    pairs, _, dist = dwithin_pairs(series(left), series(right), 0.0)
    assert [tuple(p) for p in pairs.tolist()] == want and dist.tolist() == [0.0, 0.0]
    pairs, _, _ = dwithin_pairs(series(right), series(left), 0.0)
    assert sorted((l, r) for r, l in pairs.tolist()) == want
    lines = (LS, [[(0.0, 1.0), (4.0, 1.0)]], None)
    pairs, _, _ = dwithin_pairs(series(left), series(lines), 0.0)
    assert pairs.tolist() == [[0, 0]]  # vertex on the segment; the vertex one ulp off is not returned


# ---- 4: the candidate set is a superset --------------------------------------------------------------------------------------------


@pytest.mark.parametrize("place", [(0.0, 0.0), (5e5, 4e6), (1.0e7, 6.5e6), (-2.0**33 + 2.0**20, 5 * 2.0**20)])
@pytest.mark.parametrize("t", [0.5, 3.0, 1024.0])
def test_boxes_exactly_t_apart(gpk, place, t):
    """geometries (and so their boxes) exactly t apart along one axis, for point, lineal and polygonal sides"""
    tx, ty = place
    rights = {
        PT: [(tx + 10.0 + t, ty + 1.0), (tx - t, ty + 1.0), (tx + 5.0, ty + 2.0 + t), (tx + 5.0, ty - t)],
        LS: [[(tx + 10.0 + t, ty), (tx + 10.0 + t, ty + 2.0)], [(tx - t, ty), (tx - t - 4.0, ty + 2.0)], [(tx, ty + 2.0 + t), (tx + 10.0, ty + 2.0 + t)], [(tx + 2.0, ty - t), (tx + 4.0, ty - t - 8.0)]],
        PG: [[_sq(tx + 10.0 + t, ty, tx + 12.0 + t, ty + 2.0)], [_sq(tx - t - 2.0, ty, tx - t, ty + 2.0)], [_sq(tx, ty + 2.0 + t, tx + 10.0, ty + 4.0 + t)], [_sq(tx + 2.0, ty - t - 1.0, tx + 4.0, ty - t)]],
    }
    lefts = {PG: [[_sq(tx, ty, tx + 10.0, ty + 2.0)]], LS: [[(tx, ty), (tx + 10.0, ty), (tx + 10.0, ty + 2.0), (tx, ty + 2.0), (tx, ty)]], MP: [[(tx, ty), (tx + 10.0, ty), (tx + 10.0, ty + 2.0), (tx, ty + 2.0), (tx + 5.0, ty), (tx + 5.0, ty + 2.0), (tx, ty + 1.0), (tx + 10.0, ty + 1.0), (tx + 2.0, ty), (tx + 4.0, ty)]]}
    for kl, lrows in lefts.items():
        for kr, rrows in rights.items():
            left, right = (kl, lrows, None), (kr, rrows, None)
            table = W.exact_table(left, right)  # (of the placed doubles as they are: the placement lost nothing if every pair is exactly t apart)
            assert len(table) == 4 and all(d2 == t * t for d2, _ in table.values()), (kl, kr, place, t)
            sl, sr = series(left), series(right)
            pairs, _, dist = dwithin_pairs(sl, sr, t)
            assert pairs.tolist() == [[0, 0], [0, 1], [0, 2], [0, 3]] and dist.tolist() == [t] * 4, (kl, kr, place, t, pairs.tolist(), dist.tolist())
            assert len(dwithin_pairs(sl, sr, float(np.nextafter(t, 0.0)))[0]) == 0
            pairs, _, _ = dwithin_pairs(sr, sl, t)
            assert pairs.tolist() == [[0, 0], [1, 0], [2, 0], [3, 0]]


def _t(p, axis):
    return p if axis == 0 else (p[1], p[0])


MARGIN_FAMILIES = {
    # name: (left kind, left row from (a, y), right kind, right row from (b, y)); segments of length 2 keep the distance arithmetic exact
    "pt_pt": (PT, lambda a, y: (a, y), PT, lambda b, y: (b, y)),
    "pt_mp": (PT, lambda a, y: (a, y), MP, lambda b, y: [(b, y), (b + 1.0, y)]),
    "mp_mp": (MP, lambda a, y: [(a, y), (a - 1.0, y)], MP, lambda b, y: [(b, y), (b + 1.0, y)]),
    "pt_ls": (PT, lambda a, y: (a, y), LS, lambda b, y: [(b, y - 1.0), (b, y + 1.0)]),
    "ls_ls": (LS, lambda a, y: [(a - 2.0, y), (a, y)], LS, lambda b, y: [(b, y - 1.0), (b, y + 1.0)]),
}


def _moved(kind, row, axis):
    if kind == PT:
        return _t(row, axis)
    return [_t(p, axis) for p in row]


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("fam", list(MARGIN_FAMILIES))
def test_computed_distance_is_t_but_the_box_grown_by_t_falls_short(gpk, fam, axis):
    """the margin of the box growth: fl(b - a) == t, so the library's distance is t and the pair belongs to the answer, while
    fl(a + t) < b — a left box grown by the bare distance does not reach the right box (tests/dwithin_ref.margin_cases)"""
    t, cases = W.margin_cases()
    kl, fl_, kr, fr = MARGIN_FAMILIES[fam]
    left = (kl, [_moved(kl, fl_(a, 100.0 * i), axis) for i, (a, b) in enumerate(cases)], None)
    right = (kr, [_moved(kr, fr(b, 100.0 * i), axis) for i, (a, b) in enumerate(cases)], None)
    for a, b in cases:
        assert a + t < b and b - t > a
    sl, sr = series(left), series(right)
    D = distance_matrix(left, right, sl, sr)
    assert (np.diag(D) == t).all(), np.diag(D).tolist()  # the library's own distance of every (i, i) is exactly t
    want = [[i, i] for i in range(len(cases))]
    pairs, counts, dist = dwithin_pairs(sl, sr, t)
    assert pairs.tolist() == want and counts.tolist() == [1] * len(cases) and dist.tolist() == [t] * len(cases)
    pairs, _, dist = dwithin_pairs(sr, sl, t)
    assert pairs.tolist() == want and dist.tolist() == [t] * len(cases)
    assert len(dwithin_pairs(sl, sr, float(np.nextafter(t, 0.0)))[0]) == 0


def test_box_distance_rounds_above_the_computed_distance(gpk):
    """the margin of the refine's box test: sqrt(dx * dx + dy * dy) of the two boxes can round one ulp above the point distance
    hypot(dx, dy); with t = that distance the pair belongs to the answer and a box test against the bare t would reject it"""
    rng = np.random.default_rng(11)
    dx, dy = rng.uniform(1.0, 50.0, 4000), rng.uniform(1.0, 50.0, 4000)
    left, right = (PT, [(0.0, 0.0)], None), (PT, list(zip(dx.tolist(), dy.tolist())), None)
    sl, sr = series(left), series(right)
    D = sr.distance(sl, other_rows=np.zeros(len(dx), dtype=np.uint32))  # D[j] = distance(left[0], right[j]) (hypot is symmetric)
    sel = np.flatnonzero(np.sqrt(dx * dx + dy * dy) > D)[:8]
    assert len(sel) >= 4
    for j in sel.tolist():
        pairs, _, dist = dwithin_pairs(sl, sr, float(D[j]))
        got = {p[1]: d for p, d in zip(pairs.tolist(), dist.tolist())}
        assert got.get(j) == D[j], (j, D[j])
        assert sorted(got) == np.flatnonzero(D <= D[j]).tolist()


def test_grown_boxes_against_the_grid_border_and_candidate_regimes(gpk):
    """right side: a 30 x 30 lattice of small squares (a right row spanning many cells among them).  Left rows: one whose grown box
    covers the whole grid (900+ candidates: the segmented-sort regime), one wholly outside, one straddling the border, one with
    between 17 and 48 candidates, several with a handful"""
    rrows = [[_sq(10.0 * i, 10.0 * j, 10.0 * i + 2.0, 10.0 * j + 2.0)] for j in range(30) for i in range(30)]
    rrows.append([_sq(0.0, 300.0, 292.0, 301.0)])  # spans the grid's width: listed in many cells, returned once
    right = (PG, rrows, None)
    lrows = [[(145.0, 145.0), (147.0, 147.0)], [(-5000.0, -5000.0), (-4990.0, -4990.0)], [(-3.0, 100.0), (-1.0, 101.0)],
             [(51.0, 51.0), (52.0, 52.0)], [(200.5, 200.5), (201.0, 201.5)], [(150.0, 310.0), (151.0, 312.0)]]
    left = (LS, lrows, None)
    sl, sr = series(left), series(right)
    D = distance_matrix(left, right, sl, sr)
    idx = SpatialIndex(sr, for_points=False)
    for t in (0.0, 9.0, 25.0, 250.0, 8000.0):
        p0, c0, d0 = expected(D, t)
        for ix in (None, idx):
            pairs, counts, dist = dwithin_pairs(sl, sr, t, r_index=ix)
            assert np.array_equal(pairs, p0) and np.array_equal(counts, c0) and dist.tobytes() == d0.tobytes(), t
    c25, c250 = expected(D, 25.0)[1], expected(D, 250.0)[1]
    assert 17 <= c25[3] <= 48 and c250[0] > 48 and c250[1] == 0 and 0 < c25[2] < 17 and expected(D, 8000.0)[1][1] == 901
    idx.free()


def test_degenerate_grid_axis(gpk):
    """all right boxes on one horizontal line (zero extent in y), and a single right point (zero extent on both axes)"""
    right = (PT, [(float(x), 7.0) for x in range(0, 100, 5)], None)
    left = (LS, [[(12.0, 3.0), (13.0, 4.0)], [(50.0, 107.0), (60.0, 107.0)], [(200.0, 7.0), (300.0, 7.0)]], None)
    sl, sr = series(left), series(right)
    D = distance_matrix(left, right, sl, sr)
    for t in (0.0, 3.0, 5.0, 100.0, 105.0):
        p0, c0, d0 = expected(D, t)
        pairs, counts, dist = dwithin_pairs(sl, sr, t)
        assert np.array_equal(pairs, p0) and np.array_equal(counts, c0) and dist.tobytes() == d0.tobytes(), t
    assert len(expected(D, 100.0)[0]) > 3
    one = (PT, [(3.0, 4.0)], None)
    pairs, _, dist = dwithin_pairs(series((PT, [(0.0, 0.0), (3.0, 4.0), (9.0, 4.0)], None)), series(one), 5.0)
    assert pairs.tolist() == [[0, 0], [1, 0]] and dist.tolist() == [5.0, 0.0]


# ---- 5: rules ----------------------------------------------------------------------------------------------------------------------


def test_null_empty_and_nan_rows_never_match(gpk):
    nan = float("nan")
    pts = (PT, [(0.0, 0.0), None, (nan, 0.0), (0.0, 0.0), (0.5, 0.0)], [True, True, True, False, True])
    lines = (LS, [[(0.0, 0.0), (1.0, 0.0)], [], [(0.0, 1.0), (1.0, 1.0)], [(0.0, 0.5), (1.0, 0.5)]], [True, True, False, True])
    want = W.dwithin_exact(pts, lines, 100.0)
    assert want == [(0, 0), (0, 3), (4, 0), (4, 3)]
    sp, sl = series(pts), series(lines)
    assert sp.distance(sl, other_rows=np.array([1, 1, 1, 1, 1], dtype=np.uint32))[0] == 0.0  # the point kernel's answer for an empty linestring
    pairs, counts, _ = dwithin_pairs(sp, sl, 100.0)
    assert [tuple(p) for p in pairs.tolist()] == want and counts.tolist() == [2, 0, 0, 0, 2]
    pairs, counts, _ = dwithin_pairs(sl, sp, 100.0)
    assert [tuple(p) for p in pairs.tolist()] == sorted((r, l) for l, r in want) and counts.tolist() == [2, 0, 0, 2]
    # row-wise: the same rows, an out-of-range map entry, both orders
    rows = np.array([0, 1, 0, 0, 7], dtype=np.uint32)
    assert sp.dwithin(sl, 100.0, other_rows=rows).tolist() == [True, False, False, False, False]
    # a valid point against an EMPTY row: the point kernels' distance is 0.0 (LINESTRING, POLYGON) or DBL_MAX, dwithin is False
    two = series((PT, [(0.0, 0.0), (0.5, 0.0)], None))
    assert two.distance(sl, other_rows=np.array([1, 1], dtype=np.uint32)).tolist() == [0.0, 0.0]
    assert two.dwithin(sl, 100.0, other_rows=np.array([1, 1], dtype=np.uint32)).tolist() == [False, False]
    assert two.dwithin(sl, 0.0, other_rows=np.array([1, 0], dtype=np.uint32)).tolist() == [False, True]
    for kind, empty, full in ((PG, [], [_sq(0.0, 0.0, 1.0, 1.0)]), (MLS, [], [[(0.0, 0.0), (1.0, 0.0)]]), (MPG, [], [[_sq(0.0, 0.0, 1.0, 1.0)]]), (MP, [], [(0.0, 0.0)])):
        col = series((kind, [empty, full], None))
        assert two.dwithin(col, 1e300).tolist() == [False, True] and col.dwithin(two, 1e300).tolist() == [False, True], kind
        pairs, counts, _ = dwithin_pairs(two, col, 1e300)
        assert pairs.tolist() == [[0, 1], [1, 1]] and counts.tolist() == [1, 1], kind
    four = series((PT, pts[1][:4], pts[2][:4]))
    assert four.dwithin(sl, 100.0).tolist() == [True, False, False, False]
    assert sl.dwithin(four, 100.0).tolist() == [True, False, False, False]
    # non-point pairs: empty multi-geometries, null rows
    a = (MPG, [[], [[[]]], [[_sq(0.0, 0.0, 1.0, 1.0)]], [[_sq(0.0, 0.0, 1.0, 1.0)]]], [True, True, True, False])
    b = (MP, [[(0.5, 0.5)], [], [(3.0, 1.0)], [(0.5, 0.5)]], [True, True, True, False])
    want = W.dwithin_exact(a, b, 2.0)
    assert want == [(2, 0), (2, 2)]
    pairs, _, dist = dwithin_pairs(series(a), series(b), 2.0)
    assert [tuple(p) for p in pairs.tolist()] == want and dist.tolist() == [0.0, 2.0]
    assert series(a).dwithin(series(b), 2.0).tolist() == [False, False, True, False]
    assert series(a).dwithin(series(b), float(np.nextafter(2.0, 0.0))).tolist() == [False, False, False, False]
    assert series(a).dwithin(series(b), 2.0, other_rows=np.array([0, 0, 2, 0], dtype=np.uint32)).tolist() == [False, False, True, False]


def test_empty_columns_and_bad_arguments(gpk):
    lib = _abi.lib()
    some = series((LS, [[(0.0, 0.0), (1.0, 0.0)], [(5.0, 5.0), (6.0, 5.0)]], None))
    none = series((LS, [], None))
    pairs, counts, dist = dwithin_pairs(some, none, 10.0)
    assert len(pairs) == 0 and counts.tolist() == [0, 0] and len(dist) == 0
    pairs, counts, _ = dwithin_pairs(none, some, 10.0)
    assert len(pairs) == 0 and len(counts) == 0
    pairs, counts, _ = dwithin_pairs(some, series((LS, [[], []], None)), 10.0)  # a right side of empty rows only
    assert len(pairs) == 0 and counts.tolist() == [0, 0]
    n = C.c_int64(-1)
    for d in (-1.0, float("nan"), float("inf")):
        assert lib.gpk_dwithin_join(some.device().handle, some.device().handle, None, d, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
        out = np.zeros(2, dtype=np.uint8)
        assert lib.gpk_dwithin_rowwise(some.device().handle, some.device().handle, None, d, out.ctypes.data, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    other = SpatialIndex(series((PT, [(0.0, 0.0)], None)), for_points=False)
    assert lib.gpk_dwithin_join(some.device().handle, some.device().handle, other.handle, 1.0, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    out = np.zeros(2, dtype=np.uint8)
    pts = series((PT, [(0.0, 0.0), (1.0, 1.0)], None))
    rows = np.zeros(2, dtype=np.uint32)
    assert lib.gpk_dwithin_rowwise(some.device().handle, pts.device().handle, rows.ctypes.data, 1.0, out.ctypes.data, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT
    three = series((PT, [(0.0, 0.0)] * 3, None))
    assert lib.gpk_dwithin_rowwise(some.device().handle, three.device().handle, None, 1.0, out.ctypes.data, _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("key", [(LS, PG, "g8"), (MPG, MP, "g8"), (MLS, MLS, "g32")], ids=str)
def test_rowwise_matches_distance_and_is_symmetric(gpk, key):
    left, right = W.pair_fixture(*key)
    n = min(len(left[1]), len(right[1]))
    a, b = (left[0], left[1][:n], left[2][:n]), (right[0], right[1][:n], right[2][:n])
    sa, sb = series(a), series(b)
    d = sa.distance(sb)
    ok = usable(a) & usable(b)
    for t in (0.0, float(np.nanmedian(d)), float(np.nanmax(d))):
        want = ok & (d <= t)
        assert np.array_equal(sa.dwithin(sb, t), want) and np.array_equal(sb.dwithin(sa, t), want)


@pytest.mark.parametrize("how", ["inner", "left"])
def test_table_join(gpk, how):
    key = ("linestring", 8, True)
    left, right = W.point_fixture(*key)
    keep = usable(right)
    la, ra = X.column(*left), X.column(right[0], [r for r, k in zip(right[1], keep) if k])
    t = 60.0
    pairs, counts, dist = dwithin_pairs(GeoSeries(la), GeoSeries(ra), t)
    assert 0 < len(pairs) and (counts == 0).any()
    li, ri = join_indices(counts, pairs, how)
    lt = pa.table({"id": pa.array(np.arange(len(la))), "geometry": la.to_arrow_wkb()})
    rt = pa.table({"name": pa.array([f"r{i}" for i in range(len(ra))]), "geometry": ra.to_arrow_wkb()})
    out = spatial_join_dwithin(lt, rt, SpatialJoinDWithinArgs(distance=t, join_type=how, distance_col="dist"))
    assert out.column_names == ["id_left", "geometry_left", "name_right", "geometry_right", "dist"] and out.num_rows == len(li)
    assert out.column("id_left").combine_chunks().equals(take_column(lt.column("id"), li))
    assert out.column("name_right").combine_chunks().equals(take_column(rt.column("name"), ri))
    d = out.column("dist").combine_chunks()
    assert d.null_count == np.count_nonzero(ri < 0) and np.array_equal(np.asarray(d.drop_null()), dist)
    assert (how == "left") == bool(np.count_nonzero(ri < 0))


# ---- 6: relations to existing operators ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("key", [("linestring", 8, True), ("multipolygon", 32, True), ("multipoint", 1, True)], ids=str)
def test_nearest_pairs_are_dwithin_pairs(gpk, key):
    left, right = W.point_fixture(*key)
    sl, sr = series(left), series(right)
    for t in (7.5, 60.0):
        np_, nc, nd = nearest_pairs(sl, sr, max_distance=t)
        dp, dc, dd = dwithin_pairs(sl, sr, t)
        within = {tuple(p): d for p, d in zip(dp.tolist(), dd.tolist())}
        assert len(np_) > 0
        for p, d in zip(np_.tolist(), nd.tolist()):
            assert within[tuple(p)] == d
        assert np.array_equal(nc > 0, dc > 0)


@pytest.mark.parametrize("ka,kb", [(PG, PG), (PG, MPG), (MPG, PG), (MPG, MPG)])
def test_zero_distance_equals_the_intersects_join(gpk, ka, kb):
    left, right = W.pair_fixture(ka, kb, "g8", seed=1)  # (a seed whose columns hold intersecting pairs for all four family pairs)
    assert len(W.dwithin_exact(left, right, 0.0)) > 0
    sl, sr = series(left), series(right)
    want, wc = join_pairs(sl, sr, "intersects")
    pairs, counts, _ = dwithin_pairs(sl, sr, 0.0)
    assert len(want) > 0 and np.array_equal(pairs, want) and np.array_equal(counts, wc)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------


def test_two_calls_give_identical_bytes(gpk):
    left, right = W.pair_fixture(LS, MPG, "large")
    sl, sr = series(left), series(right)
    a, b = dwithin_pairs(sl, sr, 60.0), dwithin_pairs(sl, sr, 60.0)
    assert len(a[0]) > 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
