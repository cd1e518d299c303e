"""GPU: row-wise distance between two non-point columns (gpk_distance_rowwise -> csrc/gpk_pairdist.hip) against the exact reference
of tests/pair_distance_ref.py.

Instances: pairdist_kernel<G, KA, KB> for the 15 unordered family pairs (KA <= KB by family code, the dispatch swaps the columns
otherwise) and G = 8 / 32, plus pairdist_large_kernel<KA, KB> for rows whose n_A * n_B exceeds PD_LARGE_COST.  The rules are restated
here (pair_group_size, LARGE_COST) so that each fixture is known to select the instance it is named after."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from geopolars_amd import _abi, synth
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from tests import exact_ref as X
from tests import pair_distance_ref as R

pytestmark = pytest.mark.gpu

MP, LS, MLS, PG, MPG = _abi.GEOM_MULTIPOINT, _abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON
KINDS = [MP, LS, MLS, PG, MPG]
LARGE_COST = 1 << 16  # gpk_pairdist.hip PD_LARGE_COST: rows with n_A * n_B above it go to the work-group schedule


def pair_group_size(a: GeoArrowArray, b: GeoArrowArray) -> int:
    """gpk_pairdist.hip pairdist_group_size: 32 lanes when the larger of the two columns' mean coordinate counts is >= 128, else 8"""
    m = max(x.n_coords / x.n_geoms if x.n_geoms else 0.0 for x in (a, b))
    return 32 if m >= 128 else 8


def row_coords(kind, row) -> int:
    return sum(len(s) for s in X.row_seqs(kind, row))


# ---- fixture rows -------------------------------------------------------------------------------------------------------------


def _ring(rng, cx, cy, size, n, cw=False):
    return X._star(rng, cx, cy, size, n, cw)


def make_row(kind, rng, cx, cy, size, nv):
    """a row of `kind` with about nv coordinates around (cx, cy) of extent ~size"""
    if kind == MP:
        return [tuple(p) for p in np.stack([cx + rng.uniform(-size, size, nv) / 2, cy + rng.uniform(-size, size, nv) / 2], axis=1)]
    if kind == LS:
        t = np.linspace(-0.5, 0.5, nv)
        return [tuple(p) for p in np.stack([cx + size * t, cy + size * 0.3 * np.sin(7 * t) + rng.uniform(-0.02, 0.02, nv) * size], axis=1)]
    if kind == MLS:
        k = 2
        return [make_row(LS, rng, cx + (i - 0.5) * size * 0.2, cy + (i - 0.5) * size * 0.3, size * 0.8, max(1, nv // k)) for i in range(k)]
    if kind == PG:
        ext = _ring(rng, cx, cy, size, max(3, nv - 6))
        hole = _ring(rng, cx, cy, size * 0.15, 4, cw=True)
        return [ext, hole]
    return [make_row(PG, rng, cx - size * 0.3, cy, size * 0.5, max(4, nv // 2)), [_ring(rng, cx + size * 0.4, cy, size * 0.3, max(3, nv // 2 - 1))]]


def pair_column(ka, kb, nv_a, nv_b, n=12, seed=0, size=40.0, base=(0.0, 0.0)):
    """rows pairs of ka x kb: overlapping, touching distance, near and far, placed along a diagonal from `base`"""
    rng = np.random.default_rng(seed + 97 * ka + 13 * kb + nv_a)
    ra, rb = [], []
    for i in range(n):
        cx, cy = base[0] + 1000.0 * i, base[1] + 500.0 * i
        off = [0.0, 0.6, 1.1, 3.0, 20.0][i % 5] * size
        ra.append(make_row(ka, rng, cx, cy, size, nv_a))
        rb.append(make_row(kb, rng, cx + off, cy + 0.3 * off, size, nv_b))
    return ra, rb


def gpu(ka, ra, kb, rb, b_rows=None, va=None, vb=None):
    a, b = X.column(ka, ra, va), X.column(kb, rb, vb)
    return GeoSeries(a).distance(GeoSeries(b), other_rows=b_rows), a, b


# ---- every ordered pair and every instance ----------------------------------------------------------------------------------------

SIZES = {"g8": (12, 9), "g32": (160, 140), "large": (320, 280)}


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("ka,kb", list(itertools.product(KINDS, KINDS)))
def test_every_pair_and_instance(gpk, ka, kb, size):
    nva, nvb = SIZES[size]
    ra, rb = pair_column(ka, kb, nva, nvb, n=10 if size != "large" else 5)
    got, a, b = gpu(ka, ra, kb, rb)
    G = pair_group_size(a, b)
    costs = [row_coords(ka, x) * row_coords(kb, y) for x, y in zip(ra, rb)]
    if size == "large":
        assert all(c > LARGE_COST for c in costs)
    else:
        assert G == (8 if size == "g8" else 32) and all(c <= LARGE_COST for c in costs), (G, max(costs))
    exact = R.rowwise(ka, ra, kb, rb)
    R.check(got, exact, (ka, kb, size))
    assert any(d is not None and d > 0 for d, _ in exact)
    if MP not in (ka, kb):  # (random points hit nothing exactly)
        assert any(d == 0 for d, _ in exact)


# ---- hand-made cases ------------------------------------------------------------------------------------------------------------


def _sq(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]


ULP_Y = np.nextafter(1.0, 2.0)
CASES = [
    # name, ka, a, kb, b, exact distance
    ("x_crossing", LS, [(0.0, 0.0), (4.0, 4.0)], LS, [(0.0, 4.0), (4.0, 0.0)], 0.0),
    ("plus_rectangles", PG, [_sq(-1.0, -3.0, 1.0, 3.0)], PG, [_sq(-3.0, -1.0, 3.0, 1.0)], 0.0),
    ("in_hole", PG, [_sq(4.0, 4.0, 6.0, 6.0)], PG, [_sq(0.0, 0.0, 10.0, 10.0), _sq(3.0, 3.0, 7.0, 7.0)[::-1]], 1.0),
    ("touching_hole", PG, [_sq(3.0, 4.0, 6.0, 6.0)], PG, [_sq(0.0, 0.0, 10.0, 10.0), _sq(3.0, 3.0, 7.0, 7.0)[::-1]], 0.0),
    ("line_inside_polygon", LS, [(2.0, 2.0), (3.0, 5.0)], PG, [_sq(0.0, 0.0, 10.0, 10.0)], 0.0),
    ("collinear_overlap", LS, [(0.0, 0.0), (2.0, 0.0)], LS, [(1.0, 0.0), (3.0, 0.0)], 0.0),
    ("vertex_on_segment", LS, [(1.0, 1.0), (1.0, 5.0)], LS, [(0.0, 1.0), (4.0, 1.0)], 0.0),
    ("vertex_ulp_off", LS, [(1.0, ULP_Y), (1.0, 5.0)], LS, [(0.0, 1.0), (4.0, 1.0)], float(ULP_Y - 1.0)),
    ("far_members", MLS, [[(0.0, 0.0), (1.0, 0.0)], [(100.0, 0.0), (101.0, 0.0)]], MPG, [[_sq(200.0, 0.0, 201.0, 1.0)], [_sq(104.0, 0.0, 105.0, 1.0)]], 3.0),
    ("one_coordinate_lines", LS, [(0.0, 0.0)], LS, [(3.0, 4.0)], 5.0),
    ("multipoints", MP, [(0.0, 0.0), (50.0, 50.0)], MP, [(53.0, 54.0), (-100.0, 0.0)], 5.0),
    ("point_in_polygon_member", MP, [(-50.0, 0.0), (5.0, 5.0)], MPG, [[_sq(100.0, 0.0, 101.0, 1.0)], [_sq(0.0, 0.0, 10.0, 10.0)]], 0.0),
    ("polygon_in_polygon", PG, [_sq(2.0, 2.0, 3.0, 3.0)], MPG, [[_sq(0.0, 0.0, 10.0, 10.0)]], 0.0),
    ("empty_member_ignored", MLS, [[], [(0.0, 3.0), (0.0, 5.0)]], LS, [(-4.0, 0.0), (4.0, 0.0)], 3.0),
]


def _cases_columns(cases):
    out = {}
    for name, ka, a, kb, b, d in cases:
        out.setdefault((ka, kb), []).append((name, a, b, d))
    return out


@pytest.mark.parametrize("ka,kb", list(_cases_columns(CASES)))
def test_hand_made_cases(gpk, ka, kb):
    cases = _cases_columns(CASES)[(ka, kb)]
    ra, rb = [c[1] for c in cases], [c[2] for c in cases]
    got, _, _ = gpu(ka, ra, kb, rb)
    exact = R.rowwise(ka, ra, kb, rb)
    R.check(got, exact, "hand")
    for (name, _, _, d), g, (e, _) in zip(cases, got, exact):
        assert float(e) == d, (name, e, d)
        assert (g == 0.0) == (d == 0.0), (name, g)
        if name == "vertex_ulp_off":
            assert 0.0 < g <= 4 * d, (name, g)
    rev, _, _ = gpu(kb, rb, ka, ra)  # both orders: same zero / non-zero outcome, within the contract
    R.check(rev, exact, "hand reversed")


def test_null_empty_and_out_of_range_rows(gpk):
    ra = [[(0.0, 0.0), (1.0, 0.0)], [], [(0.0, 0.0), (1.0, 1.0)], [(5.0, 5.0), (6.0, 5.0)]]
    rb = [[_sq(0.0, 2.0, 1.0, 3.0)], [_sq(0.0, 2.0, 1.0, 3.0)], [], [_sq(0.0, 2.0, 1.0, 3.0)]]
    va = [True, True, True, False]
    got, _, _ = gpu(LS, ra, PG, rb, va=va)
    assert got[0] == 2.0 and np.isnan(got[1:]).all(), got
    vb = [True, False, True, True]
    rows = np.array([3, 1, 0, 0, 4, 0xFFFFFFFF], dtype=np.uint32)
    ra2 = ra[:3] + [[(0.0, 0.0), (1.0, 0.0)]] * 3
    got, _, _ = gpu(LS, ra2, PG, rb, b_rows=rows, vb=vb)
    exact = R.rowwise(LS, ra2, PG, rb, b_rows=rows, valid_b=vb)
    R.check(got, exact, "b_rows")
    assert got[0] == 2.0 and got[2] == 1.0 and got[3] == 2.0 and np.isnan(got[[1, 4, 5]]).all(), got
    # empty multi-geometries: every member empty
    got, _, _ = gpu(MPG, [[], [[[]]]], MP, [[(1.0, 1.0)], [(1.0, 1.0)]])
    assert np.isnan(got).all(), got


# ---- georeferenced magnitudes and exact 2^k scaling -----------------------------------------------------------------------------

SCALE_CASES = [c for c in CASES if c[0] != "empty_member_ignored"]
GEO_CASES = [c for c in SCALE_CASES if c[0] != "vertex_ulp_off"]  # (1 + ulp) + a placement is not exact: checked at the origin only


def _moved(kind, row, f):
    """row with f applied to every coordinate"""
    if kind in (MP, LS):
        return [f(p) for p in row]
    if kind in (MLS, PG):
        return [[f(p) for p in s] for s in row]
    return [[[f(p) for p in r] for r in poly] for poly in row]


@pytest.mark.parametrize("place", range(len(X.PLACEMENTS)))
def test_cases_at_georeferenced_magnitudes(gpk, place):
    tx, ty = X.PLACEMENTS[place]
    shift = lambda p: (p[0] + tx, p[1] + ty)
    for (ka, kb), cases in _cases_columns(GEO_CASES).items():
        ra = [_moved(ka, c[1], shift) for c in cases]
        rb = [_moved(kb, c[2], shift) for c in cases]
        a, b = X.column(ka, ra), X.column(kb, rb)
        assert np.array_equal(a.xy - (tx, ty), X.column(ka, [c[1] for c in cases]).xy), "placement is not exact"
        got = GeoSeries(a).distance(GeoSeries(b))
        exact = R.rowwise(ka, ra, kb, rb)
        R.check(got, exact, ("placed", place))
        for (name, *_r, d), (e, _) in zip(cases, exact):
            assert float(e) == d, (name, place, e, d)
    # a random column placed there (not exactly: the reference takes the placed coordinates as they are)
    ra, rb = pair_column(PG, MLS, 30, 20, n=10, seed=place, base=(tx, ty))
    got, _, _ = gpu(PG, ra, MLS, rb)
    R.check(got, R.rowwise(PG, ra, MLS, rb), ("placed random", place))


@pytest.mark.parametrize("k", [-100, -37, -1, 1, 52, 100])
def test_exact_power_of_two_scaling(gpk, k):
    cols = [(ka, kb, [c[1] for c in cases], [c[2] for c in cases]) for (ka, kb), cases in _cases_columns(SCALE_CASES).items()]
    for i, base in enumerate([(0.0, 0.0)] + X.PLACEMENTS[:2]):
        ra, rb = pair_column(MPG, MLS, 40, 30, n=10, seed=5 + i, base=base)
        cols.append((MPG, MLS, ra, rb))
    for ka, kb, ra, rb in cols:
        a, b = X.column(ka, ra), X.column(kb, rb)
        ref = GeoSeries(a).distance(GeoSeries(b))
        sa, sb = X.scaled(a, k), X.scaled(b, k)
        assert np.array_equal(np.ldexp(sa.xy, -k), a.xy) and np.array_equal(np.ldexp(sb.xy, -k), b.xy)
        got = GeoSeries(sa).distance(GeoSeries(sb))
        assert np.array_equal(got, np.ldexp(ref, k)), (ka, kb, k, got, ref)
        rev = GeoSeries(sb).distance(GeoSeries(sa))
        assert np.array_equal(rev == 0.0, got == 0.0)


# ---- seeded random columns against the reference, both sides of the large-row threshold -----------------------------------------


def _rows_of(a: GeoArrowArray):
    """GeoArrowArray (LINESTRING / POLYGON / MULTIPOLYGON) -> exact_ref rows"""
    if a.geom_type == LS:
        return [a.xy[a.geom_offsets[i]:a.geom_offsets[i + 1]] for i in range(a.n_geoms)]
    geoms = X.polygon_geoms(a)
    return [g[0] for g in geoms] if a.geom_type == PG else geoms


def test_random_columns_against_reference(gpk):
    pl = synth.powerlaw_multipolygons(60, seed=11, cap=4000, alpha=0.6, domain=1000.0)  # (a heavy tail: 7 rows above the threshold)
    st = synth.star_polygons(60, n_verts=64, seed=12, domain=1000.0)
    got = GeoSeries(pl).distance(GeoSeries(st))
    ra, rb = _rows_of(pl), _rows_of(st)
    costs = [row_coords(MPG, x) * row_coords(PG, y) for x, y in zip(ra, rb)]
    assert min(costs) <= LARGE_COST < max(costs), (min(costs), max(costs))
    R.check(got, R.rowwise(MPG, ra, PG, rb), "powerlaw x star")
    cp = synth.clustered_polygons(400, seed=13)
    rows = (np.arange(400) + 1) % 400
    got = GeoSeries(cp).distance(GeoSeries(cp), other_rows=rows)
    rc = _rows_of(cp)
    exact = R.rowwise(PG, rc, PG, rc, b_rows=rows)
    R.check(got, exact, "clustered i, i+1")
    ln = synth.random_linestrings(200, seed=14, domain=300.0)
    perm = np.random.default_rng(3).permutation(200).astype(np.uint32)
    got = GeoSeries(ln).distance(GeoSeries(ln), other_rows=perm)
    rl = _rows_of(ln)
    R.check(got, R.rowwise(LS, rl, LS, rl, b_rows=perm), "linestrings permuted")


def test_5000_by_5000_row(gpk):
    rng = np.random.default_rng(21)
    a = [X._star(rng, 0.0, 0.0, 100.0, 4999)]
    b_far = [X._star(rng, 150.0, 20.0, 100.0, 4999)]
    b_cross = [X._star(rng, 60.0, 0.0, 100.0, 4999)]
    ra, rb = [a, a, [_sq(-1.0, -1.0, 1.0, 1.0)]], [b_far, b_cross, b_far]
    got, _, _ = gpu(PG, ra, PG, rb)
    assert row_coords(PG, a) * row_coords(PG, b_far) >= 25_000_000
    R.check(got, R.rowwise(PG, ra, PG, rb), "5000 x 5000")


# ---- symmetry, device outputs, determinism, and the point pairs' bits ----------------------------------------------------------


def test_symmetry_device_output_and_determinism(gpk):
    ra, rb = pair_column(MPG, LS, 60, 50, n=40, seed=8)
    ab, a, b = gpu(MPG, ra, LS, rb)
    ba, _, _ = gpu(LS, rb, MPG, ra)
    assert np.array_equal(ab == 0.0, ba == 0.0)
    R.check(ba, R.rowwise(LS, rb, MPG, ra), "reversed")
    for _ in range(3):
        again, _, _ = gpu(MPG, ra, LS, rb)
        assert np.array_equal(again, ab)
    sa, sb = GeoSeries(a), GeoSeries(b)
    n = len(ra)
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    rows = torch.from_numpy(np.arange(n, dtype=np.int32)[::-1].copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    _abi.check(_abi.lib().gpk_distance_rowwise(sa.device().handle, sb.device().handle, None, C.c_void_p(out.data_ptr()), _abi.MEM_DEVICE, C.c_void_p(st)))
    torch.cuda.current_stream().synchronize()
    assert np.array_equal(out.cpu().numpy(), ab)
    _abi.check(_abi.lib().gpk_distance_rowwise(sa.device().handle, sb.device().handle, C.c_void_p(rows.data_ptr()), C.c_void_p(out.data_ptr()), _abi.MEM_DEVICE, C.c_void_p(st)))
    torch.cuda.current_stream().synchronize()
    host = sa.distance(sb, other_rows=np.arange(n, dtype=np.uint32)[::-1].copy())
    assert np.array_equal(out.cpu().numpy(), host)


def test_point_pairs_keep_their_kernel(gpk, oracle):
    """POINT x anything still runs distance_kernel: both argument orders give the same bits, equal to the oracle to 1e-9"""
    ls = synth.random_linestrings(500, seed=30, domain=500.0)
    pts = synth.uniform_points(500, seed=31, domain=500.0)
    d1 = GeoSeries(pts).distance(GeoSeries(ls))
    d2 = GeoSeries(ls).distance(GeoSeries(pts))
    assert np.array_equal(d1, d2)
    od = oracle.distance_rowwise(pts, ls)
    assert np.allclose(d1, od, rtol=1e-9, atol=0) and np.array_equal(d1 == 0.0, od == 0.0)
