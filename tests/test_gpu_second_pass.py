"""GPU: every capped-grid and work-list kernel past its first pass (tests/second_pass.py has the helpers and the inventory).

A column is sized from the device's CU count so that every block of the capped grid takes a second unit and the tail is ragged, and is
filled with a shuffled tiling of a small base column.  Expected values come from the exact references, computed once per base row and
gathered with the tiling's order; they never come from the GPU.  Device outputs are prefilled with a sentinel, so a skipped unit
shows; float outputs must also be bit-identical for all rows drawn from one base row and to a small-column run at the same lane-group
size (stale state from a group's earlier unit often changes only the last bit)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from tests import exact_ref as X
from tests import linerel_ref as L
from tests import polyrel_ref as P
from tests import relation_ref as R
from tests import second_pass as SP
from tests import validity_ref as V

pytestmark = pytest.mark.gpu

PT, MP, LS, MLS, PG, MPG = (_abi.GEOM_POINT, _abi.GEOM_MULTIPOINT, _abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON,
                            _abi.GEOM_MULTIPOLYGON)
DEV = "cuda:0"
SENTINEL = 0xEE


@pytest.fixture(scope="module")
def cus(gpk):
    return gpk.device_info()[1]


def lane_group_rows(cus, G, cap_mult=32):
    """(rows, stride in rows) of a lane-group kernel: 256 / G rows a block, blocks capped at cus * cap_mult"""
    per_block = 256 // G
    return SP.second_trip_rows(cus, cap_mult, per_block), cus * cap_mult * per_block


def mean_coords(col: GeoArrowArray) -> float:
    return col.n_coords / max(col.n_geoms, 1)


def u32_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def masks_on_device(fn, a: GeoSeries, b: GeoSeries, rows=None, n=None):
    """a row-wise relation entry point (a, b, b_rows, out, space, stream) writing uint8 into a sentinel-filled device buffer"""
    n = len(a) if n is None else n
    out = torch.full((n,), SENTINEL, dtype=torch.uint8, device=DEV)
    r = None if rows is None else u32_dev(rows)
    _abi.check(fn(a.device().handle, b.device().handle, None if r is None else r.data_ptr(), out.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def map_coords(row, f):
    """a row of any family (None, a coordinate tuple, or nested lists of them) with f(x, y) in place of every coordinate"""
    if row is None:
        return None
    if isinstance(row, tuple):
        return f(*row)
    return [map_coords(r, f) for r in row]


def assert_masks(got, want, order):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), [(int(i), int(order[i]), int(got[i]), int(want[i])) for i in bad[:8]])


# ---- validity and is_simple: lane groups ----------------------------------------------------------------------------------------------


def _first_coords(kind, rows):
    return np.concatenate([[0], np.cumsum([V.n_coords(kind, r) for r in rows])])[:-1].astype(np.int64)


def _validity_base(kind, G):
    rows, valid = [], []
    for src in (V.known_column, V.random_column):
        r, v, c, _ = src(kind)
        if G == V.VAL_G_LARGE and src is V.random_column:  # (every other row: the exact reference of the padded rings takes its time)
            r, v, c = r[::2], v[::2], c[::2]
        if G == V.VAL_G_LARGE:  # 12 more vertices inside every edge (a NaN cannot be padded: those rows stay out)
            keep = [i for i, code in enumerate(c) if code != V.COORDINATE]
            r, v = V.padded(kind, [r[i] for i in keep], 12), [v[i] for i in keep]
        rows += list(r)
        valid += list(v)
    codes, where = V.validity_column(kind, rows, valid)
    local = np.where(where >= 0, where - _first_coords(kind, rows), -1)
    return rows, valid, codes, local


def _tiled_where(kind, rows, local, order):
    n_coords = np.array([V.n_coords(kind, r) for r in rows], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(n_coords[order])])[:-1]
    assert first[-1] < 2**31
    return np.where(local[order] >= 0, local[order] + first, -1).astype(np.int32)


@pytest.mark.parametrize("G", [V.VAL_G_SMALL, V.VAL_G_LARGE], ids=["G4", "G16"])
@pytest.mark.parametrize("kind", [PG, MPG], ids=["pg", "mpg"])
def test_validity_rows(gpk, cus, kind, G):
    from tests.test_gpu_validity import device_answers

    rows, valid, codes, local = _validity_base(kind, G)
    n, groups = lane_group_rows(cus, G)
    assert n > cus * 32 * (256 // G)
    order = SP.shuffled_tiling(len(rows), n, seed=10 * kind + G, groups=groups)
    col = X.column(kind, rows, valid).take(order)
    assert V.lanes_of(col.n_coords, len(col)) == G and len(col) == n
    got_c, got_w = device_answers(GeoSeries(col))  # prefilled with 77 / -7
    want_w = _tiled_where(kind, rows, local, order)
    bad = np.nonzero((got_c != codes[order]) | (got_w != want_w))[0]
    assert len(bad) == 0, (len(bad), [(int(i), int(order[i]), int(got_c[i]), int(codes[order[i]]), int(got_w[i]), int(want_w[i])) for i in bad[:8]])


def _pad_line(kind, row, k):
    return V.pad_ring(row, k) if kind == LS else [V.pad_ring(m, k) for m in row]


def _simple_on_device(col):
    s = GeoSeries(col)
    out = torch.full((len(s),), 9, dtype=torch.uint8, device=DEV)
    _abi.check(_abi.lib().gpk_is_simple(s.device().handle, out.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("G", [V.VAL_G_SMALL, V.VAL_G_LARGE], ids=["G4", "G16"])
@pytest.mark.parametrize("kind", [LS, MLS], ids=["ls", "mls"])
def test_is_simple_rows(gpk, cus, kind, G):
    rows, valid, want = V.known_simple_column(kind)
    # (a shuffled tiling needs more than a dozen different rows: the known rows again, mirrored, and moved and stretched)
    rows = rows + [map_coords(r, lambda x, y: (y, x)) for r in rows] + [map_coords(r, lambda x, y: (2 * x + 7, y - 3)) for r in rows]
    valid, want = valid * 3, V.is_simple_column(kind, rows, valid * 3)
    assert np.array_equal(want, np.tile(want[: len(want) // 3], 3))
    if G == V.VAL_G_LARGE:  # collinear vertices inside every segment until the mean picks 16 lanes; the reference answers again
        for k in (15, 31, 63):
            prows = [_pad_line(kind, r, k) for r in rows]
            if V.lanes_of(sum(V.n_coords(kind, r) for r in prows), len(prows)) == G:
                break
        rows, want = prows, V.is_simple_column(kind, prows, valid)
    n, groups = lane_group_rows(cus, G)
    assert n > cus * 32 * (256 // G)
    order = SP.shuffled_tiling(len(rows), n, seed=20 * kind + G, groups=groups)
    col = X.column(kind, rows, valid).take(order)
    assert V.lanes_of(col.n_coords, len(col)) == G
    got = _simple_on_device(col)
    assert set(np.unique(got).tolist()) <= {0, 1}, np.unique(got)  # (9: a row nobody wrote)
    assert_masks(got, want[order].astype(np.uint8), order)


# ---- validity and is_simple: the work-group list ----------------------------------------------------------------------------------


def _large_rings():
    """16 rings just above VAL_BLOCK_COORDS coordinates, of different sizes, with and without the planted faults and holes of
    validity_ref.large_column"""
    out = []
    for i, fault in enumerate([None, "first", "last", "strip"] * 3):
        out.append(V.zigzag(V.VAL_BLOCK_COORDS + 1 + 23 * i, fault=fault))
    for n, poke in ((530, False), (612, True), (702, False), (516, True)):  # (a hole pokes out through a shell vertex at y = 4: even n)
        m = n - 3
        hole = [(m - 3.0, 1.0), (m - 3.0, 5.0 if poke else 3.0), (m - 2.0, 3.0), (m - 2.0, 1.0), (m - 3.0, 1.0)]
        out.append(V.zigzag(n, hole=hole))
    return out


def _interleaved(order_large, n_large_base, n_small_base, seed):
    """the large rows in `order_large`, each followed by a random small row (base rows: the large ones first, then the small ones)"""
    rng = np.random.default_rng(seed)
    order = np.empty(2 * len(order_large), dtype=np.int64)
    order[0::2] = order_large
    order[1::2] = n_large_base + rng.integers(0, n_small_base, len(order_large))
    return order


def test_validity_large_rows(gpk, cus):
    """more listed rows than validity_big_kernel has blocks (cus * 8), small rows between them so the list fills in scattered order"""
    from tests.test_gpu_validity import device_answers

    large = _large_rings()
    small, small_valid, _, _ = V.known_column(PG)
    rows, valid = large + list(small), [True] * len(large) + list(small_valid)
    assert all(V.n_coords(PG, r) > V.VAL_BLOCK_COORDS for r in large) and all(V.n_coords(PG, r) <= V.VAL_BLOCK_COORDS for r in small)
    codes, where = V.validity_column(PG, rows, valid)
    assert {V.VALID, V.SELF_INTERSECTION, V.RINGS_CROSS} <= set(codes[: len(large)].tolist())
    local = np.where(where >= 0, where - _first_coords(PG, rows), -1)
    n_large = SP.second_trip_rows(cus, 8, 1)
    assert n_large > cus * 8 * 1
    order = _interleaved(SP.shuffled_tiling(len(large), n_large, seed=31, groups=cus * 8), len(large), len(small), seed=32)
    col = X.column(PG, rows, valid).take(order)
    got_c, got_w = device_answers(GeoSeries(col))
    want_w = _tiled_where(PG, rows, local, order)
    bad = np.nonzero((got_c != codes[order]) | (got_w != want_w))[0]
    assert len(bad) == 0, (len(bad), [(int(i), int(order[i]), int(got_c[i]), int(codes[order[i]]), int(got_w[i]), int(want_w[i])) for i in bad[:8]])


@pytest.mark.parametrize("kind", [LS, MLS], ids=["ls", "mls"])
def test_is_simple_large_rows(gpk, cus, kind):
    rings = [r[0] for r in _large_rings()[:12]]  # closed lines: simple unless a tooth was pulled across
    far = [(-10.0, -10.0), (-5.0, -12.0)]
    large = rings if kind == LS else [[r, far] if i % 2 else [[], r] for i, r in enumerate(rings)]
    small, small_valid, _ = V.known_simple_column(kind)
    rows, valid = large + list(small), [True] * len(large) + list(small_valid)
    want = V.is_simple_column(kind, rows, valid)
    assert want[: len(large)].any() and not want[: len(large)].all()
    n_large = SP.second_trip_rows(cus, 8, 1)
    assert n_large > cus * 8 * 1
    order = _interleaved(SP.shuffled_tiling(len(large), n_large, seed=41 + kind, groups=cus * 8), len(large), len(small), seed=42)
    got = _simple_on_device(X.column(kind, rows, valid).take(order))
    assert_masks(got, want[order].astype(np.uint8), order)


# ---- relation masks: lane groups, with and without a b_rows map ---------------------------------------------------------------------


def _relation_case(cus, G, a_col, b_col, want, seed, lanes):
    """the tiled pair of columns (row i of both is base row order[i]) for a relation kernel of 256 / G rows a block, cap cus * 32"""
    n, groups = lane_group_rows(cus, G)
    assert n > cus * 32 * (256 // G)
    order = SP.shuffled_tiling(len(a_col), n, seed=seed, groups=groups)
    ta, tb = a_col.take(order), b_col.take(order)
    assert lanes(ta, tb) == G, (mean_coords(ta), mean_coords(tb))
    return GeoSeries(ta), GeoSeries(tb), want[order], order


def _lanes_by_either_mean(a, b):
    return 16 if max(mean_coords(a), mean_coords(b)) >= 32.0 else 4


@pytest.mark.parametrize("ka,kb,pad", [(MPG, MPG, 0), (PG, MPG, 7)], ids=["mpg-mpg-G4", "pg-mpg-G16"])
def test_polygon_relation_rows(gpk, cus, ka, kb, pad):
    A, B, want = [], [], []
    for a, b, w in (P.random_columns(ka, kb), P.case_columns(P.KNOWN, ka, kb, pad)[:3], P.case_columns(P.TIES, ka, kb, pad)[:3]):
        first = len(A) == 0  # (the random columns are padded here, the cases by case_columns)
        A += [R.padded(ka, r, pad) for r in a] if first else list(a)
        B += [R.padded(kb, r, pad) for r in b] if first else list(b)
        want.append(np.asarray(w, dtype=np.uint8))
    want = np.concatenate(want)
    a_col, b_col = X.column(ka, A), X.column(kb, B)
    G = 16 if pad else 4
    sa, sb, exp, order = _relation_case(cus, G, a_col, b_col, want, seed=50 + G, lanes=_lanes_by_either_mean)
    n = len(order)
    assert n > cus * 32 * (256 // G)
    fn = _abi.lib().gpk_polygon_relation
    assert_masks(masks_on_device(fn, sa, sb), exp, order)
    assert_masks(masks_on_device(fn, sb, sa), P.swapped(exp), order)
    base_b = GeoSeries(b_col)  # b_rows: the tiled A against the base B
    assert _lanes_by_either_mean(sa.array, b_col) == G
    assert_masks(masks_on_device(fn, sa, base_b, rows=order), exp, order)


@pytest.mark.parametrize("kl,kp,pad", [(MLS, MPG, 0), (LS, PG, 1)], ids=["mls-mpg-G4", "ls-pg-G16"])
def test_line_polygon_relation_rows(gpk, cus, kl, kp, pad):
    lines, polys, want = R.random_columns(kl, kp)
    lines = [R.scaled_line(kl, r, pad) for r in lines]
    polys = [R.padded(kp, r, pad) for r in polys]
    want = [want]
    for src in (R.known_columns(kl, kp), R.tie_columns(kl, 0)[kp]):
        lines += [R.scaled_line(kl, r, pad) for r in src[0]]
        polys += [R.padded(kp, r, pad) for r in src[1]]
        want.append(src[2])
    want = np.concatenate(want).astype(np.uint8)
    l_col, p_col = X.column(kl, lines), X.column(kp, polys)
    G = 16 if pad else 4
    lanes = lambda a, b: 16 if mean_coords(b) >= 32.0 else 4  # noqa: E731  (gpk_linearea.h relation_group_size: the polygon column's mean)
    sl, sp, exp, order = _relation_case(cus, G, l_col, p_col, want, seed=60 + G, lanes=lanes)
    n = len(order)
    assert n > cus * 32 * (256 // G)
    fn = _abi.lib().gpk_line_polygon_relation
    assert_masks(masks_on_device(fn, sl, sp), exp, order)
    assert lanes(None, p_col) == G
    assert_masks(masks_on_device(fn, sl, GeoSeries(p_col), rows=order), exp, order)


@pytest.mark.parametrize("ka,kb,pad", [(MLS, MLS, 0), (LS, MLS, 40)], ids=["mls-mls-G4", "ls-mls-G16"])
def test_line_relation_rows(gpk, cus, ka, kb, pad):
    A, B, want = [], [], []
    for a, b, w in (L.random_columns(ka, kb), L.case_columns(L.KNOWN, ka, kb, pad)[:3], L.case_columns(L.TIES, ka, kb, pad)[:3]):
        first = len(A) == 0
        A += [L.padded(ka, r, pad) for r in a] if first else list(a)
        B += [L.padded(kb, r, pad) for r in b] if first else list(b)
        want.append(np.asarray(w, dtype=np.uint8))
    want = np.concatenate(want)
    a_col, b_col = X.column(ka, A), X.column(kb, B)
    G = 16 if pad else 4
    sa, sb, exp, order = _relation_case(cus, G, a_col, b_col, want, seed=70 + G, lanes=_lanes_by_either_mean)
    n = len(order)
    assert n > cus * 32 * (256 // G)
    fn = _abi.lib().gpk_line_relation
    assert_masks(masks_on_device(fn, sa, sb), exp, order)
    assert_masks(masks_on_device(fn, sb, sa), L.swapped(exp), order)
    assert _lanes_by_either_mean(sa.array, b_col) == G
    assert_masks(masks_on_device(fn, sa, GeoSeries(b_col), rows=order), exp, order)


# ---- convex hull: the mid and big lists, the global-scratch sort, the class edges ---------------------------------------------------


def _point_sets(sizes, seed):
    """point sets of the given sizes in the styles of test_convex_hull_adversarial_point_sets, one style after the other"""
    rng = np.random.default_rng(seed)
    out = []
    for j, n in enumerate(sizes):
        k = np.arange(n)
        style = j % 6
        if style == 0:
            s = rng.normal(size=(n, 2)) * 50.0
        elif style == 1:  # a small lattice: duplicates and collinear triples everywhere
            s = rng.integers(0, 12, (n, 2)).astype(np.float64)
            s[0] = (-1.0, -3.0)  # (the first point occurs once: a row whose last coordinate repeats the first counts one point less)
        elif style == 2:  # convex position on a parabola (exact in doubles): nothing leaves
            x = (k - n // 2).astype(np.float64)
            s = rng.permutation(np.stack([x, x * x], axis=1))
        elif style == 3:  # all collinear
            s = rng.permutation(np.stack([k * 3.0 - 7.0, k * 6.0 + 1.0], axis=1))
        elif style == 4:  # every other point on the line y = 2x, through the likely extremes
            s = rng.integers(-40, 41, (n, 2)).astype(np.float64)
            s[::2, 1] = s[::2, 0] * 2.0
            s[0] = (-50.0, 7.0)
        else:  # a spiral: the filter needs many rounds
            ang = 2 * np.pi * 6 * k / n
            s = np.stack([np.cos(ang), np.sin(ang)], axis=1) * (1.0 + k[:, None] / n)
        out.append(np.ascontiguousarray(s))
    return out


def _closed(ring):
    ring = X.canon(ring)
    return np.concatenate([ring, ring[:1]]) if len(ring) else np.zeros((0, 2))


def _multipoints(sets, valid=None):
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    xy = np.concatenate([s.reshape(-1, 2) for s in sets]) if sets else np.zeros((0, 2))
    bits = None if valid is None else np.packbits(np.asarray(valid, dtype=np.uint8), bitorder="little")
    return GeoArrowArray(MP, xy, geom_offsets=off, validity=bits)


def _hull_reference(oracle, sets, valid):
    """the expected closed rings (a LINESTRING column, empty for null and empty rows): exact_ref.exact_hull, held against the oracle"""
    base = _multipoints(sets, valid)
    hx, ho = oracle.convex_hull(base)
    rings = []
    for i, s in enumerate(sets):
        if not valid[i] or len(s) == 0:
            rings.append(np.zeros((0, 2)))
            assert ho[i + 1] == ho[i]
            continue
        e = _closed(X.exact_hull(s))
        assert np.array_equal(X.canon(hx[ho[i] : ho[i + 1]]), X.canon(e)), i
        rings.append(e)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
    return base, GeoArrowArray(LS, np.concatenate(rings), geom_offsets=off)


def _check_hulls(col, want: GeoArrowArray):
    h = GeoSeries(col).convex_hull().array
    assert np.array_equal(h.ring_offsets, want.geom_offsets), np.nonzero(np.diff(h.ring_offsets) != np.diff(want.geom_offsets))[0][:8]
    bad = np.nonzero((h.xy != want.xy).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), np.searchsorted(want.geom_offsets, bad[:8], side="right") - 1)
    for g in np.linspace(0, len(col) - 1, 64).astype(int):  # starts at the smallest vertex, closed (the gathered rings do by construction)
        ring = h.xy[h.ring_offsets[g] : h.ring_offsets[g + 1]]
        if len(ring) >= 2:
            assert np.array_equal(ring[0], ring[-1]) and tuple(ring[0]) == min(map(tuple, ring))


def _hull_list_case(oracle, cus, sizes, rows_per_block, seed):
    """more listed rows than the list kernel's cus * 8 blocks take in one trip; a null, an empty and a short row after every fourth"""
    sets = _point_sets(sizes, seed)
    n_listed_base = len(sets)
    extra = [np.zeros((0, 2)), sets[0][:7], sets[1][:40], sets[0]]  # empty, two rows for the 64-point kernel, a null row with coordinates
    sets = sets + extra
    valid = [True] * len(sets)
    valid[-1] = False
    base, want = _hull_reference(oracle, sets, valid)
    n_listed = SP.second_trip_rows(cus, 8, rows_per_block)
    groups = cus * 8 * rows_per_block
    order_l = SP.shuffled_tiling(n_listed_base, n_listed, seed=seed + 1, groups=groups)
    rng = np.random.default_rng(seed + 2)
    pieces = np.split(order_l, np.arange(4, n_listed, 4))
    order = np.concatenate([np.concatenate([p, [n_listed_base + rng.integers(0, len(extra))]]) for p in pieces]).astype(np.int64)
    return base.take(order), want.take(order), n_listed, groups


def test_hull_big_list(gpk, oracle, cus):
    """hull_sort_big_kernel's LDS tile from one row to the next: rows of 129 .. 300 points of mixed sizes (the padded size P of the
    bitonic network is 256 or 512), more of them than cus * 8 work-groups"""
    sizes = [129, 130, 200, 255, 256, 257, 300, 131, 199, 260, 288, 129, 170, 256, 299, 150, 257, 222, 140, 300, 133, 258, 190, 275]
    col, want, n_listed, groups = _hull_list_case(oracle, cus, sizes, 1, seed=80)
    assert n_listed > cus * 8 * 1 and ((np.diff(col.geom_offsets) > 128) & col.is_valid()).sum() == n_listed
    _check_hulls(col, want)


def test_hull_mid_list(gpk, oracle, cus):
    """the listed 128-point instantiation of hull_small_kernel strides over mid_list: more than cus * 8 * 16 rows of 65 .. 128 points"""
    sizes = [65, 66, 100, 127, 128, 96, 70, 111, 128, 65, 90, 120, 77, 128, 101, 83, 65, 99, 125, 110, 68, 128, 88, 115]
    col, want, n_listed, groups = _hull_list_case(oracle, cus, sizes, 16, seed=90)
    n_pts = np.diff(col.geom_offsets)
    assert n_listed > cus * 8 * 16 and ((n_pts > 64) & (n_pts <= 128) & col.is_valid()).sum() == n_listed
    _check_hulls(col, want)


def test_hull_rows_around_the_lds_sort_limit(gpk, oracle):
    """single rows of 4095 .. 10 000 points: the LDS sort (up to HULL_BIG_LDS = 4096 points) against the sort in the global scratch, and
    the chain's index stack at that size; null and empty rows between the big ones"""
    sets, valid = [], []
    for n in (4095, 4096, 4097, 5000, 10000):
        for s in _point_sets([n] * 4, seed=n)[:4]:  # random, many duplicates, convex position (nothing leaves), all collinear
            sets += [s, np.zeros((0, 2)), s[:9]]
            valid += [True, True, False]
    base, want = _hull_reference(oracle, sets, valid)
    _check_hulls(base, want)


def test_hull_class_edges_through_a_closed_rings_dropped_duplicate(gpk, oracle):
    """closed rings of exactly 65, 129 and 4097 coordinates are 64, 128 and 4096 points (the closing duplicate is dropped before the
    row is classed); the same rings left open are one point more and fall into the next class"""
    rng = np.random.default_rng(7)
    lines = []
    for n in (65, 129, 4097):
        for pts in (rng.normal(size=(n - 1, 2)) * 30.0, rng.integers(0, 40, (n - 1, 2)).astype(np.float64)):
            # (the open ring repeats an inner point instead of the first: as many coordinates, another class, the same hull)
            assert tuple(pts[0]) != tuple(pts[1])
            lines += [np.concatenate([pts, pts[:1]]), np.concatenate([pts, pts[1:2]])]
    col = GeoArrowArray(LS, np.concatenate(lines), geom_offsets=np.concatenate([[0], np.cumsum([len(s) for s in lines])]).astype(np.int32))
    _, want = _hull_reference(oracle, lines, [True] * len(lines))
    for closed, opened in zip(range(0, len(lines), 2), range(1, len(lines), 2)):
        assert np.array_equal(want.xy[want.geom_offsets[closed] : want.geom_offsets[closed + 1]], want.xy[want.geom_offsets[opened] : want.geom_offsets[opened + 1]])
    _check_hulls(col, want)


# ---- affine, exterior -------------------------------------------------------------------------------------------------------------------


def test_affine_coordinates(gpk, cus):
    """gpk_affine_transform: 256 coordinates a block, cap cus * 8"""
    n = SP.second_trip_rows(cus, 8, 256, extra=cus * 2 * 256 + 100)
    assert n > cus * 8 * 256
    xy = np.random.default_rng(1).uniform(-1000.0, 1000.0, (n, 2))
    m = [1.25, -0.5, 10.0, 0.75, 2.0, -3.0]
    got = GeoSeries(GeoArrowArray.from_points(xy)).affine_transform(m).array.xy
    exp = np.stack([(m[0] * xy[:, 0] + m[1] * xy[:, 1]) + m[2], (m[3] * xy[:, 0] + m[4] * xy[:, 1]) + m[5]], axis=1)
    assert np.array_equal(got, exp)


def _polygon_base(pad):
    rows = [R.padded(PG, r, pad) for r in P.random_columns(PG, PG)[0] if len(r)] + [[]]
    return X.column(PG, rows, [i % 17 != 16 for i in range(len(rows))])


def _affine_group(col) -> int:
    G = 4
    while G < 64 and G * 2 * 8 <= mean_coords(col):  # gpk_unary.hip pick_group
        G <<= 1
    return G


@pytest.mark.parametrize("pad", [0, 15], ids=["G4", "G8"])
def test_affine_rows(gpk, cus, pad):
    """gpk_affine_transform_rows: 256 / G rows a block, cap cus * 16; bit-exact against the expression test_gpu_structural writes out"""
    base = _polygon_base(pad)
    G = _affine_group(base)
    assert (G == 4) == (pad == 0)
    n, groups = lane_group_rows(cus, G, cap_mult=16)
    assert n > cus * 16 * (256 // G)
    order = SP.shuffled_tiling(len(base), n, seed=100 + pad, groups=groups)
    col = base.take(order)
    assert _affine_group(col) == G
    s = GeoSeries(col)
    mats = np.random.default_rng(3).uniform(-2.0, 2.0, (n, 6))
    t_m = torch.from_numpy(mats).to(DEV)
    out = torch.full((col.n_coords, 2), -7.0, dtype=torch.float64, device=DEV)
    _abi.check(_abi.lib().gpk_affine_transform_rows(s.device().handle, t_m.data_ptr(), out.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    mm = mats[np.repeat(np.arange(n), np.diff(col.ring_offsets[col.geom_offsets]))]
    exp = np.stack([(mm[:, 0] * col.xy[:, 0] + mm[:, 1] * col.xy[:, 1]) + mm[:, 2], (mm[:, 3] * col.xy[:, 0] + mm[:, 4] * col.xy[:, 1]) + mm[:, 5]], axis=1)
    live = np.repeat(col.is_valid(), np.diff(col.ring_offsets[col.geom_offsets]))  # (what a null row's coordinates become is not specified)
    assert np.array_equal(out.cpu().numpy()[live], exp[live])


@pytest.mark.parametrize("pad", [0, 7], ids=["4-lanes", "16-lanes"])
def test_exterior_rows(gpk, cus, pad):
    """gpk_exterior's copy: 16 rows a block, cap cus * 16, the instance for a mean of at most 12 coordinates and the 16-lane one"""
    base = _polygon_base(pad)
    n = SP.second_trip_rows(cus, 16, 16)
    assert n > cus * 16 * 16
    order = SP.shuffled_tiling(len(base), n, seed=110 + pad, groups=cus * 16 * 16)
    col = base.take(order)
    assert (mean_coords(col) <= 12.0) == (pad == 0)
    ext = GeoSeries(col).exterior().array
    has = col.is_valid() & (np.diff(col.geom_offsets) > 0)  # null and empty rows have no exterior
    r0 = np.where(has, col.geom_offsets[:-1], 0).astype(np.int64)
    first = col.ring_offsets[r0].astype(np.int64)
    size = np.where(has, col.ring_offsets[r0 + 1] - first, 0)
    off = np.concatenate([[0], np.cumsum(size)])
    assert np.array_equal(ext.geom_offsets, off.astype(np.int32))
    src = np.repeat(first - off[:-1], size) + np.arange(off[-1])
    assert np.array_equal(ext.xy, col.xy[src])


# ---- geodesic length ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("method,G", [("haversine", 4), ("vincenty", 16), ("geodesic", 16)])
def test_geodesic_length_rows(gpk, oracle, cus, method, G):
    """geodesic_seq_kernel: 256 / G sequences a block, cap cus * 32; the oracle's length per base row within the parity tests' 1e-9,
    every copy of a base row bit-identical to the small column's value at the same G"""
    from tests import geodesic_ref as Gd
    from tests.test_gpu_lineal_ops import _close, _lonlat_seq

    m_id = GeoSeries.GEODESIC_METHODS[method]
    rng = np.random.default_rng(120 + G + 7 * m_id)
    lengths = [0, 1, 2, G, G + 1, 3 * G + 1] * 6 + [5, 9, 2 * G, 0] + ([150] * 12 if G == 16 else [])
    seqs = [_lonlat_seq(rng, k) for k in lengths]
    valid = np.array([i % 6 != 5 for i in range(len(seqs))])
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int32)
    base = GeoArrowArray(LS, np.array([c for s in seqs for c in s]).reshape(-1, 2), geom_offsets=off, validity=np.packbits(valid, bitorder="little"))
    if method != "geodesic":  # (Karney's kernel always takes 16 lanes)
        assert Gd.geodesic_group_size(base.n_coords, len(base)) == G
    small = GeoSeries(base).geodesic_length(method)
    assert _close(small, oracle.geodesic_length(base, method)) and np.isnan(small[~valid]).all()
    n, groups = lane_group_rows(cus, G)
    assert n > cus * 32 * (256 // G)
    order = SP.shuffled_tiling(len(base), n, seed=121 + G + 7 * m_id, groups=groups)
    col = base.take(order)
    if method != "geodesic":
        assert Gd.geodesic_group_size(col.n_coords, len(col)) == G
    out = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    s = GeoSeries(col)  # (kept alive over the call: the device column is freed with its series)
    _abi.check(_abi.lib().gpk_geodesic_length(s.device().handle, m_id, out.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert _close(got, oracle.geodesic_length(base, method)[order])
    assert SP.same_bits(got, small[order])


# ---- line interpolate -----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("G", [1, 8, 32])
def test_interpolate_rows(gpk, cus, G):
    """interpolate_point_kernel<G>: 256 / G rows a block, cap cus * 32, one distance per row"""
    from tests import linref_ref as F

    rng = np.random.default_rng(130 + G)
    lo, hi = X._VERTS[G]
    kind = MLS if G == 8 else LS
    rows = []
    for i in range(40):
        walk = lambda k: [(float(x), float(y)) for x, y in np.cumsum(rng.uniform(-5.0, 5.0, (k, 2)), axis=0) + rng.uniform(0, 1000.0, 2)]  # noqa: E731
        k = int(rng.integers(lo, hi + 1))
        rows.append(walk(k) if kind == LS else [walk(max(1, k // 2)), [], walk(max(2, k - k // 2))])
    rows[5] = [] if kind == LS else [[], []]
    valid = [i != 9 for i in range(40)]
    base = X.column(kind, rows, valid)
    assert X.group_size_of(base) == G
    length = np.array([float(F.total_length(kind, r)) for r in rows])
    d_base = rng.uniform(-0.2, 1.2, 40) * length * rng.choice([1.0, -1.0], 40)
    d_base[3] = np.nan
    small = GeoSeries(base).interpolate(d_base)
    for j, row in enumerate(rows):
        ex = F.interpolate(kind, row, float(d_base[j])) if valid[j] else None
        g = small.array.xy[j]
        if ex is None:
            assert np.isnan(g).all() and not small.array.is_valid()[j], j
        else:
            assert small.array.is_valid()[j] and F.dec_err(g[0], ex[0]) <= F.M_REL * length[j] and F.dec_err(g[1], ex[1]) <= F.M_REL * length[j], (j, g, ex)
    n, groups = lane_group_rows(cus, G)
    assert n > cus * 32 * (256 // G)
    order = SP.shuffled_tiling(40, n, seed=131 + G, groups=groups)
    col = base.take(order)
    assert X.group_size_of(col) == G
    s = GeoSeries(col)
    xy = torch.full((n, 2), -7.0, dtype=torch.float64, device=DEV)
    ok = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    t_d = torch.from_numpy(np.ascontiguousarray(d_base[order])).to(DEV)
    _abi.check(_abi.lib().gpk_line_interpolate_point(s.device().handle, t_d.data_ptr(), n, 0, xy.data_ptr(), ok.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    assert np.array_equal(ok.cpu().numpy().astype(bool), small.array.is_valid()[order])
    assert SP.same_bits(xy.cpu().numpy(), small.array.xy[order])  # (the small column's values were held against the exact reference above)


# ---- distance between two non-point columns, dwithin -----------------------------------------------------------------------------------

PAIR_CASES = {8: (LS, PG, 12, 9), 32: (MPG, MLS, 160, 140)}  # G: (kind a, kind b, coordinates a row in a, in b)


def _pair_base(G, n=20):
    from tests.test_gpu_distance_pairs import pair_column, pair_group_size

    ka, kb, nva, nvb = PAIR_CASES[G]
    ra, rb = pair_column(ka, kb, nva, nvb, n=n, seed=140)
    ra[7], rb[11] = [], []
    va, vb = [i != 3 for i in range(n)], [i != 13 for i in range(n)]
    a, b = X.column(ka, ra, va), X.column(kb, rb, vb)
    assert pair_group_size(a, b) == G
    return ka, ra, va, a, kb, rb, vb, b


def _distance_on_device(a: GeoSeries, b: GeoSeries, rows=None):
    out = torch.full((len(a),), -7.0, dtype=torch.float64, device=DEV)
    r = None if rows is None else u32_dev(rows)
    _abi.check(_abi.lib().gpk_distance_rowwise(a.device().handle, b.device().handle, None if r is None else r.data_ptr(), out.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("G", [8, 32])
def test_pair_distance_rows(gpk, cus, G):
    """pairdist_kernel<G>: 256 / G rows a block, cap cus * 16"""
    from tests import pair_distance_ref as D
    from tests.test_gpu_distance_pairs import pair_group_size

    ka, ra, va, a, kb, rb, vb, b = _pair_base(G)
    exact = D.rowwise(ka, ra, kb, rb, valid_a=va, valid_b=vb)
    small = _distance_on_device(GeoSeries(a), GeoSeries(b))
    D.check(small, exact, ("small", G))
    n, groups = lane_group_rows(cus, G, cap_mult=16)
    assert n > cus * 16 * (256 // G)
    order = SP.shuffled_tiling(len(ra), n, seed=141 + G, groups=groups)
    ta, tb = a.take(order), b.take(order)
    assert pair_group_size(ta, tb) == G
    got = _distance_on_device(GeoSeries(ta), GeoSeries(tb))
    first = SP.first_rows(order, len(ra))
    D.check(got[first], exact, ("tiled", G))
    assert SP.same_bits(got, small[order])
    assert pair_group_size(ta, b) == G  # b_rows: the tiled A against the base B
    assert SP.same_bits(_distance_on_device(GeoSeries(ta), GeoSeries(b), rows=order), small[order])


def _large_pairs():
    """four LINESTRING x POLYGON pairs with n_A * n_B > PD_LARGE_COST and different staged lengths, intersecting and apart, and six small ones"""
    from tests.test_gpu_distance_pairs import LARGE_COST, make_row, row_coords

    rng = np.random.default_rng(150)
    ra, rb = [], []
    for i, (nva, nvb, off) in enumerate([(257, 263, 0.0), (320, 280, 3.0), (270, 250, 0.0), (400, 170, 20.0), (12, 9, 0.0), (12, 9, 3.0), (9, 14, 0.6), (20, 11, 1.1),
                                         (12, 9, 20.0), (16, 16, 0.0)]):
        cx, cy = 1000.0 * i, 500.0 * i
        ra.append(make_row(LS, rng, cx, cy, 40.0, nva))
        rb.append(make_row(PG, rng, cx + off * 40.0, cy + 0.3 * off * 40.0, 40.0, nvb))
    costs = [row_coords(LS, x) * row_coords(PG, y) for x, y in zip(ra, rb)]
    assert all(c > LARGE_COST for c in costs[:4]) and all(c <= LARGE_COST for c in costs[4:])
    return ra, rb


def _large_pair_order(cus):
    n_large = SP.second_trip_rows(cus, 4, 1)
    assert n_large > cus * 4 * 1
    return _interleaved(SP.rotating_tiling(4, n_large, groups=cus * 4), 4, 6, seed=151), n_large


def test_pair_distance_large_rows(gpk, cus):
    """pairdist_large_kernel: one listed row a work-group, cus * 4 work-groups; consecutive trips stage different lengths"""
    from tests import pair_distance_ref as D

    ra, rb = _large_pairs()
    exact = D.rowwise(LS, ra, PG, rb)
    assert [d == 0 for d, _ in exact[:4]] == [True, False, True, False]  # (both outcomes: crossing and apart)
    a, b = X.column(LS, ra), X.column(PG, rb)
    small = _distance_on_device(GeoSeries(a), GeoSeries(b))
    D.check(small, exact, "small")
    order, n_large = _large_pair_order(cus)
    assert n_large > cus * 4
    got = _distance_on_device(GeoSeries(a.take(order)), GeoSeries(b.take(order)))
    D.check(got[SP.first_rows(order, len(ra))], exact, "tiled")
    assert SP.same_bits(got, small[order])
    assert SP.same_bits(_distance_on_device(GeoSeries(b.take(order)), GeoSeries(a.take(order))), got)  # (the other order of the families: the same value)


def _dwithin_on_device(a: GeoSeries, b: GeoSeries, t, rows=None):
    out = torch.full((len(a),), SENTINEL, dtype=torch.uint8, device=DEV)
    r = None if rows is None else u32_dev(rows)
    _abi.check(_abi.lib().gpk_dwithin_rowwise(a.device().handle, b.device().handle, None if r is None else r.data_ptr(), float(t), out.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _within(exact, t):
    """expected dwithin answers from exact distances; no pair may be so close to t that the f64 distance could fall on the other side"""
    out = []
    for d, bound in exact:
        if d is None:
            out.append(0)
            continue
        assert d == 0 or X.abs_err(float(t), d) > bound, (t, d)
        out.append(int(d <= Fraction(float(t))))
    return np.array(out, dtype=np.uint8)


DWITHIN_T = 60.0


@pytest.mark.parametrize("G", [8, 32])
def test_dwithin_rows(gpk, cus, G):
    """gpk_dwithin_rowwise of two non-point columns: gpk_distance_rowwise's pairdist_kernel<G> (256 / G rows a block, cap cus * 16)
    and a threshold on its result; the join's own refine kernels are run by the test_dwithin_join_* tests"""
    from tests import pair_distance_ref as D
    from tests.test_gpu_distance_pairs import pair_group_size

    ka, ra, va, a, kb, rb, vb, b = _pair_base(G)
    want = _within(D.rowwise(ka, ra, kb, rb, valid_a=va, valid_b=vb), DWITHIN_T)
    assert 4 <= want.sum() <= len(want) - 6
    n, groups = lane_group_rows(cus, G, cap_mult=16)
    assert n > cus * 16 * (256 // G)
    order = SP.shuffled_tiling(len(ra), n, seed=160 + G, groups=groups)
    ta, tb = a.take(order), b.take(order)
    assert pair_group_size(ta, tb) == G
    assert_masks(_dwithin_on_device(GeoSeries(ta), GeoSeries(tb), DWITHIN_T), want[order], order)
    assert_masks(_dwithin_on_device(GeoSeries(tb), GeoSeries(ta), DWITHIN_T), want[order], order)
    assert pair_group_size(ta, b) == G
    assert_masks(_dwithin_on_device(GeoSeries(ta), GeoSeries(b), DWITHIN_T, rows=order), want[order], order)


def test_dwithin_large_rows(gpk, cus):
    """gpk_dwithin_rowwise over more large rows than pairdist_large_kernel has work-groups (cus * 4): the thresholded distances"""
    from tests import pair_distance_ref as D

    ra, rb = _large_pairs()
    want = _within(D.rowwise(LS, ra, PG, rb), DWITHIN_T)
    assert want[:4].tolist() == [1, 0, 1, 0]
    a, b = X.column(LS, ra), X.column(PG, rb)
    order, n_large = _large_pair_order(cus)
    assert n_large > cus * 4
    assert_masks(_dwithin_on_device(GeoSeries(a.take(order)), GeoSeries(b.take(order)), DWITHIN_T), want[order], order)
    far = 2000.0  # every row within
    assert_masks(_dwithin_on_device(GeoSeries(a.take(order)), GeoSeries(b.take(order)), far), _within(D.rowwise(LS, ra, PG, rb), far)[order], order)


# ---- representative point ---------------------------------------------------------------------------------------------------------------


def _interior_fillers(fam):
    from tests import interior_ref as I

    line = lambda k, m: [(float(i), float((i * 7) % m)) for i in range(k)]  # noqa: E731
    return {"pg": ([I.TRI], [I.comb(17)]), "mpg": ([[I.TRI]], [[I.comb(17)], [I.L_SHAPE]]), "ls": (line(3, 2), line(70, 5)),
            "mls": ([line(2, 2), line(3, 3)], [line(50, 5), [], line(41, 7)])}[fam]


def _interior_base(fam, G):
    """the family's fixture rows of at most INT_BLOCK_COORDS coordinates, with filler rows until the mean picks G with a margin"""
    from tests import interior_ref as I

    kind = I.FAMILIES[fam]
    _, rows, valid = I.family_rows(fam)
    keep = [i for i, r in enumerate(rows) if len(I.row_coords(kind, r)) <= I.BLOCK_COORDS]
    rows, valid = [rows[i] for i in keep], [valid[i] for i in keep]
    if len(rows) < 24:  # (a shuffled tiling needs more than a dozen different rows: the same rows again, moved and mirrored)
        rows, valid = rows + [map_coords(r, lambda x, y: (y + 100.0, x - 50.0)) for r in rows], valid + valid
    light, heavy = _interior_fillers(fam)
    mean = lambda: sum(len(I.row_coords(kind, r)) for r in rows) / len(rows)  # noqa: E731
    while (mean() >= 0.8 * I.G_MEAN) if G == I.G_SMALL else (mean() < 1.25 * I.G_MEAN):
        rows.append(light if G == I.G_SMALL else heavy)
        valid.append(True)
    return kind, rows, valid


def _interior_check(kind, rows, valid, col, order):
    """the tiled column's answers through device buffers (prefilled with 7.0 / 9): the first copy of every base row against the exact
    reference, every copy bit-identical to the base column's own run"""
    from tests import interior_ref as I
    from tests.test_gpu_interior import abi_answers, check_column

    base = X.column(kind, rows, valid)
    group = lambda c: I.G_LARGE if mean_coords(c) >= I.G_MEAN else I.G_SMALL  # noqa: E731
    assert group(base) == group(col)
    small = abi_answers(GeoSeries(base).device(), len(base), "device")
    check_column(kind, I.column_rows(base), np.asarray(valid), *small)
    got = abi_answers(GeoSeries(col).device(), len(col), "device")
    first = SP.first_rows(order, len(rows))
    check_column(kind, I.column_rows(base), np.asarray(valid), got[0][first], got[1][first], got[2][first])
    assert np.array_equal(got[1], small[1][order])
    assert SP.same_bits(got[0], small[0][order]) and SP.same_bits(got[2], small[2][order])
    return group(col)


@pytest.mark.parametrize("G", [4, 16], ids=["G4", "G16"])
@pytest.mark.parametrize("fam", ["pg", "mpg", "ls", "mls"])
def test_representative_point_rows(gpk, cus, fam, G):
    """interior_poly_rows_kernel / the vertex families' rows kernel: 256 / G rows a block, cap cus * 32.  The combs above the slice
    capacity are queued by the lane groups, so the work-group kernel's list is longer than its cus * 8 blocks here too."""
    kind, rows, valid = _interior_base(fam, G)
    n, groups = lane_group_rows(cus, G)
    assert n > cus * 32 * (256 // G)
    order = SP.shuffled_tiling(len(rows), n, seed=170 + G + kind, groups=groups)
    col = X.column(kind, rows, valid).take(order)
    assert _interior_check(kind, rows, valid, col, order) == G


def _interior_large_rows(fam):
    from tests import interior_ref as I

    if fam == "pg":
        shapes = [[I.rect(0, 0, 7, 3)], [I.L_SHAPE], [I.U_SHAPE], I.RING_SHAPE, I.holed((2, 3), (12, 13), (16, 17)), [I.comb(3, wide=1)], [I.comb(16, wide=11)], [I.TRI]]
        large = [[I.pad_base(row[0], I.BLOCK_COORDS + 1 + 37 * i + 150 * j)] + list(row[1:]) for j in range(2) for i, row in enumerate(shapes)]
        small = [r for _, r in I.polygon_rows() if len(I.row_coords(I.PG, r)) <= I.BLOCK_COORDS]
        return I.PG, large, small
    large = [[(float(i), float((i * 7) % (11 + k))) for i in range(I.BLOCK_COORDS + 1 + 29 * k)] for k in range(16)]
    small = [r for _, r in I.line_rows() if len(r) <= I.BLOCK_COORDS]
    return I.LS, large, small


@pytest.mark.parametrize("fam", ["pg", "ls"])
def test_representative_point_large_rows(gpk, cus, fam):
    """more rows above INT_BLOCK_COORDS than the work-group kernel has blocks (cus * 8), small rows between them"""
    from tests import interior_ref as I

    kind, large, small = _interior_large_rows(fam)
    assert all(len(I.row_coords(kind, r)) > I.BLOCK_COORDS for r in large)
    rows = large + small
    n_large = SP.second_trip_rows(cus, 8, 1)
    assert n_large > cus * 8 * 1
    order = _interleaved(SP.shuffled_tiling(len(large), n_large, seed=180 + kind, groups=cus * 8), len(large), len(small), seed=181)
    col = X.column(kind, rows).take(order)
    _interior_check(kind, rows, [True] * len(rows), col, order)


# ---- join refines: every candidate of a join goes to its refine in one launch -------------------------------------------------------


def _tiled_pairs(pairs_b, n_left_base, order):
    """base pairs sorted by (l, r) -> (pairs, counts per left row, index of every pair in pairs_b) of the left column tiled by `order`"""
    cnt = np.bincount(pairs_b[:, 0], minlength=n_left_base).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)])
    k = cnt[order]
    new = np.concatenate([[0], np.cumsum(k)])
    src = np.repeat(off[order] - new[:-1], k) + np.arange(new[-1])
    pairs = np.stack([np.repeat(np.arange(len(order)), k), pairs_b[src, 1]], axis=1).astype(np.uint32)
    return pairs, k.astype(np.uint32), src


def _join_case(cus, G, pairs_b, n_left_base, seed, cap_mult=32, per_block=None):
    """(order of the left column, expected pairs, counts, index of every pair among the base pairs): the expected pairs alone — a
    lower bound of the candidates — outnumber the candidates the refine's capped grid takes in one trip, and the pair a group
    meets a trip later is another base pair"""
    per_block = 256 // G if per_block is None else per_block
    cap_pairs = cus * cap_mult * per_block
    n_left = int(1.25 * cap_pairs / (len(pairs_b) / n_left_base)) + n_left_base
    rng = np.random.default_rng(seed)
    order = np.concatenate([rng.permutation(n_left_base), rng.integers(0, n_left_base, n_left - n_left_base)]).astype(np.int64)
    pairs, counts, src = _tiled_pairs(pairs_b, n_left_base, order)
    assert len(pairs) > cap_pairs
    if per_block != 1:  # (a work-group list is filled by atomics, in scattered order: the column's order does not say which pair comes a trip later)
        assert (src[:-cap_pairs] != src[cap_pairs:]).mean() >= 0.9
    return order, pairs, counts, src


@pytest.mark.parametrize("ka,kb,pad", [(PG, PG, 0), (MPG, MPG, 7)], ids=["pg-pg-G4", "mpg-mpg-G16"])
def test_polygon_relation_join(gpk, cus, ka, kb, pad):
    import ctypes as C

    from geopolars_amd.spatial_index import polygon_relation_pairs

    left, lv, right, rv, table, _ = P.join_fixture(ka, kb)
    a = X.column(ka, [R.padded(ka, r, pad) for r in left], lv)
    b = X.column(kb, [R.padded(kb, r, pad) for r in right], rv)
    G = 16 if pad else 4
    p0, c0, m0 = P.expected_pairs(table, "intersects")
    order, pairs, counts, src = _join_case(cus, G, p0, len(left), seed=190 + G)
    n_pairs = len(pairs)
    assert n_pairs > cus * 32 * (256 // G)
    sl, sr = GeoSeries(a.take(order)), GeoSeries(b)
    assert _lanes_by_either_mean(sl.array, b) == G
    got_p, got_c, got_m = polygon_relation_pairs(sl, sr, "intersects")
    assert np.array_equal(got_c, counts) and np.array_equal(got_p, pairs) and np.array_equal(got_m, m0[src])
    n = C.c_int64(-1)  # count-only: the early-exit form of the refine
    assert _abi.lib().gpk_polygon_relation_join(sl.device().handle, sr.device().handle, None, P.PRED_IDS["intersects"], 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_OK
    assert n.value == n_pairs


@pytest.mark.parametrize("kl,kp,pad", [(LS, PG, 0), (MLS, MPG, 7)], ids=["ls-pg-G4", "mls-mpg-G16"])
def test_line_polygon_join(gpk, cus, kl, kp, pad):
    from geopolars_amd.spatial_index import relation_pairs

    lines, lv, polys, pv, table = R.join_fixture(kl, kp)
    a = X.column(kl, [R.scaled_line(kl, r, pad) for r in lines], lv)
    b = X.column(kp, [R.padded(kp, r, pad) for r in polys], pv)
    G = 16 if mean_coords(b) >= 32.0 else 4
    assert G == (16 if pad else 4)
    p0, c0, m0 = R.expected_pairs(table, "intersects")
    order, pairs, counts, src = _join_case(cus, G, p0, len(lines), seed=200 + G)
    n_pairs = len(pairs)
    assert n_pairs > cus * 32 * (256 // G)
    got_p, got_c, got_m = relation_pairs(GeoSeries(a.take(order)), GeoSeries(b), "intersects")
    assert np.array_equal(got_c, counts) and np.array_equal(got_p, pairs) and np.array_equal(got_m, m0[src])


@pytest.mark.parametrize("ka,kb,pad", [(LS, LS, 0), (MLS, MLS, 40)], ids=["ls-ls-G4", "mls-mls-G16"])
def test_line_relation_join(gpk, cus, ka, kb, pad):
    from geopolars_amd.spatial_index import line_relation_pairs

    left, lv, right, rv, table, _ = L.join_fixture(ka, kb)
    a = X.column(ka, [L.padded(ka, r, pad) for r in left], lv)
    b = X.column(kb, [L.padded(kb, r, pad) for r in right], rv)
    G = _lanes_by_either_mean(a, b)
    assert G == (16 if pad else 4)
    p0, c0, m0 = L.expected_pairs(table, "intersects")
    order, pairs, counts, src = _join_case(cus, G, p0, len(left), seed=210 + G)
    n_pairs = len(pairs)
    assert n_pairs > cus * 32 * (256 // G)
    sl = GeoSeries(a.take(order))
    assert _lanes_by_either_mean(sl.array, b) == G
    got_p, got_c, got_m = line_relation_pairs(sl, GeoSeries(b), "intersects")
    assert np.array_equal(got_c, counts) and np.array_equal(got_p, pairs) and np.array_equal(got_m, m0[src])


# ---- the dwithin join: point refine, pair refine and the pair refine's large list ----------------------------------------------------


def _dwithin_fixture(key):
    """(left, right, exact table) of a dwithin_ref fixture; the 32-lane and the large pair fixtures hold only a few rows a side, so two
    of them (two seeds) are joined into one: more different pairs than a refine group meets in a row"""
    from tests import dwithin_ref as W

    if isinstance(key[0], str):
        return (*W.point_fixture(*key), W.fixture_table(key))
    if key[2] == "g8":
        return (*W.pair_fixture(*key), W.fixture_table(key))
    parts = [W.pair_fixture(*key, seed=s) for s in (0, 1)]
    left = (key[0], [r for p in parts for r in p[0][1]], [v for p in parts for v in p[0][2]])
    right = (key[1], [r for p in parts for r in p[1][1]], [v for p in parts for v in p[1][2]])
    return left, right, W.exact_table(left, right)


def _dwithin_join(cus, key, t, G, cap_mult=32, per_block=None, seed=220):
    """a dwithin fixture of tests/dwithin_ref.py with its left column tiled: pairs and counts against the exact table, the distances
    bit-identical to the base join's, which are held against the exact distances"""
    from geopolars_amd.spatial_index import dwithin_pairs
    from tests import dwithin_ref as W

    left, right, table = _dwithin_fixture(key)
    within, close = W.classify(table, t, exact_zero=not isinstance(key[0], str))
    assert close == [] and len(within) >= 8
    p0 = np.array(within, dtype=np.uint32).reshape(-1, 2)
    a, b = W.columns(left, right)
    sr = GeoSeries(b)
    bp, bc, bd = dwithin_pairs(GeoSeries(a), sr, t)
    assert np.array_equal(bp, p0)
    for (l, r), d in zip(within, bd):
        d2, lmax = table[(l, r)]
        exact = X.dec_sqrt(d2)
        assert X.abs_err(float(d), exact) <= X.distance_bound(float(exact), lmax), (l, r, d)
    order, pairs, counts, src = _join_case(cus, G, p0, len(a), seed, cap_mult, per_block)
    got_p, got_c, got_d = dwithin_pairs(GeoSeries(a.take(order)), sr, t)
    assert np.array_equal(got_c, counts) and np.array_equal(got_p, pairs)
    assert SP.same_bits(got_d, bd[src])
    return a.take(order), b, len(pairs)


@pytest.mark.parametrize("family,G", [("linestring", 1), ("polygon", 8), ("multipolygon", 32)])
def test_dwithin_join_point_refine(gpk, cus, family, G):
    from tests import dwithin_ref as W

    key = (family, G, True)
    assert key in W.POINT_FIXTURES
    a, b, n_pairs = _dwithin_join(cus, key, 400.0, G)
    assert n_pairs > cus * 32 * (256 // G) and X.group_size_of(b) == G


@pytest.mark.parametrize("size,G", [("g8", 8), ("g32", 32)])
def test_dwithin_join_pair_refine(gpk, cus, size, G):
    from tests.test_gpu_distance_pairs import pair_group_size

    a, b, n_pairs = _dwithin_join(cus, (LS, PG, size), 60.0 if size == "g8" else 400.0, G)
    assert n_pairs > cus * 32 * (256 // G) and pair_group_size(a, b) == G


def test_dwithin_join_large_list(gpk, cus):
    """every pair of the fixture costs more than PD_LARGE_COST: the refine lists them all for dwithin_pair_large_kernel's cus * 4 work-groups"""
    from tests import dwithin_ref as W
    from tests.test_gpu_distance_pairs import row_coords

    left, right, _ = _dwithin_fixture((MLS, MPG, "large"))
    assert min(row_coords(MLS, x) for x in left[1]) * min(row_coords(MPG, y) for y in right[1]) > W.LARGE_COST
    a, b, n_pairs = _dwithin_join(cus, (MLS, MPG, "large"), 400.0, 32, cap_mult=4, per_block=1)
    assert n_pairs > cus * 4 * 1


# ---- the intersection measure join ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("what", ["area", "length"])
def test_intersection_measure_join(gpk, cus, what):
    """the overlay refine past its cap: pairs and counts from the golden table's exact measures, the measures within the contract's
    tolerance of them and bit for bit the row-wise measure of the pair"""
    from geopolars_amd.spatial_index import intersection_measure_pairs
    from tests import overlay_ref as O
    from tests.test_gpu_overlay import JOIN_TOL_AREA, JOIN_TOL_LENGTH, THETA, expected, lanes_of, pair_tolerance, rowwise_of_pairs

    golden = np.load(O.GOLDEN)
    kind = PG if what == "area" else LS
    l = GeoSeries(O.unpack(golden, "join_left_" if what == "area" else "join_lines_", kind))
    r = GeoSeries(O.unpack(golden, "join_right_", PG))
    tol = JOIN_TOL_AREA if what == "area" else JOIN_TOL_LENGTH
    p0, c0, exact0 = expected(golden[f"join_{what}"], len(l), THETA, tol)
    bp, bc, bm = intersection_measure_pairs(l, r, THETA)
    assert np.array_equal(bp, p0) and np.array_equal(bm, rowwise_of_pairs(l, r, kind, p0))
    each = pair_tolerance(l, r, kind, p0)
    assert (np.abs(bm - exact0) <= each).all()
    G = lanes_of(l, r)
    order, pairs, counts, src = _join_case(cus, G, p0, len(l), seed=230)
    n_pairs = len(pairs)
    assert n_pairs > cus * 32 * (256 // G)
    tl = GeoSeries(l.array.take(order))
    assert lanes_of(tl, r) == G
    got_p, got_c, got_m = intersection_measure_pairs(tl, r, THETA)
    assert np.array_equal(got_c, counts) and np.array_equal(got_p, pairs)
    assert (np.abs(got_m - exact0[src]) <= each[src]).all() and SP.same_bits(got_m, bm[src])


# ---- locate and closest point: tiles of LINREF_TILE points -----------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["linestrings", "multilinestrings"])
def test_locate_and_closest_point_tiles(gpk, cus, name):
    """gpk_line_locate_point and gpk_closest_point_rowwise take tiles of 2048 points on a grid capped at cus * 16 tiles: the reference
    points of linref_ref tiled over their lines (a b_rows map into the small line column), every copy bit-identical to the small run,
    which test_gpu_linref's checker holds against the exact reference"""
    from tests import linref_ref as F
    from tests.test_gpu_linref import check_closest

    tile = 2048  # LINREF_TILE
    col, pts = F.random_columns()[name]
    assert X.group_size_of(col) == 8  # (the kernels are instantiated per lane-group size; the tile loop around them is one)
    q0, seg0 = check_closest(pts, col, max_ambiguous=0.01 * len(pts), what=name)
    S = GeoSeries(col)
    m0 = S.project(GeoSeries(GeoArrowArray.from_points(pts)))
    n = SP.second_trip_rows(cus, 16, tile, extra=cus * 2 * tile + 100)
    assert n > cus * 16 * tile
    order = SP.shuffled_tiling(len(pts), n, seed=240, groups=cus * 16 * tile)
    P_dev = GeoSeries(GeoArrowArray.from_points(pts[order])).device()
    rows = u32_dev(order)
    xy = torch.full((n, 2), -1.0, dtype=torch.float64, device=DEV)
    seg = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    m = torch.full((n,), -1.0, dtype=torch.float64, device=DEV)
    lib = _abi.lib()
    _abi.check(lib.gpk_closest_point_rowwise(P_dev.handle, S.device().handle, rows.data_ptr(), xy.data_ptr(), seg.data_ptr(), _abi.MEM_DEVICE, None))
    _abi.check(lib.gpk_line_locate_point(P_dev.handle, S.device().handle, rows.data_ptr(), 0, m.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    assert np.array_equal(seg.cpu().numpy(), seg0[order])
    assert SP.same_bits(xy.cpu().numpy(), q0[order]) and SP.same_bits(m.cpu().numpy(), m0[order])


# ---- the sequence reductions' class lists, the row-wise predicates ---------------------------------------------------------------------

SEQ_CLASSES = {2: (2, 16), 8: (17, 128), 16: (129, 220)}  # lanes: coordinates of a sequence (gpk_unary.hip SEQ_LANES / SEQ_MAXLEN, the third up to 512)


@pytest.mark.parametrize("lanes", [2, 8, 16])
def test_sequence_class_lists(gpk, cus, lanes):
    """seq_stats_kernel gives every length class its own blocks, 256 / lanes sequences each, capped at cus * 16 a class: more
    sequences of one class than that, through euclidean_length, against exact lengths within the a-priori bound"""
    lo, hi = SEQ_CLASSES[lanes]
    rng = np.random.default_rng(250 + lanes)
    seqs = [np.cumsum(rng.uniform(-3.0, 3.0, (int(k), 2)), axis=0) + rng.uniform(0.0, 500.0, 2) for k in np.linspace(lo, hi, 40).astype(int)]
    base = GeoArrowArray(LS, np.concatenate(seqs), geom_offsets=np.concatenate([[0], np.cumsum([len(q) for q in seqs])]).astype(np.int32))
    small = GeoSeries(base).euclidean_length()
    for i, q in enumerate(seqs):
        e = X.exact_length([q])
        assert X.abs_err(small[i], e) <= X.length_bound([q], float(e)), i
    per_block = 256 // lanes
    n = SP.second_trip_rows(cus, 16, per_block)
    assert n > cus * 16 * per_block
    order = SP.shuffled_tiling(40, n, seed=251 + lanes, groups=cus * 16 * per_block)
    out = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    s = GeoSeries(base.take(order))  # (kept alive over the call: the device column is freed with its series)
    _abi.check(_abi.lib().gpk_euclidean_length(s.device().handle, out.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    assert SP.same_bits(out.cpu().numpy(), small[order])


def _predicate_on_device(a: GeoSeries, b: GeoSeries, name, rows=None):
    out = torch.full((len(a),), SENTINEL, dtype=torch.uint8, device=DEV)
    r = None if rows is None else u32_dev(rows)
    _abi.check(_abi.lib().gpk_predicate_rowwise(a.device().handle, b.device().handle, None if r is None else r.data_ptr(), _abi.PREDICATES[name], out.data_ptr(),
                                                _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("kind,G", [(PG, 1), (MPG, 16), (PG, 64)])
def test_point_polygon_predicate_rows(gpk, cus, kind, G):
    """point_poly_predicate_kernel<G>: 256 / G points a block, cap cus * 32; the probes of the exact fixture tiled over its polygon
    column through a b_rows map"""
    from tests import exact_predicates as E

    fx = E.point_poly_fixture(kind, G)
    n, groups = lane_group_rows(cus, G)
    assert n > cus * 32 * (256 // G)
    order = SP.shuffled_tiling(len(fx["points"]), n, seed=260 + G, groups=groups)
    q, polys = GeoSeries(GeoArrowArray.from_points(fx["points"][order])), GeoSeries(fx["array"])
    rows = fx["rows_of"][order]
    assert_masks(_predicate_on_device(q, polys, "within", rows), fx["inside"][order].astype(np.uint8), order)
    assert_masks(_predicate_on_device(q, polys, "intersects", rows), fx["not_outside"][order].astype(np.uint8), order)


@pytest.mark.parametrize("ka,kb", [(PG, PG), (MPG, MPG)], ids=["pg-pg", "mpg-mpg"])
def test_polygon_predicate_rows(gpk, cus, ka, kb):
    """poly_poly_intersects_kernel / poly_poly_contains_kernel: 16 lanes a row, 16 rows a block, cap cus * 32; intersects, contains and
    within as the exact relation masks state them (test_gpu_polyrel holds the same statement on the base rows)"""
    A, B, m = P.random_columns(ka, kb)
    m = np.asarray(m)
    n, groups = lane_group_rows(cus, 16)
    assert n > cus * 32 * 16
    order = SP.shuffled_tiling(len(A), n, seed=270 + ka, groups=groups)
    sa, sb = GeoSeries(X.column(ka, A).take(order)), GeoSeries(X.column(kb, B).take(order))
    want = {"intersects": (m & 3) != 0, "contains": ((m & 1) != 0) & ((m & 8) == 0), "within": ((m & 1) != 0) & ((m & 4) == 0)}
    for name, w in want.items():
        assert w.any() and not w.all()
        assert_masks(_predicate_on_device(sa, sb, name), w[order].astype(np.uint8), order)
    assert_masks(_predicate_on_device(sa, GeoSeries(X.column(kb, B)), "intersects", rows=order), want["intersects"][order].astype(np.uint8), order)


# ---- point distance: the per-row kernel's tiles, the grouped kernel's chunks, the nearest join --------------------------------------


def _point_distances_on_device(pts_xy, right: GeoSeries, rows=None):
    p = GeoSeries(GeoArrowArray.from_points(pts_xy))
    out = torch.full((len(pts_xy),), -7.0, dtype=torch.float64, device=DEV)
    r = None if rows is None else u32_dev(rows)
    _abi.check(_abi.lib().gpk_distance_rowwise(p.device().handle, right.device().handle, None if r is None else r.data_ptr(), out.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_point_distances(got, pts, kind, rows, rows_of=None):
    for i, p in enumerate(pts):
        d, bound = X.exact_row_distance((float(p[0]), float(p[1])), kind, rows[i if rows_of is None else int(rows_of[i])])
        assert d is not None and X.abs_err(float(got[i]), d) <= bound, (i, got[i], d, bound)


@pytest.mark.parametrize("form", ["b_rows-G8", "rows-G1"])
def test_point_distance_tiles(gpk, cus, form):
    """distance_kernel<G, KIND> takes tiles of DIST_TILE = 2048 points on a grid capped at cus * 16 tiles and keeps the tile's
    ordering lists in LDS from one tile to the next.  With a b_rows map into a small MULTILINESTRING column (a row map is built only
    for LINESTRING targets), and row against row with a MULTIPOINT column tiled like the points."""
    from tests import linref_ref as F

    tile = 2048
    n = SP.second_trip_rows(cus, 16, tile, extra=cus * 2 * tile + 100)
    assert n > cus * 16 * tile
    if form == "b_rows-G8":
        col, pts = F.random_columns()["multilinestrings"]
        kind, rows = F.rows_of(col)
        assert kind == MLS and X.group_size_of(col) == 8
        right = GeoSeries(col)
        small = _point_distances_on_device(pts, right)
        _check_point_distances(small, pts, kind, rows)
        order = SP.shuffled_tiling(len(pts), n, seed=280, groups=cus * 16 * tile)
        assert SP.same_bits(_point_distances_on_device(pts[order], right, rows=order), small[order])
    else:
        rng = np.random.default_rng(281)
        rows = [[tuple(c) for c in rng.uniform(0.0, 1000.0, (1 + i % 3, 2))] for i in range(60)]
        pts = rng.uniform(0.0, 1000.0, (60, 2))
        base = X.column(MP, rows)
        assert X.group_size_of(base) == 1
        small = _point_distances_on_device(pts, GeoSeries(base))
        _check_point_distances(small, pts, MP, rows)
        order = SP.shuffled_tiling(60, n, seed=282, groups=cus * 16 * tile)
        col = base.take(order)
        assert X.group_size_of(col) == 1
        assert SP.same_bits(_point_distances_on_device(pts[order], GeoSeries(col)), small[order])


def test_point_distance_grouped_chunks(gpk, cus):
    """distance_grouped_kernel (a b_rows map into a LINESTRING column with at least 8 points a line): a wave takes chunks of 128 rows
    ordered by line, 512 rows a block, cap cus * 16.  The small run repeats every point 8 times so that it takes the same kernel."""
    from tests import linref_ref as F

    col, pts = F.random_columns()["linestrings"]
    kind, rows = F.rows_of(col)
    assert kind == LS
    right = GeoSeries(col)
    rep8 = np.tile(np.arange(len(pts)), 8)
    assert len(rep8) >= 8 * len(col)
    small8 = _point_distances_on_device(pts[rep8], right, rows=rep8)
    small = small8[: len(pts)]
    assert SP.same_bits(small8, small[rep8])
    _check_point_distances(small, pts, kind, rows)
    n = SP.second_trip_rows(cus, 16, 512)
    assert n > cus * 16 * 512 and n >= 8 * len(col)
    order = SP.shuffled_tiling(len(pts), n, seed=290, groups=cus * 16 * 512)
    assert SP.same_bits(_point_distances_on_device(pts[order], right, rows=order), small[order])


@pytest.mark.parametrize("family,G", [("point", 1), ("linestring", 8)])
def test_nearest_join_rows(gpk, oracle, cus, family, G):
    """nearest_best_kernel / nearest_emit_kernel <G>: 256 / G left points a block, cap cus * 32.  The base join is held against the
    brute-force oracle as test_gpu_nearest does; the tiled join must give every point its base pairs and distances, bit for bit."""
    from geopolars_amd import synth
    from geopolars_amd.spatial_index import nearest_pairs
    from tests.test_gpu_nearest import RIGHTS, _check_against_oracle, _oracle_matrix

    right = RIGHTS[family]()
    assert X.group_size_of(right) == G
    left = synth.uniform_points(400, seed=300 + G)
    sr = GeoSeries(right)
    bp, bc, bd = nearest_pairs(GeoSeries(left), sr)
    _check_against_oracle(_oracle_matrix(oracle, left, right), bp, bc, bd)
    n, groups = lane_group_rows(cus, G)
    assert n > cus * 32 * (256 // G)
    order = SP.shuffled_tiling(len(left), n, seed=301 + G, groups=groups)
    pairs, counts, src = _tiled_pairs(bp, len(left), order)
    got_p, got_c, got_d = nearest_pairs(GeoSeries(GeoArrowArray.from_points(left.xy[order])), sr)
    assert np.array_equal(got_c, counts) and np.array_equal(got_p, pairs) and SP.same_bits(got_d, bd[src])
