"""GPU: the k-nearest-neighbours join (gpk_knn_join / knn_pairs / knn_pairs_device / spatial_join_knn).

  1. against the library's own distance, bit for bit, all 36 ordered pairs of families and every refine instance: the matrix D[l, r] of
     gpk_distance_rowwise's per-row kernels (tests/test_gpu_dwithin.distance_matrix), the expected result a stable sort of (D, r) per
     left row (tests/knn_ref.expected_from_matrix), at k = 1, 3 and 8, without a bound and within the matrix's median entry;
  2. against the exact reference at k = 2, 3 and 5 on the rows tests/test_knn_host.py counts as decided;
  3. k = 1 against gpk_nearest_join_any: its lowest right row per left row, the same distance bits;
  4. ties on an integer lattice, GPK_KNN_EXCLUDE_SELF, left_row_base, each selection class at its thresholds and past the first pass of
     the list kernel's fixed grid, right rows listed in many cells, grid cases, the never-matched rules, arguments and buffers,
     determinism, the table join, and the bytes of two joins that share the emit hook."""
import ctypes as C
import os
import re

import numpy as np
import pyarrow as pa
import pytest
import torch

from geopolars_amd import _abi
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import (
    SpatialIndex,
    SpatialJoinKnnArgs,
    dwithin_pairs,
    join_indices,
    knn_pairs,
    knn_pairs_device,
    nearest_pairs_any,
    spatial_join_knn,
    take_column,
)
from tests import dwithin_ref as W
from tests import knn_ref as K
from tests import nearest_any_ref as N
from tests import second_pass as SP
from tests.test_gpu_dwithin import distance_matrix, expected as dwithin_expected, series

pytestmark = pytest.mark.gpu

PT, MP, LS, MLS, PG, MPG = W.PT, W.MP, W.LS, W.MLS, W.PG, W.MPG
INF = float("inf")
KNN_SRC = os.path.join(SP.CSRC, "gpk_knn.hip")


def _constant(name):
    m = re.search(rf"constexpr \w+ {name} = (\d+);", open(KNN_SRC).read())
    assert m, name
    return int(m.group(1))


LIST_BLOCKS, LDS_KEYS = _constant("KNN_LIST_BLOCKS"), _constant("KNN_LDS_KEYS")


def _sq(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]


def squares(boxes, valid=None):
    return (PG, [[_sq(*map(float, b))] for b in boxes], valid)


def median_entry(D):
    d = D[~np.isnan(D)]
    assert len(d) > 2
    return float(np.quantile(d, 0.5, method="lower"))


def same(got, want, what=None):
    (gp, gc, gd), (wp, wc, wd) = got, want
    assert np.array_equal(gc, wc), (what, np.nonzero(gc != wc)[0][:8], gc[:8], wc[:8])
    assert np.array_equal(gp, wp), (what, len(gp), len(wp), np.nonzero((gp != wp).any(axis=1))[0][:8])
    assert SP.same_bits(gd, wd), what


def check_against_matrix(left, right, ks, bounds=None, D=None, sl=None, sr=None, exclude_self=False):
    """knn_pairs == the first k of the sorted rows of the library's own distance matrix, with and without a prebuilt index; returns D"""
    sl, sr = sl or series(left), sr or series(right)
    D = distance_matrix(left, right, sl, sr) if D is None else D
    idx = SpatialIndex(sr, for_points=False)
    for md in bounds if bounds is not None else (INF, median_entry(D)):
        for k in ks:
            want = K.expected_from_matrix(D, k, md, exclude_self)
            assert (want[1] <= k).all()
            same(knn_pairs(sl, sr, k, max_distance=md, exclude_self=exclude_self), want, (k, md))
            same(knn_pairs(sl, sr, k, r_index=idx, max_distance=md, exclude_self=exclude_self), want, (k, md, "index"))
    idx.free()
    return D


def rows_matrix(left, right, sr=None):
    """D[l, r] for a handful of left rows against a long right column: one row-wise call per left row (its row repeated, right row j for
    element j — one left row per target, so the per-row kernels run and not the grouped schedule)"""
    sr = sr or series(right)
    nr = len(right[1])
    rows = np.arange(nr, dtype=np.uint32)
    D = np.stack([series((left[0], [row] * nr, None)).distance(sr, other_rows=rows) for row in left[1]])
    assert not np.isnan(D).any()
    return D


def candidates_of(call):
    """the candidates one call lists (the join statistics, as tools/bench_nearest_any.py reads them)"""
    lib = _abi.lib()
    st = (C.c_int64 * 4)()
    lib.gpk_join_stats_enable(1)
    lib.gpk_join_stats(st, 1)
    out = call()
    lib.gpk_join_stats(st, 1)
    lib.gpk_join_stats_enable(0)
    return out, int(st[2])


# ---- 1 + 2 + 3: every ordered pair of families, every refine instance ---------------------------------------------------------------


def check_fixture(key, seed, left, right):
    sl, sr = series(left), series(right)
    D = check_against_matrix(left, right, (1, 3, 8), sl=sl, sr=sr)
    # k = 1 is the lowest right row of the nearest join's tie set, with its distance
    p1, c1, d1 = knn_pairs(sl, sr, 1)
    pn, cn, dn = nearest_pairs_any(sl, sr)
    first = (np.cumsum(cn.astype(np.int64)) - cn)[cn > 0]
    assert np.array_equal(c1, np.minimum(cn, 1)) and np.array_equal(p1, pn[first]) and SP.same_bits(d1, dn[first])
    # the exact k nearest sets on the decided rows
    table = N.fixture_table(key, seed)
    for k in (2, 3, 5):
        exact = K.exact_knn(table, k)
        pairs, counts, _ = knn_pairs(sl, sr, k)
        off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        assert set(np.nonzero(counts)[0].tolist()) == set(exact)
        for l, (want, decided) in exact.items():
            got = pairs[off[l]:off[l + 1], 1].tolist()
            assert len(got) == len(want) == len(set(got)), (key, k, l)
            if decided:
                assert set(got) == want, (key, k, l, got, sorted(want))
    return D


@pytest.mark.parametrize("key", W.POINT_FIXTURES, ids=lambda k: f"{k[0]}-G{k[1]}-{'pl' if k[2] else 'pr'}")
def test_point_side_against_own_distance_and_exact_reference(gpk, key):
    check_fixture(key, None, *W.point_fixture(*key))


@pytest.mark.parametrize("key", W.PAIR_INSTANCES, ids=lambda k: f"{k[0]}x{k[1]}-{k[2]}")
def test_non_point_pairs_against_own_distance_and_exact_reference(gpk, key):
    left, right = W.pair_fixture(*key)
    D = check_fixture(key, 0, left, right)
    if key[2] != "g8":
        assert (~np.isnan(D)).sum(axis=1).max() < 8  # (k = 8 is the "fewer than k" path on every row)


# ---- 4: ties on an integer lattice ----------------------------------------------------------------------------------------------------


def lattice(n):
    return (PT, [(float(x), float(y)) for y in range(n) for x in range(n)], None)


def test_ties_on_an_integer_lattice(gpk):
    right = lattice(9)
    left = (PT, [(4.0, 4.0)], None)
    sl, sr = series(left), series(right)
    D = distance_matrix(left, right, sl, sr)
    rings = [40, 31, 39, 41, 49, 30, 32, 48, 50, 22, 38, 42, 58]  # the centre, the axis ring, the diagonal ring, the ring at 2: r ascending
    dists = [0.0] + [1.0] * 4 + [2.0 ** 0.5] * 4 + [2.0] * 4
    for k in (3, 5, 7, 9, 13):  # (3 and 7 cut inside a tie ring)
        p, c, d = knn_pairs(sl, sr, k)
        assert p[:, 1].tolist() == rings[:k] and d.tolist() == dists[:k] and c.tolist() == [k] and (p[:, 0] == 0).all()
    check_against_matrix(left, right, (5, 9, 13, 64), D=D, sl=sl, sr=sr, bounds=(INF, 2.0 ** 0.5, 0.0))


def test_exclude_self_on_a_column_against_itself(gpk):
    col = lattice(9)
    s = series(col)
    D = distance_matrix(col, col, s, s)
    p, c, d = knn_pairs(s, s, 4, exclude_self=True)
    assert (p[:, 0] != p[:, 1]).all() and (c == 4).all()
    for y in range(1, 8):
        for x in range(1, 8):
            i = 9 * y + x
            assert p[p[:, 0] == i, 1].tolist() == [i - 9, i - 1, i + 1, i + 9] and (d[p[:, 0] == i] == 1.0).all()
    check_against_matrix(col, col, (1, 4, 64), D=D, sl=s, sr=s, exclude_self=True, bounds=(INF, 1.0))
    # without the flag every row is its own nearest neighbour
    p, c, d = knn_pairs(s, s, 1)
    assert (p[:, 0] == p[:, 1]).all() and (d == 0.0).all()
    # a shard of the column against the whole of it: the self pair is r == l + left_row_base
    lo, hi = 27, 54
    shard = series((PT, col[1][lo:hi], None))
    for k in (4, 64):
        want = K.expected_from_matrix(D[lo:hi], k, INF, True, lo)
        assert (want[0][:, 0] >= lo).all() and (want[0][:, 0] != want[0][:, 1]).all()
        same(knn_pairs(shard, s, k, exclude_self=True, left_row_base=lo), want, k)
    same(knn_pairs(shard, s, 4, left_row_base=lo), K.expected_from_matrix(D[lo:hi], 4, INF, False, lo))


# ---- each selection class --------------------------------------------------------------------------------------------------------------
# A fan: N horizontal segments from x = -100 to x = 100 at heights 1, 1, 1 + 1/32, 1 + 1/32, ... (every height twice: ties between
# different right rows).  The far distance from a left point near the middle to any of them is at least 100, more than every true
# distance, so every segment is a candidate of every left point and is eligible: a left row has exactly N candidates.


def fan(n):
    return (LS, [[(-100.0, 1.0 + (j // 2) / 32.0), (100.0, 1.0 + (j // 2) / 32.0)] for j in range(n)], None)


FAN_LEFT = (PT, [(0.0, 0.0), (3.5, 20.25), (-41.0, 7.015625), (12.0, 1.0), (-7.25, 33.0), (60.0, 2.53125), (1.0, 64.5)], None)


@pytest.mark.parametrize("n", [64, 65, LDS_KEYS, LDS_KEYS + 1, 3 * LDS_KEYS // 2 + 3], ids=lambda n: f"{n}-candidates")
def test_selection_classes_at_their_thresholds(gpk, n):
    """64: the wave kernel's last size; 65: the list's first; KNN_LDS_KEYS: the last row ranked from LDS; above: the radix select"""
    right = fan(n)
    assert 1.0 + (n // 2) / 32.0 < 100.0  # (the heights stay below the far distances)
    sl, sr = series(FAN_LEFT), series(right)
    D = rows_matrix(FAN_LEFT, right, sr)
    assert len(np.unique(D[0])) < n  # ties
    idx = SpatialIndex(sr, for_points=False)
    for k in (1, 7, 64):
        got, cand = candidates_of(lambda: knn_pairs(sl, sr, k, r_index=idx))
        assert cand == n * len(FAN_LEFT[1])  # every left row has exactly n candidates
        same(got, K.expected_from_matrix(D, k), k)
    md = median_entry(D)
    same(knn_pairs(sl, sr, 64, r_index=idx, max_distance=md), K.expected_from_matrix(D, 64, md), "bounded")
    same(knn_pairs(sl, sr, 64, r_index=idx, max_distance=0.0), K.expected_from_matrix(D, 64, 0.0), "zero")
    idx.free()


@pytest.mark.parametrize("n,k", [(70, 5), (LDS_KEYS + 9, 64)], ids=["lds-keys", "radix-select"])
def test_list_kernel_past_its_first_pass(gpk, n, k):
    """more listed rows than the list kernel's fixed grid has work-groups: every work-group takes a second row, of another left point"""
    right = fan(n)
    sr = series(right)
    D = rows_matrix(FAN_LEFT, right, sr)
    n_rows = LIST_BLOCKS + LIST_BLOCKS // 4 + 37
    order = SP.rotating_tiling(len(FAN_LEFT[1]), n_rows, LIST_BLOCKS)
    left = (PT, [FAN_LEFT[1][i] for i in order], None)
    got, cand = candidates_of(lambda: knn_pairs(series(left), sr, k))
    assert cand == n * n_rows
    same(got, K.expected_from_matrix(D[order], k), (n, k))


def test_wave_kernel_over_many_rows(gpk):
    """the one-wave kernel takes a row per wave on a grid sized from the rows, so it has no stride to get past: 5000 rows of a few to
    some 80 candidates (at k = 60 the square around the 60th neighbour holds about 77 right points: those rows go to the list)"""
    rng = np.random.default_rng(11)
    right = (PT, [tuple(p) for p in rng.integers(0, 64, (700, 2)).astype(np.float64)], None)  # (a lattice with repeats: ties)
    base = (PT, [tuple(p) for p in rng.integers(-8, 72, (40, 2)).astype(np.float64) + 0.5], None)
    sr = series(right)
    D = rows_matrix(base, right, sr)
    order = SP.shuffled_tiling(len(base[1]), 5000, 3, 4)
    left = series((PT, [base[1][i] for i in order], None))
    for k in (1, 6, 33, 60):
        same(knn_pairs(left, sr, k), K.expected_from_matrix(D[order], k), k)


# ---- right rows listed in many cells -------------------------------------------------------------------------------------------------


def test_right_rows_listed_in_many_cells(gpk):
    rng = np.random.default_rng(7)
    long_ones = [[(0.0 + o, 0.0), (100.0, 100.0 - o)] for o in rng.integers(0, 40, 40).astype(np.float64)]
    short = [[(float(x), float(y)), (float(x) + 1.0, float(y) + 0.5)] for x, y in rng.integers(0, 99, (200, 2))]
    right = (LS, long_ones + short, None)
    left = (PT, [tuple(p) for p in rng.integers(0, 100, (24, 2)).astype(np.float64)], None)
    sr = series(right)
    D = rows_matrix(left, right, sr)
    sl = series(left)
    for k in (4, 48):
        p, c, d = knn_pairs(sl, sr, k)
        same((p, c, d), K.expected_from_matrix(D, k), k)
        assert all(len(set(p[p[:, 0] == l, 1].tolist())) == k for l in range(24))  # no right row twice


# ---- grid cases ------------------------------------------------------------------------------------------------------------------------


def test_grid_cases(gpk):
    rng = np.random.default_rng(5)
    left = squares([(x, y, x + 1, y + 2) for x, y in rng.uniform(-40, 40, (40, 2))])
    ks = (1, 4, 12)
    # a single right row; every right row at one coordinate (both axes of the directory have zero extent); one vertical line
    check_against_matrix(squares([(x, y, x + 1, y + 1) for x, y in rng.uniform(-50, 50, (6, 2))]), squares([(0, 0, 2, 2)]), ks, bounds=(INF, 30.0))
    check_against_matrix(left, (PT, [(3.0, 8.0)] * 9, None), ks)
    check_against_matrix(left, (LS, [[(3.0, float(y)), (3.0, float(y) + 0.5)] for y in rng.uniform(0, 50, 30)], None), ks)
    # left rows far outside the extent on each side and corner, and one covering all of it
    small = squares([(x, y, x + 0.5, y + 0.5) for x, y in rng.uniform(0, 100, (60, 2))])
    far = [(-1e6, 50), (1e6, 50), (50, -1e6), (50, 1e6), (-300, -300), (400, 400), (-250, 350), (320, -120), (-1, 50), (101, 50)]
    outside = squares([(x, y, x + 3, y + 3) for x, y in far] + [(-10, -10, 120, 120), (0, 0, 100.5, 100.5)])
    check_against_matrix(outside, small, ks)
    check_against_matrix((LS, [[(x, y), (x + 3.0, y + 1.0)] for x, y in far], None), small, ks)


# ---- arguments and buffers ---------------------------------------------------------------------------------------------------------------


def test_max_distance_is_closed(gpk):
    right = lattice(9)
    sl, sr = series((PT, [(4.0, 4.0)], None)), series(right)
    D = distance_matrix((PT, [(4.0, 4.0)], None), right, sl, sr)
    for d in np.unique(D)[[1, 4, 9]].tolist():  # exact lattice distances: whole rings of right rows lie at them
        n = int((D <= d).sum())
        below, above = float(np.nextafter(d, 0.0)), float(np.nextafter(d, INF))
        assert knn_pairs(sl, sr, 64, max_distance=d)[1].tolist() == [min(n, 64)]
        assert knn_pairs(sl, sr, 64, max_distance=above)[1].tolist() == [min(n, 64)]
        assert knn_pairs(sl, sr, 64, max_distance=below)[1].tolist() == [min(int((D < d).sum()), 64)] and int((D < d).sum()) < n
    sq = series(squares([(0, 0, 1, 1)]))
    two = series(squares([(3, 0, 4, 1), (10, 0, 11, 1)]))
    p, c, d = knn_pairs(sq, two, 2, max_distance=2.0)
    assert p.tolist() == [[0, 0]] and d.tolist() == [2.0]
    assert len(knn_pairs(sq, two, 2, max_distance=float(np.nextafter(2.0, 0.0)))[0]) == 0
    p, c, d = knn_pairs(sq, two, 2, max_distance=9.0)
    assert p.tolist() == [[0, 0], [0, 1]] and d.tolist() == [2.0, 9.0]


def test_null_empty_and_nan_rows(gpk):
    nan = float("nan")
    left = (MP, [[(0.0, 0.0)], [], [(5.0, 5.0), (6.0, 6.0)], [(1.0, 1.0)], [(9.0, 9.0)]], [True, True, True, False, True])
    right = (PT, [(0.0, 1.0), (nan, 2.0), (5.0, 4.0), (3.0, nan), (5.0, 4.0), (100.0, 100.0)], [True, True, True, True, True, False])
    check_against_matrix(left, right, (1, 2, 5), bounds=(INF, 1.0, 0.0))
    p, c, d = knn_pairs(series(left), series(right), 2)
    assert p.tolist() == [[0, 0], [0, 2], [2, 2], [2, 4], [4, 2], [4, 4]] and c.tolist() == [2, 0, 2, 0, 2]
    check_against_matrix(right, left, (1, 2, 5), bounds=(INF, 1.0, 0.0))
    assert knn_pairs(series(right), series(left), 5)[1].tolist() == [3, 0, 3, 0, 3, 0]
    lp = (PG, [[_sq(0.0, 0.0, 1.0, 1.0)], [], [_sq(5.0, 5.0, 6.0, 6.0)]], [True, True, False])
    rl = (MLS, [[[(3.0, 0.0), (3.0, 1.0)]], [], [[(0.5, 0.5), (0.6, 0.6)]], [[(2.0, 0.0), (2.0, 1.0)]]], [True, True, False, True])
    check_against_matrix(lp, rl, (1, 3), bounds=(INF, 1.5))
    p, c, d = knn_pairs(series(lp), series(rl), 3)
    assert p.tolist() == [[0, 3], [0, 0]] and d.tolist() == [1.0, 2.0] and c.tolist() == [2, 0, 0]
    # an all-empty right side, and empty columns on either side
    p, c, d = knn_pairs(series(lp), series((LS, [[], []], None)), 3)
    assert len(p) == 0 and len(d) == 0 and c.tolist() == [0, 0, 0]
    none = (LS, [], None)
    p, c, d = knn_pairs(series(lp), series(none), 3)
    assert len(p) == 0 and c.tolist() == [0, 0, 0]
    p, c, d = knn_pairs(series(none), series(lp), 3)
    assert len(p) == 0 and len(c) == 0 and len(d) == 0


def test_arguments_capacity_and_device_buffers(gpk):
    lib = _abi.lib()
    left, right = W.pair_fixture(LS, PG, "g8")
    sl, sr = series(left), series(right)
    D = distance_matrix(left, right, sl, sr)
    md, k = median_entry(D), 3
    p0, c0, d0 = K.expected_from_matrix(D, k, md)
    assert len(p0) > 2 and (c0 == 0).any() and (c0 == k).any()
    call = lambda kk, m, flags, *a: lib.gpk_knn_join(sl.device().handle, sr.device().handle, None, kk, m, flags, *a)  # noqa: E731
    n = C.c_int64(-1)
    counts = np.full(len(c0), 77, np.uint32)
    assert call(k, md, 0, 0, counts.ctypes.data, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_OK  # count-only
    assert n.value == len(p0) and np.array_equal(counts, c0)
    small = np.zeros((len(p0) - 1, 2), np.uint32)
    n.value = -1
    assert call(k, md, 0, 0, None, small.ctypes.data, None, len(small), C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_CAPACITY
    assert n.value == len(p0) and np.array_equal(small, p0[:-1])
    for bad_k, bad_md, bad_flags in ((0, md, 0), (-1, md, 0), (65, md, 0), (k, -1.0, 0), (k, float("nan"), 0), (k, -INF, 0), (k, md, 2), (k, md, 0x80000001)):
        n.value = -1
        assert call(bad_k, bad_md, bad_flags, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT and n.value == 0
    assert call(k, md, 0, 0, None, None, None, 4, C.byref(n), _abi.MEM_HOST, None) == _abi.GPK_ERR_INVALID_ARGUMENT  # capacity without pairs
    wrong = SpatialIndex(sl, for_points=False)  # an index of another column
    assert lib.gpk_knn_join(sl.device().handle, sr.device().handle, wrong.handle, k, md, 0, 0, None, None, None, 0, C.byref(n), _abi.MEM_HOST,
                            None) == _abi.GPK_ERR_INVALID_ARGUMENT
    wrong.free()
    # device buffers == host buffers, with left_row_base, with and without distances
    idx = SpatialIndex(sr, for_points=False)
    dc = torch.full((len(c0),), -1, dtype=torch.int32, device="cuda:0")
    assert knn_pairs_device(sl.device(), sr.device(), None, k, dc, None, max_distance=md) == len(p0)
    torch.cuda.synchronize()
    assert np.array_equal(dc.cpu().numpy().astype(np.uint32), c0)
    based = p0 + np.array([1000, 0], dtype=np.uint32)
    dp = torch.zeros((len(c0) * k, 2), dtype=torch.int32, device="cuda:0")
    dd = torch.full((len(c0) * k,), -1.0, dtype=torch.float64, device="cuda:0")
    assert knn_pairs_device(sl.device(), sr.device(), idx, k, dc, dp, dd, max_distance=md, left_row_base=1000) == len(p0)
    torch.cuda.synchronize()
    assert np.array_equal(dp.cpu().numpy().astype(np.uint32)[: len(p0)], based)
    assert SP.same_bits(dd.cpu().numpy()[: len(p0)], d0) and (dd.cpu().numpy()[len(p0):] == -1.0).all()
    dp.zero_()
    assert knn_pairs_device(sl.device(), sr.device(), idx, k, None, dp, None, max_distance=md, left_row_base=1000) == len(p0)  # out_dist=None
    torch.cuda.synchronize()
    assert np.array_equal(dp.cpu().numpy().astype(np.uint32)[: len(p0)], based)
    same(knn_pairs(sl, sr, k, r_index=idx, max_distance=md, left_row_base=1000), (based, c0, d0))
    idx.free()


def test_two_calls_give_identical_bytes(gpk):
    for key in ((MLS, MPG, "g8"), (PG, LS, "g32"), (MPG, MLS, "large")):
        left, right = W.pair_fixture(*key)
        sl, sr = series(left), series(right)
        a, b = knn_pairs(sl, sr, 3), knn_pairs(sl, sr, 3)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a[0]) > 0
    right = fan(LDS_KEYS + 40)
    sl, sr = series(FAN_LEFT), series(right)
    a, b = knn_pairs(sl, sr, 64), knn_pairs(sl, sr, 64)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a[0]) == 64 * len(FAN_LEFT[1])


# ---- table level -----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", [PG, LS], ids=["polygons", "lines"])
@pytest.mark.parametrize("how", ["inner", "left"])
def test_spatial_join_knn_over_tables(gpk, how, kind):
    left, right = W.pair_fixture(PG, kind, "g8")
    la, ra = W.columns(left, right)
    lt = pa.table({"id": pa.array(np.arange(len(la))), "geometry": la.to_arrow_wkb()})
    rt = pa.table({"name": pa.array([f"r{i}" for i in range(len(ra))]), "geometry": ra.to_arrow_wkb()})
    lgeo, rgeo = GeoSeries.from_arrow(lt.column("geometry")), GeoSeries.from_arrow(rt.column("geometry"))
    k = 3
    base = knn_pairs(lgeo, rgeo, k)
    md = float(np.quantile(base[2], 0.5, method="lower"))
    pairs, counts, dist = knn_pairs(lgeo, rgeo, k, max_distance=md)
    assert 0 < len(pairs) < len(base[0]) and 0 < np.count_nonzero(counts == 0) < len(la)
    li, ri = join_indices(counts, pairs, how)
    t = spatial_join_knn(lt, rt, SpatialJoinKnnArgs(k=k, join_type=how, max_distance=md, distance_col="dist", rank_col="rank"))
    assert t.column_names == ["id_left", "geometry_left", "name_right", "geometry_right", "dist", "rank"] and t.num_rows == len(li)
    assert t.column("id_left").combine_chunks().equals(take_column(lt.column("id"), li))
    assert t.column("name_right").combine_chunks().equals(take_column(rt.column("name"), ri))
    # the joined rows keep the pairs' order: nearest first within a left row
    assert np.array_equal(li[ri >= 0], pairs[:, 0].astype(np.int64)) and np.array_equal(ri[ri >= 0], pairs[:, 1].astype(np.int64))
    d, rank = t.column("dist").combine_chunks(), t.column("rank").combine_chunks()
    assert rank.type == pa.uint32()
    assert d.null_count == rank.null_count == np.count_nonzero(ri < 0) and (how == "inner") == (d.null_count == 0)
    assert SP.same_bits(np.asarray(d.drop_null()), dist)
    want_rank = np.concatenate([np.arange(c) for c in counts]).astype(np.uint32)
    assert np.array_equal(np.asarray(rank.drop_null()), want_rank) and want_rank.max() >= 1
    t = spatial_join_knn(lt, rt, SpatialJoinKnnArgs(k=k, join_type=how))
    assert t.column_names == ["id_left", "geometry_left", "name_right", "geometry_right"]
    assert t.num_rows == int(base[1].sum()) + (np.count_nonzero(base[1] == 0) if how == "left" else 0)


# ---- the joins that share the emit hook return what they returned --------------------------------------------------------------------


def test_existing_payload_joins_keep_their_bytes(gpk):
    left, right = W.pair_fixture(LS, PG, "g8")
    sl, sr = series(left), series(right)
    D = distance_matrix(left, right, sl, sr)
    md = median_entry(D)
    for bound in (INF, md):
        same(nearest_pairs_any(sl, sr, max_distance=bound), N.expected_from_matrix(D, bound), bound)
    want = dwithin_expected(D, md)
    assert len(want[0]) > 4
    same(dwithin_pairs(sl, sr, md), want, "dwithin")
