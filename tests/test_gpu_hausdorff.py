"""GPU: row-wise discrete Hausdorff and discrete Frechet distance (gpk_hausdorff_distance -> csrc/gpk_hausdorff.hip,
gpk_frechet_distance -> csrc/gpk_frechet.hip) against the exact reference of tests/hausdorff_ref.py.

The shapes are the smallest at which each mechanism can go wrong: sample counts around the lane group, the maximising sample in the
first and the last lane and in the partial round, rows just above and below the large-row thresholds, a walked side that needs a
second LDS chunk, the wavefront's corner, fill, drain and strip boundary, the cap of the boundary column, and lists longer than the
fixed grid of the list kernels."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest
import torch

from geopolars_amd import _abi
from geopolars_amd.geoarrow import DeviceGeoArray
from geopolars_amd.geoseries import GeoSeries
from tests import exact_ref as X
from tests import hausdorff_ref as H
from tests import second_pass as SP

pytestmark = pytest.mark.gpu

PT, MPT, LS, MLS, PG, MPG = H.PT, H.MPT, H.LS, H.MLS, H.PG, H.MPG
KINDS = [PT, MPT, LS, MLS, PG, MPG]
LIST_BLOCKS = 1024  # the fixed grid of hausdorff_large_kernel and frechet_large_kernel


def group_size(a, b) -> int:
    """pairdist_group_size: 32 lanes when the larger mean coordinate count of the two columns is >= 128, else 8"""
    return 32 if max(x.n_coords / x.n_geoms if x.n_geoms else 0.0 for x in (a, b)) >= 128 else 8


def dev(col, separated=False) -> DeviceGeoArray:
    if not separated:
        return GeoSeries(col).device()
    t = lambda v, dt: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).cuda()
    xy = np.ascontiguousarray(col.xy, dtype=np.float64)
    return DeviceGeoArray.from_device_buffers(col.geom_type, (t(xy[:, 0], np.float64), t(xy[:, 1], np.float64)), t(col.geom_offsets, np.int32),
                                              t(col.part_offsets, np.int32), t(col.ring_offsets, np.int32), t(col.validity, np.uint8))


def hausdorff(da, db, n, k=1, rows=None, device_out=True, rc=False):
    lib = _abi.lib()
    if device_out:
        out = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
        r = None if rows is None else torch.from_numpy(np.asarray(rows, dtype=np.int64).astype(np.uint32).view(np.int32)).cuda()
        code = lib.gpk_hausdorff_distance(da.handle, db.handle, None if r is None else r.data_ptr(), k, out.data_ptr(), _abi.MEM_DEVICE, None)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
    else:
        got = np.full(n, -7.0)
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint32)
        code = lib.gpk_hausdorff_distance(da.handle, db.handle, None if r is None else r.ctypes.data, k, got.ctypes.data, _abi.MEM_HOST, None)
    if rc:
        return code
    _abi.check(code)
    return got


def frechet(da, db, n, k=1, rows=None, count=True, rc=False):
    out = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    r = None if rows is None else torch.from_numpy(np.asarray(rows, dtype=np.int64).astype(np.uint32).view(np.int32)).cuda()
    n_over = C.c_int64(-1)
    code = _abi.lib().gpk_frechet_distance(da.handle, db.handle, None if r is None else r.data_ptr(), k, out.data_ptr(), C.byref(n_over) if count else None,
                                           _abi.MEM_DEVICE, None)
    torch.cuda.synchronize()
    if rc:
        return code
    _abi.check(code)
    return out.cpu().numpy(), int(n_over.value)


def with_ballast(kind_rows, G):
    """LINESTRING rows plus one long row that lifts the column's mean coordinate count to the group size wanted (G = 32) — or nothing"""
    rows = list(kind_rows)
    if G == 32:
        rows.append([(float(i), 1000.0 + (i % 3)) for i in range(128 * (len(rows) + 1))])
    return rows


def line(n, x0=0.0, y=0.0, step=1.0):
    return [(x0 + step * i, y) for i in range(n)]


# ---- Hausdorff -----------------------------------------------------------------------------------------------------------------------
KNOWN_H = [  # name of the pair in H.KNOWN, densify, H
    ("postgis_1", None, 14.142135623730951), ("postgis_1", 0.5, 70.0), ("jts_1", None, 22.360679774997898), ("reversed", None, 0.0),
    ("directed", None, 4.123105625617661), ("frechet_doc", None, 50.0),
]


def known(name):
    return next(p for p in H.KNOWN if p[0] == name)


@pytest.mark.parametrize("separated", [False, True])
@pytest.mark.parametrize("device_out", [False, True])
def test_hausdorff_known_answers(gpk, separated, device_out):
    for name, densify, want in KNOWN_H:
        _, ka, ra, kb, rb = known(name)
        a, b = X.column(ka, [ra]), X.column(kb, [rb])
        k = H.densify_k(densify)
        got = hausdorff(dev(a, separated), dev(b, separated), 1, k, device_out=device_out)
        assert got[0] == want, (name, densify, got)
        assert GeoSeries(a).hausdorff_distance(GeoSeries(b), densify=densify)[0] == want
        assert GeoSeries(b).hausdorff_distance(GeoSeries(a), densify=densify)[0] == want


EMPTY = {PT: None, MPT: [], LS: [], MLS: [[]], PG: [], MPG: []}
SPECIAL = {
    MPG: [[[(0, 0), (20, 0), (20, 20), (0, 20), (0, 0)], [(8, 8), (12, 8), (12, 12), (8, 12), (8, 8)]], [[(40, 0), (50, 0), (45, 9), (40, 0)]]],
    MLS: [[(0, 0), (20, 0)], [], [(45, 30)]],
    MPT: [(1, 1), (30, 2)],
}


@pytest.mark.parametrize("ka,kb", list(itertools.combinations_with_replacement(KINDS, 2)))
def test_hausdorff_every_family_pair(gpk, ka, kb):
    """three seeded rows a side, a multipolygon of two parts with a hole, a multi-geometry with an empty member, an empty row, a null row
    and a row map with an entry out of range; both argument orders, bit for bit"""
    rng = random.Random(100 * ka + kb)
    ra = [H.random_row(rng, ka) for _ in range(3)] + [SPECIAL.get(ka, H.random_row(rng, ka)), EMPTY[ka], H.random_row(rng, ka)]
    rb = [H.random_row(rng, kb) for _ in range(3)] + [SPECIAL.get(kb, H.random_row(rng, kb)), H.random_row(rng, kb), H.random_row(rng, kb)]
    va, vb = [1, 1, 1, 1, 1, 1], [1, 1, 0, 1, 1, 1]
    a, b = X.column(ka, ra, va), X.column(kb, rb, vb)
    da, db = dev(a), dev(b)
    for k in (1, 3):
        exact = H.hausdorff_rowwise(ka, ra, kb, rb, k, valid_a=va, valid_b=vb)
        got = hausdorff(da, db, len(ra), k)
        H.check_hausdorff(got, exact, (ka, kb, k))
        assert np.isnan(got[2]) and np.isnan(got[4]) and np.isfinite(got[[0, 1, 3, 5]]).all()
        assert SP.same_bits(hausdorff(db, da, len(ra), k), got) and SP.same_bits(hausdorff(da, db, len(ra), k), got)
    rows = np.array([5, 0, 99, 3, 1, 4], dtype=np.uint32)
    got = hausdorff(da, db, len(ra), 1, rows=rows)
    H.check_hausdorff(got, H.hausdorff_rowwise(ka, ra, kb, rb, 1, b_rows=rows, valid_a=va, valid_b=vb), (ka, kb, "rows"))
    assert np.isnan(got[2])
    assert SP.same_bits(hausdorff(da, db, len(ra), 1, rows=rows, device_out=False), got)


@pytest.mark.parametrize("G", [8, 32])
def test_hausdorff_sample_counts_around_the_group(gpk, G):
    """1, G - 1, G, G + 1 and 2 G + 1 samples on both sides, and the maximising sample in lane 0, in lane G - 1 and in the last, partial
    round, over the interior of the other side's one segment (vertex-to-vertex code fails), in the first direction and — the columns
    exchanged — in the second only"""
    sizes = [1, G - 1, G, G + 1, 2 * G + 1]
    ra, rb = [], []
    for na, nb in itertools.product(sizes, sizes):
        ra.append([(1.5 * i, 0.25 * (i % 3)) for i in range(na)])
        rb.append([(0.5 + 1.25 * i, 3.0 + 0.5 * (i % 2)) for i in range(nb)])
    n = 2 * G + 3
    for spike in (0, G - 1, 2 * G + 1):
        row = line(n)
        row[spike] = (float(spike), 5.0)
        ra.append(row)
        rb.append([(-1.0, 0.0), (float(n), 0.0)])
    ra, rb = with_ballast(ra, G), with_ballast(rb, G)
    a, b = X.column(LS, ra), X.column(LS, rb)
    assert group_size(a, b) == G
    exact = H.hausdorff_rowwise(LS, ra, LS, rb, 1)
    assert [float(h) for h, _ in exact[25:28]] == [5.0, 5.0, 5.0]
    got = hausdorff(dev(a), dev(b), len(ra))
    H.check_hausdorff(got, exact, G)
    assert list(got[25:28]) == [5.0, 5.0, 5.0]
    assert SP.same_bits(hausdorff(dev(b), dev(a), len(ra)), got)


def test_hausdorff_subdivisions(gpk):
    """k = 1, 2, 3, 7: a sample that is not a vertex carries the maximum (the end points of A are the two points of B), 3 and 7 make the
    sample doubles inexact; and seeded line x polygon rows"""
    rng = random.Random(5)
    ra = [[(0.0, 0.0), (20.0, 0.0)]] + [H.random_row(rng, LS) for _ in range(12)]
    a = X.column(LS, ra)
    for kb, first in ((MPT, [(0.0, 0.0), (20.0, 0.0)]), (PG, H.random_row(rng, PG))):
        rb = [first] + [H.random_row(rng, kb) for _ in range(12)]
        b = X.column(kb, rb)
        for k in (1, 2, 3, 7):
            exact = H.hausdorff_rowwise(LS, ra, kb, rb, k)
            got = hausdorff(dev(a), dev(b), len(ra), k)
            H.check_hausdorff(got, exact, (kb, k))
            assert SP.same_bits(hausdorff(dev(b), dev(a), len(ra), k), got)
            if kb == MPT:
                assert got[0] == {1: 0.0, 2: 10.0}.get(k, got[0]) and (k < 3 or 6.0 < got[0] < 9.0)


def wiggle(rng, n, x0=0.0, y0=0.0):
    return [(x0 + i + rng.uniform(-0.3, 0.3), y0 + rng.uniform(-2.0, 2.0)) for i in range(n)]


def test_hausdorff_listed_rows(gpk):
    """260 x 260 coordinates (just above HD_LARGE_COST), 1100 x 70 and 70 x 1100 (the walked side needs a second LDS chunk), 181 x 181
    (just below: the lane-group kernel) and 1100 x 1100 (more than one chunk AND more than one round of 256 samples: the walked side is
    staged again for every round), against the exact reference"""
    rng = random.Random(11)
    ra = [wiggle(rng, 260), wiggle(rng, 1100), wiggle(rng, 181), wiggle(rng, 70, y0=1.0), wiggle(rng, 1100)]
    rb = [wiggle(rng, 260, y0=3.0), wiggle(rng, 70, x0=500.0), wiggle(rng, 181, y0=-2.0), wiggle(rng, 1100, x0=-20.0), wiggle(rng, 1100, x0=7.0, y0=1.5)]
    costs = [H.cost(LS, x, LS, y, 1) for x, y in zip(ra, rb)]
    assert all(costs[i] > H.HD_LARGE_COST for i in (0, 1, 3, 4)) and H.HD_LARGE_COST - 100 < costs[2] <= H.HD_LARGE_COST
    a, b = X.column(LS, ra), X.column(LS, rb)
    exact = H.hausdorff_rowwise(LS, ra, LS, rb, 1)
    got = hausdorff(dev(a), dev(b), 5)
    H.check_hausdorff(got, exact, "listed")
    assert SP.same_bits(hausdorff(dev(b), dev(a), 5), got)
    got2 = hausdorff(dev(a), dev(b), 5, 2)
    H.check_hausdorff(got2, H.hausdorff_rowwise(LS, ra, LS, rb, 2), "listed k = 2")


def test_hausdorff_list_loop_past_its_first_pass(gpk):
    """more listed rows than hausdorff_large_kernel has work-groups: a shuffled tiling of 96 distinct listed rows, every row the bits
    of the base column's answer"""
    rng = random.Random(12)
    ra = [wiggle(rng, 185 + i % 7) for i in range(96)]
    rb = [wiggle(rng, 185 + i % 5, y0=rng.uniform(-3, 3)) for i in range(96)]
    assert all(H.cost(LS, x, LS, y, 1) > H.HD_LARGE_COST for x, y in zip(ra, rb))
    a, b = X.column(LS, ra), X.column(LS, rb)
    base = hausdorff(dev(a), dev(b), 96)
    H.check_hausdorff(base, H.hausdorff_rowwise(LS, ra, LS, rb, 1), "base")
    n = SP.second_trip_rows(LIST_BLOCKS, 1, 1)
    assert n == 1317
    order = SP.shuffled_tiling(96, n, seed=13, groups=LIST_BLOCKS)
    got = hausdorff(dev(a.take(order)), dev(b.take(order)), n)
    assert SP.same_bits(got, base[order])
    assert SP.same_bits(hausdorff(dev(a.take(order)), dev(b), n, rows=order), base[order])


def test_hausdorff_identical_rows_are_zero(gpk):
    rng = random.Random(14)
    for kind in KINDS:
        rows = [H.random_row(rng, kind) for _ in range(5)]
        col = X.column(kind, rows)
        got = hausdorff(dev(col), dev(col), 5)
        assert (got == 0.0).all() and not np.signbit(got).any(), (kind, got)


def test_hausdorff_georeferenced_placements(gpk):
    """the fixture's pairs at the lattice and at the georeferenced placements stay within the same tolerance"""
    z = np.load(H.GOLDEN)
    worst = 0.0
    for off in [(0.0, 0.0)] + list(X.PLACEMENTS):
        pairs = H.load_pairs(z, off)
        for (ka, kb), grp in itertools.groupby(sorted(pairs, key=lambda p: (p[1], p[3])), key=lambda p: (p[1], p[3])):
            grp = list(grp)
            ra, rb = [p[2] for p in grp], [p[4] for p in grp]
            for k in (1, 3):
                got = hausdorff(dev(X.column(ka, ra)), dev(X.column(kb, rb)), len(ra), k)
                worst = max(worst, H.check_hausdorff(got, H.hausdorff_rowwise(ka, ra, kb, rb, k), (off, ka, kb, k)))
    print(f"worst Hausdorff error: {worst:.3g} of the bound")


def test_hausdorff_refusals(gpk):
    col = X.column(LS, [[(0.0, 0.0), (1.0, 0.0)]])
    for k in (0, -1, 4097):
        assert hausdorff(dev(col), dev(col), 1, k, rc=True) == _abi.GPK_ERR_INVALID_ARGUMENT
    two = X.column(LS, [[(0.0, 0.0)], [(1.0, 1.0)]])
    assert hausdorff(dev(col), dev(two), 1, 1, rc=True) == _abi.GPK_ERR_INVALID_ARGUMENT  # row counts differ
    with pytest.raises(ValueError):
        GeoSeries(col).hausdorff_distance(GeoSeries(col), densify=1.5)


# ---- Frechet -------------------------------------------------------------------------------------------------------------------------
def test_frechet_known_answers(gpk):
    for name, densify, want in (("frechet_doc", None, 70.71067811865476), ("frechet_doc", 0.5, 50.0), ("reversed", None, 10.0), ("one_coordinate", None, None)):
        _, _, ra, _, rb = known(name)
        a, b = X.column(LS, [ra]), X.column(LS, [rb])
        k = H.densify_k(densify)
        got, over = frechet(dev(a), dev(b), 1, k)
        assert over == 0
        H.check_frechet(got[0], H.frechet_exact(ra, rb, k), name)
        if want is not None:
            assert got[0] == want, (name, got)
        assert GeoSeries(a).frechet_distance(GeoSeries(b), densify=densify)[0] == got[0]
        assert GeoSeries(b).frechet_distance(GeoSeries(a), densify=densify)[0] == got[0]


@pytest.mark.parametrize("G", [8, 32])
def test_frechet_wavefront_sizes(gpk, G):
    """n' x m' over {1, 2, G - 1, G, G + 1, 2 G + 1}^2: corner, fill and drain of the wavefront and the strip boundary; lattice zigzags
    against the int64 table; a null row, an empty row and a row map"""
    sizes = [1, 2, G - 1, G, G + 1, 2 * G + 1]
    ra, rb = [], []
    for t, (na, nb) in enumerate(itertools.product(sizes, sizes)):
        ra.append(H.zigzag(na, seed=t))
        rb.append(H.zigzag(nb, x0=1, y0=2, amp=4, step=3, seed=100 + t))
    ra += [H.zigzag(5), []]
    rb += [H.zigzag(4), H.zigzag(3)]
    valid = [1] * 36 + [0, 1]
    ra, rb = with_ballast(ra, G), with_ballast(rb, G)
    valid += [1] * (len(ra) - len(valid))
    a, b = X.column(LS, ra, valid), X.column(LS, rb)
    assert group_size(a, b) == G
    got, over = frechet(dev(a), dev(b), len(ra))
    assert over == 0 and np.isnan(got[36]) and np.isnan(got[37])
    want = [H.frechet_exact(x, y, 1, lattice=True) for x, y in zip(ra[:36], rb[:36])]
    for i in range(36):
        H.check_frechet(got[i], want[i], (G, i))
    back, _ = frechet(dev(b), dev(a), len(ra), rows=np.arange(len(ra)))
    assert SP.same_bits(back[:36], got[:36])
    rows = np.array([(7 * i) % 36 for i in range(len(ra))])
    rows[3] = 1000  # out of range
    mapped, _ = frechet(dev(a), dev(b), len(ra), rows=rows)
    assert np.isnan(mapped[3])
    for i in (0, 5, 17, 35):
        H.check_frechet(mapped[i], H.frechet_exact(ra[i], rb[rows[i]], 1, lattice=True), (G, "rows", i))


# hand-made 3 x 3 tables in which exactly one predecessor of an inner cell decides the answer
PREDECESSORS = {
    "up": ([(6, 2), (8, 1), (9, 4)], [(8, 2), (1, 9), (9, 3)], 74),
    "left": ([(7, 6), (0, 1), (8, 9)], [(5, 5), (5, 9), (7, 9)], 41),
    "diag": ([(9, 6), (2, 4), (5, 9)], [(5, 7), (1, 1), (7, 7)], 17),
}


@pytest.mark.parametrize("G", [8, 32])
def test_frechet_each_predecessor_decides(gpk, G):
    """the three cases alone and behind m copies of their first points (which leave the value unchanged), so that the deciding cells sit
    in the last lane of the first strip and in the first lane of the second"""
    ra, rb, want = [], [], []
    for p, q, c in PREDECESSORS.values():
        for m in (0, G - 2, G - 1, G):
            for x, y in ((p, q), (q, p)):
                ra.append([x[0]] * m + list(x))
                rb.append([y[0]] * m + list(y))
                want.append(c)
    assert [H.frechet_exact(x, y, 1, lattice=True) for x, y in zip(ra, rb)] == want
    ra, rb = with_ballast(ra, G), with_ballast(rb, G)
    a, b = X.column(LS, ra), X.column(LS, rb)
    assert group_size(a, b) == G
    got, _ = frechet(dev(a), dev(b), len(ra))
    assert list(got[: len(want)]) == [float(np.sqrt(c)) for c in want]


def test_frechet_subdivisions(gpk):
    rng = random.Random(21)
    ra = [wiggle(rng, rng.randint(1, 14)) for _ in range(24)]
    rb = [wiggle(rng, rng.randint(1, 14), y0=1.0) for _ in range(24)]
    a, b = X.column(LS, ra), X.column(LS, rb)
    for k in (1, 2, 3):
        got, over = frechet(dev(a), dev(b), 24, k)
        assert over == 0
        for i in range(24):
            H.check_frechet(got[i], H.frechet_exact(ra[i], rb[i], k), (k, i))
        back, _ = frechet(dev(b), dev(a), 24, k)
        assert SP.same_bits(back, got)
        again, _ = frechet(dev(a), dev(b), 24, k, count=False)
        assert SP.same_bits(again, got)


def test_frechet_listed_rows_and_the_cap(gpk):
    """300 x 300, 70 x 3000, a 700 x 3000 lattice row, a row whose shorter side has exactly GPK_FRECHET_MAX_SHORT samples (closed form:
    1.25) and one a sample over the cap (NaN, counted)"""
    rng = random.Random(22)
    cap = H.FRECHET_MAX_SHORT
    ra = [wiggle(rng, 300), wiggle(rng, 70), H.zigzag(700, amp=9, seed=1), [(float(i), 0.0) for i in range(cap)], [(float(i), 0.0) for i in range(cap + 1)]]
    rb = [wiggle(rng, 300, y0=2.0), wiggle(rng, 3000, x0=-10.0), H.zigzag(3000, y0=4, amp=7, step=1, seed=2), [(float(i), 0.75) for i in range(cap + 1)],
          [(float(i), 0.75) for i in range(cap + 2)]]
    a, b = X.column(LS, ra), X.column(LS, rb)
    got, over = frechet(dev(a), dev(b), 5)
    assert over == 1 and np.isnan(got[4])
    assert got[3] == 1.25
    H.check_frechet(got[0], H.frechet_exact(ra[0], rb[0]), "300 x 300")
    H.check_frechet(got[1], H.frechet_exact(ra[1], rb[1]), "70 x 3000")
    H.check_frechet(got[2], H.frechet_exact(ra[2], rb[2], lattice=True), "700 x 3000")
    # the other order and the Python layer, without the row at the cap (its table alone is most of this test's time)
    keep = [0, 1, 2, 4]
    a4, b4 = a.take(keep), b.take(keep)
    back, over = frechet(dev(b4), dev(a4), 4)
    assert over == 1 and SP.same_bits(back, got[keep])
    with pytest.raises(ValueError, match=f"1 of 4 rows.*{cap}"):
        GeoSeries(a4).frechet_distance(GeoSeries(b4))
    lenient = GeoSeries(a4).frechet_distance(GeoSeries(b4), errors="nan")
    assert SP.same_bits(lenient, got[keep])
    # k = 2 on a shorter closed-form row: the samples of A = (i / 2, 0), of B = (i / 2, 0.75): the last step of B alone is 0.5 long
    k2, _ = frechet(dev(X.column(LS, [ra[3][:200]])), dev(X.column(LS, [rb[3][:201]])), 1, 2)
    H.check_frechet(k2[0], H.frechet_exact(ra[3][:200], rb[3][:201], 2), "k = 2")


def test_frechet_list_loop_past_its_first_pass(gpk):
    rng = random.Random(23)
    ra = [H.zigzag(129 + i % 9, amp=5, seed=i) for i in range(96)]
    rb = [H.zigzag(131 + i % 4, y0=rng.randint(-3, 3), amp=6, seed=200 + i) for i in range(96)]
    assert all(len(x) * len(y) > H.FR_LARGE_COST for x, y in zip(ra, rb))
    a, b = X.column(LS, ra), X.column(LS, rb)
    base, _ = frechet(dev(a), dev(b), 96)
    for i in range(96):
        H.check_frechet(base[i], H.frechet_exact(ra[i], rb[i], 1, lattice=True), i)
    n = SP.second_trip_rows(LIST_BLOCKS, 1, 1)
    order = SP.shuffled_tiling(96, n, seed=24, groups=LIST_BLOCKS)
    got, over = frechet(dev(a.take(order)), dev(b.take(order)), n)
    assert over == 0 and SP.same_bits(got, base[order])


def test_frechet_refusals(gpk):
    ls = X.column(LS, [[(0.0, 0.0), (1.0, 0.0)]])
    for kind, row in ((MPT, [(0.0, 0.0)]), (MLS, [[(0.0, 0.0), (1.0, 1.0)]]), (PG, [[(0, 0), (1, 0), (1, 1), (0, 0)]]), (PT, (0.0, 0.0))):
        other = X.column(kind, [row])
        assert frechet(dev(ls), dev(other), 1, rc=True) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
        assert frechet(dev(other), dev(ls), 1, rc=True) == _abi.GPK_ERR_MISMATCHED_GEOMETRY
        with pytest.raises(_abi.MismatchedGeometry):
            GeoSeries(ls).frechet_distance(GeoSeries(other))
    for k in (0, 4097):
        assert frechet(dev(ls), dev(ls), 1, k, rc=True) == _abi.GPK_ERR_INVALID_ARGUMENT


def test_frechet_is_at_least_hausdorff(gpk):
    rng = np.random.default_rng(25)
    n = 2000
    counts = rng.integers(2, 20, size=(2, n))
    cols = []
    for side in range(2):
        rows = []
        for i in range(n):
            steps = rng.normal(0.0, 1.0, size=(counts[side, i], 2)).cumsum(axis=0) + rng.uniform(0, 5, size=2)
            rows.append([tuple(p) for p in steps])
        cols.append(X.column(LS, rows))
    da, db = dev(cols[0]), dev(cols[1])
    for k in (1, 3):
        f, over = frechet(da, db, n, k)
        h = hausdorff(da, db, n, k)
        assert over == 0 and np.isfinite(f).all() and np.isfinite(h).all()
        assert (f >= h * (1 - 1e-12)).all()
