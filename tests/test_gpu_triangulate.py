"""GPU: gpk_triangulate (csrc/gpk_triangulate.hip) held to the exact checker of tests/triangulate_ref.py.  A triangulation is not
unique, so nothing is compared with a stored answer: every valid row (gpk_validity's code 0, known exactly from tests/validity_ref.py)
must have status 0 and pass (a) - (e); the indices must be identical wherever the header promises a function of the figure (placements,
lane-group sizes and the work-group path, coordinate layouts, host and device buffers, repeated calls); invalid rows must terminate
inside their row and their share."""
import ctypes as C
import os
from functools import lru_cache

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import DeviceGeoArray, GeoArrowArray
from geopolars_amd.geoseries import GeoSeries, triangulate_device
from tests import triangulate_ref as T
from tests import validity_ref as V
from tests.exact_ref import column

pytestmark = pytest.mark.gpu
PG, MPG = V.PG, V.MPG
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@lru_cache(maxsize=None)
def fixture(kind):
    """known_column and random_column(kind, 480, seed) for seeds 5, 6, 7 as one column: (rows, valid, codes)"""
    rows, valid, codes = [], [], []
    for r, v, c, _ in [V.known_column(kind)] + [V.random_column(kind, 480, seed) for seed in (5, 6, 7)]:
        rows += list(r)
        valid += list(v)
        codes += [int(x) for x in c]
    return rows, valid, np.array(codes)


def bases(kind, rows):
    return np.concatenate(([0], np.cumsum([V.n_coords(kind, r) for r in rows]))).astype(np.int64)


def group_of(kind, rows) -> int:
    """the lane-group size the library picks for the column: by its mean share"""
    return T.TRI_G_LARGE if sum(T.share(kind, r) for r in rows) / len(rows) >= T.TRI_G_MEAN else T.TRI_G_SMALL


def answers(kind, rows, valid=None):
    s = GeoSeries(column(kind, rows, valid))
    off, idx, st = s.triangulate(return_status=True)
    assert off[0] == 0 and off[-1] == len(idx) and (np.diff(off) >= 0).all()
    return off, idx, st


def check_column(kind, rows, valid, codes, got, full=True):
    """every row: safe; valid rows: status 0 (1 without a member) and the checker.  Returns the number of valid rows checked."""
    off, idx, st = got
    base = bases(kind, rows)
    n_valid = 0
    for i, row in enumerate(rows):
        tris = idx[off[i] : off[i + 1]].astype(np.int64)
        T.check_safe(kind, row, int(st[i]), tris, int(base[i]))
        ok = valid is None or valid[i]
        if not T.has_member(kind, row, ok):
            assert st[i] != T.TRI_OK and (st[i] == T.TRI_EMPTY or codes[i] != V.VALID), (i, int(st[i]))
        if codes[i] == V.VALID:
            n_valid += 1
            assert st[i] == (T.TRI_OK if T.has_member(kind, row, ok) else T.TRI_EMPTY), (i, int(st[i]), row)
            try:
                T.check_row(kind, row, tris, int(base[i]), full=full)
            except T.TriangulationError as e:
                raise AssertionError(f"row {i}: {e}\n{row}") from None
        elif codes[i] == V.NULL:
            assert st[i] == T.TRI_EMPTY
    return n_valid


@lru_cache(maxsize=None)
def fixture_answers(kind, pad):
    rows, valid, codes = fixture(kind)
    prows = V.padded(kind, rows, pad)
    return prows, answers(kind, prows, valid)


@pytest.mark.parametrize("pad", [0, 1, 2])
@pytest.mark.parametrize("kind", [PG, MPG])
def test_every_fixture_row(kind, pad):
    """all 400 (POLYGON) / 250 (MULTIPOLYGON) valid rows, none left out — among them a hole touching the shell mid-edge and at a
    repeated closing coordinate, two and three holes meeting at one point, members touching at a point, a member inside another
    member's hole — plain and with 1 / 2 collinear vertices inside every edge; every invalid, null and empty row stays safe"""
    rows, valid, codes = fixture(kind)
    prows, got = fixture_answers(kind, pad)
    pcodes = codes if pad == 0 else V.validity_column(kind, prows, valid)[0]
    n_valid = 9 + 391 if kind == PG else 13 + 237  # (the known answers + the three random columns)
    assert (codes == V.VALID).sum() == n_valid and np.array_equal(pcodes == V.VALID, codes == V.VALID)
    assert check_column(kind, prows, valid, pcodes, got) == n_valid


@pytest.mark.parametrize("kind", [PG, MPG])
def test_placements_give_identical_indices(kind):
    rows, valid, codes = fixture(kind)
    flat = lambda row: [v for ring in (row if kind == PG else [q for p in row for q in p]) for pt in ring for v in pt]  # noqa: E731
    keep = [i for i, r in enumerate(rows) if np.isfinite(flat(r)).all()]  # (a NaN has no exact placement)
    rows, valid = [rows[i] for i in keep], [valid[i] for i in keep]
    off, idx, st = answers(kind, rows, valid)
    assert check_column(kind, rows, valid, codes[keep], (off, idx, st)) > 200
    for scale, shift in V.PLACEMENTS:
        o, i, s = answers(kind, V.placed(kind, rows, scale, shift), valid)
        assert np.array_equal(o, off) and np.array_equal(i, idx) and np.array_equal(s, st), (scale, shift)


def device_call(dev, n, capacity, guard=0):
    """gpk_triangulate through device buffers: (offsets, index, status, total, the guard words after the index buffer)"""
    import torch

    off = torch.full((n + 1,), -5, dtype=torch.int32, device="cuda")
    st = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    buf = torch.full((3 * capacity + guard,), -9, dtype=torch.int32, device="cuda")
    total = triangulate_device(dev, buf[: 3 * capacity].view(capacity, 3) if capacity else None, off, st)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    return off.cpu().numpy(), b[: 3 * total].view(np.uint32).reshape(-1, 3) if capacity else None, st.cpu().numpy(), total, b[3 * capacity :]


@pytest.mark.parametrize("kind", [PG, MPG])
def test_layouts_buffers_and_repeats(kind):
    """host and device outputs, interleaved and separated (Struct<x, y>) coordinates, two calls: bit-identical"""
    import torch

    rows, valid, codes = fixture(kind)
    prows, (off, idx, st) = fixture_answers(kind, 0)
    a = column(kind, prows, valid)
    s = GeoSeries(a)
    again = s.triangulate(return_status=True)
    assert all(np.array_equal(x, y) for x, y in zip(again, (off, idx, st)))
    cap = a.n_coords + 3 * a.n_rings
    o, i, t, total, _ = device_call(s.device(), len(s), cap)
    assert total == len(idx) and np.array_equal(o, off) and np.array_equal(i, idx) and np.array_equal(t, st)
    dt = lambda x: None if x is None else torch.from_numpy(x).cuda()  # noqa: E731
    for xy in (dt(a.xy), (dt(np.ascontiguousarray(a.xy[:, 0])), dt(np.ascontiguousarray(a.xy[:, 1])))):
        view = DeviceGeoArray.from_device_buffers(kind, xy, dt(a.geom_offsets), dt(a.part_offsets), dt(a.ring_offsets), dt(a.validity))
        o, i, t, total, _ = device_call(view, len(s), cap)
        assert total == len(idx) and np.array_equal(o, off) and np.array_equal(i, idx) and np.array_equal(t, st)


@pytest.mark.parametrize("kind", [PG, MPG])
def test_both_lane_group_sizes_and_the_work_group_agree(kind):
    """the same rows on 4 lanes a row (slice of 32: the larger rows take the work-group) and on 16 (slice of 128): the column's mean
    share is pushed across TRI_G_MEAN by rows appended behind the fixture — 4096-coordinate rings to lift it, unit squares to lower
    it — and the fixture's rows must keep their indices"""
    rows, valid, codes = fixture(kind)
    prows, (off, idx, st) = fixture_answers(kind, 0)
    wrap = (lambda r: r) if kind == PG else (lambda r: [r])
    if group_of(kind, prows) == T.TRI_G_SMALL:
        extra, per = [wrap(V.zigzag(4096))] * 16, 4093
    else:
        extra, per = [wrap([V.sq(0, 0, 1, 1)])] * (2 * len(prows)), 2
    more = prows + extra
    assert {group_of(kind, prows), group_of(kind, more)} == {T.TRI_G_SMALL, T.TRI_G_LARGE}
    shares = np.array([T.share(kind, r) for r in prows])
    assert (shares > T.TRI_SLICE_SMALL).sum() >= 20 and shares.max() <= T.TRI_SLICE_LARGE  # 4 lanes: both the slice and the work-group
    o, i, s = answers(kind, more, valid + [True] * len(extra))
    n = len(prows)
    assert np.array_equal(o[: n + 1], off) and np.array_equal(i[: off[-1]], idx) and np.array_equal(s[:n], st)
    assert (s[n:] == T.TRI_OK).all() and (np.diff(o[n:]) == per).all()


def test_work_group_path_and_every_threshold():
    """zigzag(4096) with and without a hole (valid) and the four faulty zigzags; one row exactly at and one just above every size
    threshold: the slice of 16 lanes (share 128), the LDS list (share TRI_LDS_NODES; above it the list lies in global scratch)"""
    rows, codes, _ = V.large_column()
    edge = [V.zigzag(n) for n in (T.TRI_SLICE_LARGE - 3, T.TRI_SLICE_LARGE - 2, T.TRI_LDS_NODES - 3, T.TRI_LDS_NODES - 2)]
    assert [T.share(PG, r) for r in edge] == [T.TRI_SLICE_LARGE, T.TRI_SLICE_LARGE + 1, T.TRI_LDS_NODES, T.TRI_LDS_NODES + 1]
    allrows = list(rows) + edge
    allcodes = np.concatenate([codes, [V.VALID] * len(edge)])
    assert group_of(PG, allrows) == T.TRI_G_LARGE
    got = answers(PG, allrows)
    assert check_column(PG, allrows, None, allcodes, got) == 2 + len(edge)
    assert np.diff(got[0]).tolist()[-4:] == [len(r[0]) - 3 for r in edge]  # n - 1 positions, n - 3 triangles
    # the slice of 4 lanes (share 32) among small squares that keep the mean low
    small = [V.zigzag(T.TRI_SLICE_SMALL - 3), V.zigzag(T.TRI_SLICE_SMALL - 2)] + [[V.sq(0, 0, 2 + k, 3)] for k in range(40)]
    assert group_of(PG, small) == T.TRI_G_SMALL and [T.share(PG, r) for r in small[:2]] == [T.TRI_SLICE_SMALL, T.TRI_SLICE_SMALL + 1]
    assert all(V.validity(PG, r)[0] == V.VALID for r in small[:2])
    assert check_column(PG, small, None, np.zeros(len(small), dtype=int), answers(PG, small)) == len(small)


def _golden(name):
    z = np.load(os.path.join(GOLD, f"{name}.npz"))
    return GeoArrowArray.from_wkb(z["wkb_values"], z["wkb_offsets"])


def test_naturalearth_every_row():
    """177 rows with non-integer coordinates: status 0 and the full checker on every row"""
    a = _golden("naturalearth_lowres")
    kind, rows = T.array_rows(a)
    s = GeoSeries(a)
    assert len(rows) == 177 and s.is_valid().all()
    assert check_column(kind, rows, None, np.zeros(len(rows), dtype=int), s.triangulate(return_status=True)) == 177


def test_nybb_linear_checks():
    """five boroughs of up to 29 273 node slots (the global-scratch form): every row gpk_validity calls valid passes (a), (b), (d) and
    the directed-edge part of (c)"""
    a = _golden("nybb")
    kind, rows = T.array_rows(a)
    s = GeoSeries(a)
    ok = s.is_valid()
    assert max(T.share(kind, r) for r in rows) > T.TRI_LDS_NODES
    got = s.triangulate(return_status=True)
    codes = np.where(ok, V.VALID, V.SELF_INTERSECTION)
    assert check_column(kind, rows, None, codes, got, full=False) == int(ok.sum())


def test_capacity():
    import torch

    rows, valid, codes = fixture(PG)
    prows, (off, idx, st) = fixture_answers(PG, 0)
    s = GeoSeries(column(PG, prows, valid))
    n, total = len(s), len(idx)
    o, i, t, got, _ = device_call(s.device(), n, 0)  # the size query
    assert got == total and i is None and np.array_equal(o, off) and np.array_equal(t, st)
    o, i, t, got, guard = device_call(s.device(), n, total, guard=64)  # an exactly fitting buffer, guard words behind it
    assert got == total and np.array_equal(i, idx) and (guard == -9).all()
    o32 = torch.full((n + 1,), -5, dtype=torch.int32, device="cuda")
    buf = torch.full((3 * (total - 1) + 64,), -9, dtype=torch.int32, device="cuda")
    n_tri = C.c_int64(-1)
    rc = _abi.lib().gpk_triangulate(s.device().handle, buf.data_ptr(), total - 1, o32.data_ptr(), None, C.byref(n_tri), _abi.MEM_DEVICE, None)
    torch.cuda.synchronize()
    assert rc == _abi.GPK_ERR_CAPACITY and n_tri.value == total
    assert (buf.cpu().numpy() == -9).all() and np.array_equal(o32.cpu().numpy(), off)  # nothing written, the offsets still produced
    with pytest.raises(_abi.GeopolarsHipError):
        triangulate_device(s.device(), buf[: 3 * (total - 1)].view(total - 1, 3), o32)


def test_70001_rows_shuffled():
    """several blocks and a ragged tail: a shuffled tiling of the fixture; offsets monotone, every row equal to its base row's answer,
    re-based"""
    rows, valid, codes = fixture(MPG)
    prows, (off, idx, st) = fixture_answers(MPG, 0)
    n = 70001
    pick = np.random.default_rng(11).integers(0, len(prows), n)
    a0 = column(MPG, prows, valid)
    # the tiled column, built from the base column's buffers
    go, po, ro = a0.geom_offsets.astype(np.int64), a0.part_offsets.astype(np.int64), a0.ring_offsets.astype(np.int64)
    np_parts = (go[1:] - go[:-1])[pick]
    part_src = np.concatenate([np.arange(go[r], go[r + 1]) for r in pick]) if n else np.zeros(0, dtype=np.int64)
    nr = (po[1:] - po[:-1])[part_src]
    ring_src = np.repeat(po[part_src] - np.concatenate(([0], np.cumsum(nr)[:-1])), nr) + np.arange(nr.sum())
    nc = (ro[1:] - ro[:-1])[ring_src]
    coord_src = np.repeat(ro[ring_src] - np.concatenate(([0], np.cumsum(nc)[:-1])), nc) + np.arange(nc.sum())
    cum = lambda v: np.concatenate(([0], np.cumsum(v))).astype(np.int32)  # noqa: E731
    vbits = np.packbits(np.array(valid, dtype=bool)[pick], bitorder="little")
    tiled = GeoArrowArray(MPG, a0.xy[coord_src], geom_offsets=cum(np_parts), part_offsets=cum(nr), ring_offsets=cum(nc), validity=vbits)
    o, i, s = GeoSeries(tiled).triangulate(return_status=True)
    assert (np.diff(o) >= 0).all() and np.array_equal(s, st[pick]) and np.array_equal(np.diff(o), np.diff(off)[pick])
    base0 = bases(MPG, prows)
    new_base = np.concatenate(([0], np.cumsum((base0[1:] - base0[:-1])[pick])))
    cnt = np.diff(off)[pick]
    src = np.repeat(off[:-1][pick] - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt) + np.arange(cnt.sum())
    shift = np.repeat(new_base[:-1] - base0[:-1][pick], cnt)
    assert np.array_equal(i.astype(np.int64), idx[src].astype(np.int64) + shift[:, None])


def test_triangles_series():
    """triangles(): four coordinates a ring, counter-clockwise by exact orientation, the input's coordinates bit for bit; the areas per
    parent sum to the parent's area; every triangle's representative point lies in its parent"""
    a = _golden("naturalearth_lowres")
    s = GeoSeries(a)
    off, idx = s.triangulate()
    tri, parents = s.triangles(return_parents=True)
    t = tri.array
    assert t.geom_type == PG and len(tri) == len(idx) and np.array_equal(t.ring_offsets, np.arange(0, 4 * len(idx) + 1, 4))
    ring = t.xy.reshape(-1, 4, 2)
    assert np.array_equal(ring[:, :3], a.xy[idx.astype(np.int64)]) and np.array_equal(ring[:, 3], ring[:, 0])
    ints = T._ints([tuple(p) for p in ring[:200].reshape(-1, 2)])
    assert all(T._orient(ints[4 * k], ints[4 * k + 1], ints[4 * k + 2]) > 0 for k in range(200))
    assert np.array_equal(parents, np.repeat(np.arange(len(s)), np.diff(off)))
    total = np.bincount(parents, weights=tri.area(), minlength=len(s))
    area = s.area()
    assert (np.abs(total - area) <= 1e-9 * area).all()
    # representative_point promises a strictly interior point where the widest section is at least 1e-6 of the row's diagonal: the
    # slivers among 9791 real triangles are below that, the others must lie in their parent
    pts, width = tri.representative_point(return_width=True)
    b = tri.bounds()
    wide = width >= 1e-6 * np.hypot(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1])
    assert wide.sum() > 0.9 * len(wide)
    assert pts.within(s, parents.astype(np.uint32))[wide].all()  # (row-wise: point k against its parent row — contains, from the point's side)
    # every triangle of the lattice fixture is wide: no row left out
    rows, valid, codes = fixture(PG)
    f = GeoSeries(column(PG, rows, valid))
    tri, parents = f.triangles(return_parents=True)
    assert len(tri) == fixture_answers(PG, 0)[1][0][-1] > 3000
    total = np.bincount(parents, weights=tri.area(), minlength=len(f))
    ok = codes == V.VALID
    assert np.array_equal(total[ok], f.area()[ok])  # (small integers: the float sums are exact)
    assert tri.representative_point().within(f, parents.astype(np.uint32))[ok[parents]].all() and ok[parents].sum() > 2000
