"""The entry points with optional outputs or optional row maps, through the C ABI: every combination of host or device buffers and
of each optional argument present or absent gives, bit for bit, what the call with everything present and host buffers gives — on a
column of 5 rows (a live row on each side of a null row and of an empty row) and on a column of 0 rows.  Most of these entry points return at 0 rows before they plan any scratch, so
there the 0-row case pins that early return for every combination of arguments; only the clips plan with 0 rows (their lists are
sized for at least one pair).  The rule that a carve of zero bytes is still a carve is checked on the host side
(tests/test_scratch_host.py), not here.  What goes wrong when a call's scratch record loses a carve or flips a condition shows on exactly one of
these combinations; the values themselves are pinned by the suites of the operators."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from geopolars_amd import _abi, synth
from geopolars_amd.geoarrow import DeviceGeoArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import SpatialIndex
from tests import exact_ref as X

pytestmark = pytest.mark.gpu

HOST, DEV = _abi.MEM_HOST, _abi.MEM_DEVICE
PT, LS, PG = _abi.GEOM_POINT, _abi.GEOM_LINESTRING, _abi.GEOM_POLYGON
VALID5 = [True, False, True, True, True]  # row 1 is null, row 3 is empty


def _square(x, y, s=2.0):
    return [[(x, y), (x + s, y), (x + s, y + s), (x, y + s), (x, y)]]


def _column(kind, n):
    """5 rows: live, null, live, empty, live — or no row at all"""
    if n == 0:
        return GeoSeries(X.column(kind, []))
    if kind == PT:
        rows = [(0.5, 0.5), (4.5, 0.5), (8.5, 1.0), None, (12.25, 1.5)]
    elif kind == LS:
        rows = [[(0.0, 0.0), (1.0, 1.0), (3.0, 1.0)], [(4.0, 0.0), (5.0, 1.0)], [(7.0, -1.0), (9.0, 3.0), (10.0, 0.5)], [], [(11.0, 1.0), (14.0, 1.0)]]
    else:
        rows = [_square(0, 0), _square(4, 0), _square(8, 0) + [[(8.5, 0.5), (8.5, 1.5), (9.5, 1.5), (9.5, 0.5), (8.5, 0.5)]], [], _square(12, 0)]
    return GeoSeries(X.column(kind, rows, VALID5))


class Buf:
    """`count` elements of `dtype` in `space`, filled with 0x5A bytes (or with `values`), never of zero length: its address is handed over"""

    def __init__(self, count, dtype, space, values=None):
        self.count, self.dtype = count, np.dtype(dtype)
        raw = np.full(max(count, 1) * self.dtype.itemsize, 0x5A, np.uint8)
        if values is not None:
            raw[: count * self.dtype.itemsize] = np.asarray(values, dtype).view(np.uint8)
        self.t = raw if space == HOST else torch.from_numpy(raw).cuda()

    @property
    def ptr(self):
        return self.t.ctypes.data if isinstance(self.t, np.ndarray) else self.t.data_ptr()

    def bytes(self, count=None):
        raw = self.t if isinstance(self.t, np.ndarray) else self.t.cpu().numpy()
        return raw[: (self.count if count is None else count) * self.dtype.itemsize].tobytes()


def _ptr(b):
    return None if b is None else b.ptr


def _opt(present, *args):
    return Buf(*args) if present else None


def _combos(options):
    """(space, {option: present}) for both spaces and every subset of the options; the first is the reference: host, all present"""
    out = []
    for space in (HOST, DEV):
        for present in itertools.product((True, False), repeat=len(options)):
            out.append((space, dict(zip(options, present))))
    return out


def _check(run, options):
    """run(space, present) -> {name: bytes} of the outputs that were asked for; every combination == the reference on what it has"""
    combos = _combos(options)
    want = run(*combos[0])
    for space, present in combos[1:]:
        got = run(space, present)
        torch.cuda.synchronize()
        for name, value in got.items():
            assert value == want[name], (name, "device" if space == DEV else "host", present)
        assert set(got) <= set(want)
    return want


def _ok(rc):
    assert rc == _abi.GPK_OK, _abi.last_error()
    torch.cuda.synchronize()


ROWS = [0, 5]


@pytest.mark.parametrize("n", ROWS)
def test_minimum_bounding_circle(gpk, n):
    a = _column(PG, n)

    def run(space, p):
        centre, radius, valid = _opt(p["out_center"], 2 * n, "f8", space), Buf(n, "f8", space), _opt(p["out_valid"], n, "u1", space)
        _ok(_abi.lib().gpk_minimum_bounding_circle(a.device().handle, _ptr(centre), radius.ptr, _ptr(valid), space, None))
        return {k: b.bytes() for k, b in (("centre", centre), ("radius", radius), ("valid", valid)) if b is not None}

    want = _check(run, ["out_center", "out_valid"])
    if n:
        assert np.frombuffer(want["valid"], np.uint8).tolist() == [1, 0, 1, 0, 1]


@pytest.mark.parametrize("n", ROWS)
def test_minimum_rotated_rectangle(gpk, n):
    a = _column(PG, n)

    def run(space, p):
        rect, valid = Buf(10 * n, "f8", space), _opt(p["out_valid"], n, "u1", space)
        _ok(_abi.lib().gpk_minimum_rotated_rectangle(a.device().handle, rect.ptr, _ptr(valid), space, None))
        return {k: b.bytes() for k, b in (("rect", rect), ("valid", valid)) if b is not None}

    _check(run, ["out_valid"])


@pytest.mark.parametrize("kind", [PT, LS, PG])
@pytest.mark.parametrize("n", ROWS)
def test_centroid(gpk, n, kind):
    a = _column(kind, n)

    def run(space, p):
        xy, valid = Buf(2 * n, "f8", space), _opt(p["out_valid"], n, "u1", space)
        _ok(_abi.lib().gpk_centroid(a.device().handle, xy.ptr, _ptr(valid), space, None))
        return {k: b.bytes() for k, b in (("xy", xy), ("valid", valid)) if b is not None}

    _check(run, ["out_valid"])


@pytest.mark.parametrize("kind", [PT, LS, PG])
@pytest.mark.parametrize("n", ROWS)
def test_representative_point(gpk, n, kind):
    a = _column(kind, n)

    def run(space, p):
        xy, valid, width = Buf(2 * n, "f8", space), _opt(p["out_valid"], n, "u1", space), _opt(p["out_width"], n, "f8", space)
        _ok(_abi.lib().gpk_representative_point(a.device().handle, xy.ptr, _ptr(valid), _ptr(width), space, None))
        return {k: b.bytes() for k, b in (("xy", xy), ("valid", valid), ("width", width)) if b is not None}

    _check(run, ["out_valid", "out_width"])


@pytest.mark.parametrize("n", ROWS)
def test_closest_point(gpk, n):
    a, b = _column(PT, n), _column(LS, n)

    def run(space, p):
        rows = _opt(p["b_rows"], n, "u4", space, np.arange(n))  # (the identity: the answer with and without the list is the same)
        xy, seg = Buf(2 * n, "f8", space), _opt(p["out_seg"], n, "i4", space)
        _ok(_abi.lib().gpk_closest_point_rowwise(a.device().handle, b.device().handle, _ptr(rows), xy.ptr, _ptr(seg), space, None))
        return {k: v.bytes() for k, v in (("xy", xy), ("seg", seg)) if v is not None}

    _check(run, ["out_seg", "b_rows"])


@pytest.mark.parametrize("entry", ["gpk_hausdorff_distance", "gpk_frechet_distance"])
@pytest.mark.parametrize("n", ROWS)
def test_hausdorff_and_frechet(gpk, n, entry):
    a, b = _column(LS, n), _column(LS, n)

    def run(space, p):
        rows, out = _opt(p["b_rows"], n, "u4", space, np.arange(n)), Buf(n, "f8", space)
        if entry == "gpk_hausdorff_distance":
            _ok(_abi.lib().gpk_hausdorff_distance(a.device().handle, b.device().handle, _ptr(rows), 1, out.ptr, space, None))
            return {"out": out.bytes()}
        n_over = C.c_int64(-1)
        _ok(_abi.lib().gpk_frechet_distance(a.device().handle, b.device().handle, _ptr(rows), 1, out.ptr, C.byref(n_over) if p["n_over"] else None,
                                            space, None))
        return {"out": out.bytes(), **({"n_over": int(n_over.value)} if p["n_over"] else {})}

    _check(run, ["b_rows"] + (["n_over"] if entry == "gpk_frechet_distance" else []))


@pytest.mark.parametrize("n", ROWS)
def test_dwithin_rowwise(gpk, n):
    a, b = _column(PT, n), _column(PG, n)

    def run(space, p):
        rows, out = _opt(p["b_rows"], n, "u4", space, np.arange(n)), Buf(n, "u1", space)
        _ok(_abi.lib().gpk_dwithin_rowwise(a.device().handle, b.device().handle, _ptr(rows), 0.75, out.ptr, space, None))
        return {"out": out.bytes()}

    _check(run, ["b_rows"])


@pytest.mark.parametrize("n", ROWS)
def test_validity(gpk, n):
    a = _column(PG, n)

    def run(space, p):
        code, where = Buf(n, "u1", space), _opt(p["out_where"], n, "i4", space)
        _ok(_abi.lib().gpk_validity(a.device().handle, code.ptr, _ptr(where), space, None))
        return {k: v.bytes() for k, v in (("code", code), ("where", where)) if v is not None}

    _check(run, ["out_where"])


@pytest.mark.parametrize("n", ROWS)
def test_triangulate(gpk, n):
    a = _column(PG, n)
    cap = 64

    def run(space, p):
        index, offsets, status = Buf(3 * cap, "u4", space), Buf(n + 1, "i4", space), _opt(p["out_status"], n, "u1", space)
        n_tri = C.c_int64(-1)
        _ok(_abi.lib().gpk_triangulate(a.device().handle, index.ptr, cap, offsets.ptr, _ptr(status), C.byref(n_tri), space, None))
        out = {"index": index.bytes(3 * int(n_tri.value)), "offsets": offsets.bytes(), "n": int(n_tri.value)}
        return {**out, **({"status": status.bytes()} if status is not None else {})}

    want = _check(run, ["out_status"])
    assert (want["n"] > 0) == (n > 0)


def _column_bytes(handle, geom_type):
    """everything a result column holds, and its release"""
    dev = DeviceGeoArray(handle, geom_type, 0, -1)
    host = dev.download()
    levels = [o.tobytes() for o in (host.geom_offsets, host.part_offsets, host.ring_offsets) if o is not None]
    return {"rows": host.n_geoms, "levels": levels, "xy": host.xy.tobytes(), "validity": None if host.validity is None else host.validity.tobytes()}


@pytest.mark.parametrize("entry", ["gpk_line_clip", "gpk_polygon_clip"])
@pytest.mark.parametrize("n", ROWS)
def test_clip(gpk, n, entry):
    """out_src with DROP_EMPTY, out_status (polygon clip), and the row lists on the host or on the device — each in its own space"""
    a, b = _column(LS if entry == "gpk_line_clip" else PG, n), _column(PG, n)
    # (pair k: row k of a against row k of b shifted by half a unit, so that live pairs meet)
    b = GeoSeries(X.translated_exactly(b.array, (0.5, 0.5))) if n else b
    result_type = _abi.GEOM_MULTILINESTRING if entry == "gpk_line_clip" else _abi.GEOM_MULTIPOLYGON
    options = ["out_src"] + (["out_status"] if entry == "gpk_polygon_clip" else [])

    def run(space, p):
        got = {}
        for rows_space in (HOST, DEV):
            a_rows, b_rows = Buf(n, "u4", rows_space, np.arange(n)), Buf(n, "u4", rows_space, np.arange(n))
            src, status = _opt(p["out_src"], n, "i4", space), _opt(p.get("out_status", False), n, "u1", space)
            out = C.c_void_p()
            args = [a.device().handle, b.device().handle, a_rows.ptr, b_rows.ptr, n, rows_space, _abi.CLIP_INSIDE, _abi.CLIP_DROP_EMPTY, _ptr(src), space]
            if entry == "gpk_polygon_clip":
                args += [_ptr(status), space]
            _ok(getattr(_abi.lib(), entry)(*args, None, C.byref(out)))
            col = _column_bytes(out.value, result_type)
            one = {"column": col, **({"src": src.bytes(col["rows"])} if src is not None else {}), **({"status": status.bytes()} if status is not None else {})}
            if got:
                assert one == got, ("row lists on the device", p)
            got = one
        return got

    want = _check(run, options)
    assert (want["column"]["rows"] > 0) == (n > 0)
    if n:
        src = np.frombuffer(want["src"], np.int32)
        assert len(src) == want["column"]["rows"] and (np.diff(src) > 0).all() and src[0] >= 0 and src[-1] < n


@pytest.mark.parametrize("n", ROWS)
def test_spatial_join(gpk, n):
    """out_counts present or absent, a pairs capacity of 0 or more"""
    left = _column(PT, n)
    right = GeoSeries(X.column(PG, [_square(0, 0), _square(4, 0), _square(8, 0), [], _square(12, 0)], VALID5))
    index = SpatialIndex(right)

    def run(space, p):
        cap = 8 if p["pairs"] else 0
        counts, pairs = _opt(p["out_counts"], n, "u4", space), _opt(p["pairs"], 2 * cap, "u4", space)
        total = C.c_int64(-1)
        _ok(_abi.lib().gpk_spatial_join(left.device().handle, right.device().handle, index.handle, _abi.PRED_INTERSECTS, 0, _ptr(counts), _ptr(pairs), cap,
                                        C.byref(total), space, None))
        out = {"total": int(total.value)}
        if counts is not None:
            out["counts"] = counts.bytes()
        if pairs is not None:
            out["pairs"] = pairs.bytes(2 * int(total.value))
        return out

    want = _check(run, ["out_counts", "pairs"])
    assert (want["total"] > 0) == (n > 0) and int(np.frombuffer(want["counts"], np.uint32).sum()) == want["total"]


def test_second_async_join_on_one_stream_repeats_the_first(gpk):
    """two consecutive gpk_spatial_join_async calls with one index on one stream: the second finds the rare arm's record of the first
    at the same place of the stream's arena and skips the launch that writes it — counts, pairs and total are identical.  The index
    has a routing image (the one-launch join), and gpk_join_prep is launched ONCE over the two calls: by the first, for an index
    this arena has not seen; the chain kernel's path would launch it twice, the queue kernels' never"""
    n = 20_000
    polys, pts = GeoSeries(synth.star_polygons(1000, 64)), GeoSeries(synth.uniform_points(n, seed=7))
    index = SpatialIndex(polys)
    assert index.describe()["route"] == 1
    lib, stream = _abi.lib(), torch.cuda.current_stream().cuda_stream
    outs = []
    torch.cuda.synchronize()
    lib.gpk_profile_reset()
    lib.gpk_profile_filter(b"gpk_join_prep")
    lib.gpk_profile_enable(1)
    try:
        for _ in range(2):
            counts, pairs, total = Buf(n, "u4", DEV), Buf(2 * n, "u4", DEV), Buf(1, "i8", DEV)
            rc = lib.gpk_spatial_join_async(pts.device().handle, polys.device().handle, index.handle, _abi.PRED_INTERSECTS, 0, counts.ptr, pairs.ptr, n,
                                            total.ptr, stream)  # (no host wait between the two)
            assert rc == _abi.GPK_OK, _abi.last_error()
            outs.append((counts, pairs, total))
        torch.cuda.synchronize()
    finally:
        lib.gpk_profile_enable(0)
        lib.gpk_profile_filter(None)
    ms, launches = C.c_double(0), C.c_int64(-1)
    lib.gpk_profile_query(b"gpk_join_prep", C.byref(ms), C.byref(launches))
    lib.gpk_profile_reset()
    assert launches.value == 1, launches.value
    first, second = [(c.bytes(), p.bytes(), t.bytes()) for c, p, t in outs]
    assert first == second
    total = int(np.frombuffer(first[2], np.int64)[0])
    assert 0 < total <= n and int(np.frombuffer(first[0], np.uint32).sum()) == total
