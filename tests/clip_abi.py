"""gpk_line_clip, gpk_polygon_clip and gpk_polygon_union called through ctypes, past the Python layer: that layer returns early on zero
pairs, so the library's own n == 0 branch, a result from which every pair is dropped and the last, partial byte of the validity bitmap
are reached only from here.  The checks are shared by tests/test_gpu_lineclip.py, test_gpu_polyclip.py and test_gpu_polyunion.py;
nothing in this file is collected as a test."""
import ctypes as C

import numpy as np
import torch

from geopolars_amd import _abi
from geopolars_amd.geoarrow import DeviceGeoArray
from geopolars_amd.geoseries import GeoSeries
from tests import exact_ref as X

LS, PG = _abi.GEOM_LINESTRING, _abi.GEOM_POLYGON
RESULT_TYPE = {"gpk_line_clip": _abi.GEOM_MULTILINESTRING, "gpk_polygon_clip": _abi.GEOM_MULTIPOLYGON, "gpk_polygon_union": _abi.GEOM_MULTIPOLYGON}


def unit_square(x, y):
    return [[(x, y), (x + 1, y), (x + 1, y + 1), (x, y + 1), (x, y)]]


def unit_line(x, y):
    """the diagonal of unit_square(x, y)"""
    return [(x, y), (x + 1, y + 1)]


def disjoint_sides(entry):
    """two columns of three unit shapes: no shape of the first meets a shape of the second"""
    a = [unit_line(4 * k, 0) for k in range(3)] if entry == "gpk_line_clip" else [unit_square(4 * k, 0) for k in range(3)]
    return GeoSeries(X.column(LS if entry == "gpk_line_clip" else PG, a)), GeoSeries(X.column(PG, [unit_square(4 * k + 2, 0) for k in range(3)]))


def meeting_sides(entry):
    """two columns of one row each: a unit shape, and a square of side 3 that holds it in its interior"""
    a = X.column(LS, [unit_line(0, 0)]) if entry == "gpk_line_clip" else X.column(PG, [unit_square(0, 0)])
    return GeoSeries(a), GeoSeries(X.column(PG, [[[(-1, -1), (2, -1), (2, 2), (-1, 2), (-1, -1)]]]))


def _ptr(t):
    if t is None:
        return None
    return t.data_ptr() if isinstance(t, torch.Tensor) else t.ctypes.data


def _in_space(values, dtype, space):
    """a list for the call: a numpy array (MEM_HOST) or a CUDA tensor (MEM_DEVICE), never of zero length (its address is handed over)"""
    host = np.asarray(values if len(values) else [0]).astype(dtype)
    return host if space == _abi.MEM_HOST else torch.from_numpy(host.view(np.int32)).cuda()


def call(entry, a, b, a_rows, b_rows, n, mode, flags, out_src=None, space=_abi.MEM_HOST):
    """-> (status, the owned result as a DeviceGeoArray or None)"""
    out = C.c_void_p()
    args = [a.device().handle, b.device().handle, _ptr(a_rows), _ptr(b_rows), n, space, mode, flags, _ptr(out_src), space]
    if entry != "gpk_line_clip":
        args += [None, _abi.MEM_HOST]  # no out_status
    rc = getattr(_abi.lib(), entry)(*args, None, C.byref(out))
    return rc, (DeviceGeoArray(out.value, RESULT_TYPE[entry], 0, -1) if out.value else None)


def levels(host):
    """the offsets of every level the result's type has"""
    return [o.tolist() for o in (host.geom_offsets, host.part_offsets, host.ring_offsets) if o is not None]


def n_levels(entry):
    return 2 if entry == "gpk_line_clip" else 3


def take(dev):
    """(rows by gpk_geoarray_len, the downloaded column, the status of gpk_geoarray_free)"""
    n = C.c_int64(-1)
    _abi.check(_abi.lib().gpk_geoarray_len(dev.handle, C.byref(n)))
    host = dev.download()
    rc = _abi.lib().gpk_geoarray_free(dev.handle)
    dev._h = C.c_void_p()  # (freed here: nothing left for the object to free)
    return int(n.value), host, rc


def check_zero_pairs(entry, mode):
    """n_rows = 0 with row lists given: GPK_OK, a column of 0 rows whose offsets are [0] at every level, no coordinates, a clean free"""
    a, b = meeting_sides(entry)
    for space in (_abi.MEM_HOST, _abi.MEM_DEVICE):
        for flags in (0, _abi.CLIP_DROP_EMPTY):
            rows = _in_space([], np.uint32, space)
            rc, dev = call(entry, a, b, rows, rows, 0, mode, flags, space=space)
            assert rc == _abi.GPK_OK and dev is not None, (space, flags, _abi.last_error())
            n, host, freed = take(dev)
            assert n == 0 and host.n_geoms == 0 and levels(host) == [[0]] * n_levels(entry), (space, flags, levels(host))
            assert host.xy.shape == (0, 2) and host.validity is None and freed == _abi.GPK_OK


def check_every_pair_dropped(entry, mode):
    """three pairs of disjoint shapes.  DROP_EMPTY: 0 rows, offsets [0], out_src as it was; without it: 3 valid empty rows and a
    bitmap of one byte"""
    a, b = disjoint_sides(entry)
    for space in (_abi.MEM_HOST, _abi.MEM_DEVICE):
        rows = _in_space([0, 1, 2], np.uint32, space)
        src = _in_space([-1, -1, -1], np.int32, space)
        rc, dev = call(entry, a, b, rows, rows, 3, mode, _abi.CLIP_DROP_EMPTY, out_src=src, space=space)
        assert rc == _abi.GPK_OK and dev is not None, (space, _abi.last_error())
        n, host, freed = take(dev)
        torch.cuda.synchronize()
        assert n == 0 and levels(host) == [[0]] * n_levels(entry) and host.xy.shape == (0, 2) and freed == _abi.GPK_OK
        assert (src.cpu().numpy() if space == _abi.MEM_DEVICE else src).tolist() == [-1, -1, -1]
        rc, dev = call(entry, a, b, rows, rows, 3, mode, 0, space=space)
        assert rc == _abi.GPK_OK and dev is not None, (space, _abi.last_error())
        n, host, freed = take(dev)
        assert n == 3 and levels(host) == [[0, 0, 0, 0]] + [[0]] * (n_levels(entry) - 1) and host.xy.shape == (0, 2) and freed == _abi.GPK_OK
        assert host.validity is not None and host.validity.tolist() == [0b111]


def check_bitmap_edge(entry, mode):
    """9 pairs, the last with a row index past the end of its column: a bitmap of two bytes, the second partial"""
    a, b = meeting_sides(entry)
    for space in (_abi.MEM_HOST, _abi.MEM_DEVICE):
        a_rows, b_rows = _in_space([0] * 8 + [len(a)], np.uint32, space), _in_space([0] * 9, np.uint32, space)
        rc, dev = call(entry, a, b, a_rows, b_rows, 9, mode, 0, space=space)
        assert rc == _abi.GPK_OK and dev is not None, (space, _abi.last_error())
        n, host, freed = take(dev)
        assert n == 9 and len(host.geom_offsets) == 10 and freed == _abi.GPK_OK
        assert host.validity is not None and host.validity.tolist() == [0xFF, 0x00] and host.is_valid().tolist() == [True] * 8 + [False]
        assert (np.diff(host.geom_offsets) == [1] * 8 + [0]).all()  # every pair that has both rows gives the shape back, in one part
