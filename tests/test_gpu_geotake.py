"""gpk_geoarray_take / gpk_geoarray_filter on the GPU (csrc/gpk_geotake.hip) against GeoArrowArray.take on the host: every comparison
is exact — offsets level by level, is_valid(), whether there is a bitmap at all, the coordinates bit for bit.  Columns, index lists
and the hand-built shapes: tests/geotake_cases.py (the fill's strip is 1024 output elements, its LDS window 2048 row starts).  Every
case runs with host and with device idx / mask."""
import ctypes as C

import numpy as np
import pytest

from geopolars_amd import _abi, synth
from geopolars_amd.geoarrow import DeviceGeoArray, GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import SpatialJoinArgs, join_indices, join_pairs, spatial_join
from tests import geotake_cases as K
from tests.second_pass import same_bits

pytestmark = pytest.mark.gpu

COLUMNS = K.columns()
EDGES = K.edge_columns()


def _on_device(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _take_both_ways(dev: DeviceGeoArray, host: GeoArrowArray, idx, what):
    want = K.expected_take(host, idx)
    for where, ix in (("host idx", idx), ("device idx", _on_device(idx))):
        got = dev.take(ix)
        assert (got.n_geoms, got.n_coords) == (len(want), want.n_coords), (what, where)
        K.assert_same(got.download(), want, (what, where))


def _filter_raw(dev: DeviceGeoArray, mask: np.ndarray, bits: int, on_device: bool):
    """gpk_geoarray_filter itself, with either mask form -> (column, n_kept)"""
    m = np.packbits(mask, bitorder="little") if bits == 1 else mask.astype(np.uint8)
    keep = _on_device(m) if on_device else m
    ptr = (keep.data_ptr() if on_device else keep.ctypes.data) if len(m) else None
    h, kept = C.c_void_p(), C.c_int64(-1)
    _abi.check(_abi.lib().gpk_geoarray_filter(dev.handle, ptr, bits, _abi.MEM_DEVICE if on_device else _abi.MEM_HOST, None, C.byref(h), C.byref(kept)))
    return dev._owned_result(h, 0), int(kept.value)


@pytest.mark.parametrize("name", list(COLUMNS))
def test_take_equals_the_host_take_for_every_type(gpk, name):
    host = COLUMNS[name]
    dev = DeviceGeoArray.upload(host)
    for what, idx in K.index_lists(len(host), seed=len(name)).items():
        _take_both_ways(dev, host, idx, (name, what))


@pytest.mark.parametrize("name", list(EDGES))
def test_take_at_the_strip_and_window_boundaries(gpk, name):
    """rows that span three strips, that end on / one before / one after a strip boundary, 1024 rows in a strip, more empty rows in a
    strip than the LDS window holds (the fallback to bisecting in global memory), rows without parts / rings / coordinates, a result
    without coordinates"""
    host = EDGES[name]
    dev = DeviceGeoArray.upload(host)
    lists = K.index_lists(len(host), seed=len(name))
    if name == "multipoint empty run":  # only empty rows: a result whose coordinate total is 0, of more rows than a window
        lists["only empty rows"] = np.arange(1, 5001, dtype=np.int64)
    for what, idx in lists.items():
        _take_both_ways(dev, host, idx, (name, what))


def test_a_bitmap_appears_only_with_a_null(gpk):
    host = COLUMNS["linestring"]
    dev = DeviceGeoArray.upload(host)
    pts = DeviceGeoArray.upload(COLUMNS["point"])
    idx = np.array([5, 4, 4, 0, 516], np.int64)
    assert dev.take(idx).download().validity is None and pts.take(idx).download().validity is None
    for d, n in ((dev, len(host)), (pts, len(COLUMNS["point"]))):
        for bad in (-1, n, 1 << 40, -(1 << 40)):
            idx[2] = bad
            got = d.take(idx).download()
            assert got.validity is not None and np.array_equal(got.is_valid(), [True, True, False, True, True])
    got = pts.take(idx).download()
    assert np.isnan(got.xy[2]).all() and same_bits(got.xy[[0, 1, 3, 4]], COLUMNS["point"].xy[[5, 4, 0, 516]])


def test_take_at_scale_compared_in_full(gpk):
    host = synth.clustered_polygons(701)
    idx = np.random.default_rng(5).integers(0, len(host), 70_001).astype(np.int64)
    _take_both_ways(DeviceGeoArray.upload(host), host, idx, "70 001 indices")


@pytest.mark.parametrize("name", list(COLUMNS) + ["multipoint empty run", "linestring strips"])
def test_filter_equals_the_host_take_of_the_kept_rows(gpk, name):
    """all false, all true, random at 0.5 and 0.01; a byte a row and an Arrow bitmap; host and device masks; n % 8 != 0"""
    host = {**COLUMNS, **EDGES}[name]
    n = len(host)
    assert n % 8 != 0
    dev = DeviceGeoArray.upload(host)
    rng = np.random.default_rng(len(name))
    for what, mask in (("none", np.zeros(n, bool)), ("all", np.ones(n, bool)), ("0.5", rng.uniform(size=n) < 0.5), ("0.01", rng.uniform(size=n) < 0.01)):
        want = host.take(np.nonzero(mask)[0])
        for bits in (8, 1):
            for on_device in (False, True):
                got, kept = _filter_raw(dev, mask, bits, on_device)
                assert kept == int(mask.sum()) == got.n_geoms, (name, what, bits, on_device)
                K.assert_same(got.download(), want, (name, what, bits, on_device))
        K.assert_same(dev.filter(mask).download(), want, (name, what, "numpy"))
        K.assert_same(dev.filter(_on_device(mask)).download(), want, (name, what, "torch bool"))
        K.assert_same(dev.filter(_on_device(mask.astype(np.uint8))).download(), want, (name, what, "torch uint8"))


def test_take_of_a_take_and_a_source_freed_first(gpk):
    host = COLUMNS["multipolygon+nulls"]
    dev = DeviceGeoArray.upload(host)
    rng = np.random.default_rng(9)
    first = rng.integers(0, len(host), 300).astype(np.int64)
    second = rng.integers(0, 300, 500).astype(np.int64)
    once = dev.take(first)
    twice = once.take(_on_device(second))
    dev.free()
    once.free()  # the result owns all of its buffers
    K.assert_same(twice.download(), host.take(first[second]), "take of a take")


def test_a_source_that_is_a_zero_copy_view_of_device_buffers(gpk):
    host = COLUMNS["polygon"]
    tensors = {k: _on_device(getattr(host, k)) for k in ("geom_offsets", "ring_offsets")}
    view = DeviceGeoArray.from_device_buffers(host.geom_type, _on_device(host.xy), **tensors)
    idx = K.index_lists(len(host), seed=3)["3n draws"]
    _take_both_ways(view, host, idx, "device view")
    mask = np.random.default_rng(4).uniform(size=len(host)) < 0.3
    K.assert_same(view.filter(mask).download(), host.take(np.nonzero(mask)[0]), "device view, filter")


def test_geoseries_indexing_take_and_filter(gpk):
    host = synth.clustered_polygons(701, seed=4)
    s = GeoSeries(host)
    rng = np.random.default_rng(2)
    mask = rng.uniform(size=len(host)) < 0.4
    idx = rng.integers(0, len(host), 900)
    for got, want in ((s[10:20], host.take(np.arange(10, 20))), (s[::-3], host.take(np.arange(len(host))[::-3])), (s[mask], host.take(np.nonzero(mask)[0])),
                      (s[idx], host.take(idx)), (s[idx.astype(np.int32)], host.take(idx)), (s.take(list(idx[:7])), host.take(idx[:7])),
                      (s.filter(mask), host.take(np.nonzero(mask)[0]))):
        assert got._array is None and got._dev is not None and len(got) == len(want)  # device-resident
        K.assert_same(got.array, want)
    with_null = np.array([3, -1, 700, -1, 0], np.int64)
    got = s.take(with_null, allow_null=True)
    K.assert_same(got.array, K.expected_take(host, with_null))
    # The gathered column serves the kernels: area() of it equals s.area()[idx] bit for bit.  The area kernel sums a ring in an order
    # fixed by where the ring lies in the coordinate buffer (csrc/gpk_ringstream.hip: four consecutive coordinates a lane, strips of
    # the buffer), so moving a row may change the rounding of an inexact sum, whoever moves it: the column for this equality has
    # coordinates on an integer lattice, where every shoelace term and every partial sum is an exact integer below 2^53 in any order.
    # On the ragged column the same layout gives the same bits: the gathered column against the uploaded host take.
    lattice = GeoArrowArray(host.geom_type, np.round(host.xy * 16.0), host.geom_offsets, ring_offsets=host.ring_offsets)
    sl = GeoSeries(lattice)
    area = sl.area()
    assert (area > 0).all() and (area == np.round(area * 2) / 2).all()
    assert same_bits(sl[idx].area(), area[idx])
    assert same_bits(s[idx].area(), GeoSeries(host.take(idx)).area())


@pytest.mark.parametrize("join_type", ["inner", "left"])
def test_join_returns_native_geometry(gpk, join_type):
    import pyarrow as pa

    polys = synth.star_polygons(60, 12)
    pts = synth.uniform_points(1500, seed=31)
    lhs = pa.table({"geometry": pts.to_arrow_wkb(), "id": pa.array(np.arange(len(pts)))})
    rhs = pa.table({"geometry": polys.to_arrow_wkb(), "name": pa.array(["poly-%d" % i for i in range(len(polys))])})
    pairs, counts = join_pairs(GeoSeries(pts), GeoSeries(polys), "intersects")
    li, ri = join_indices(counts, pairs, join_type)
    assert len(li) > 0 and ((ri < 0).any() == (join_type == "left"))
    native = spatial_join(lhs, rhs, SpatialJoinArgs(join_type=join_type, geometry_encoding="geoarrow"))
    plain = spatial_join(lhs, rhs, SpatialJoinArgs(join_type=join_type))
    assert native.column_names == plain.column_names == ["geometry_left", "id_left", "geometry_right", "name_right"]
    gl = DeviceGeoArray.from_arrow(native.column("geometry_left"), _abi.GEOM_POINT).download()
    gr = DeviceGeoArray.from_arrow(native.column("geometry_right"), _abi.GEOM_POLYGON).download()
    K.assert_same(gl, K.expected_take(pts, li), "left geometry")
    want_r = K.expected_take(polys, ri)
    assert np.array_equal(gr.is_valid(), want_r.is_valid()) and np.array_equal(gr.is_valid(), ri >= 0)
    K.assert_same(gr, want_r, "right geometry")
    for name in ("id_left", "name_right"):
        assert native.column(name).equals(plain.column(name))
    # the default encoding returns what it returned before: WKB, equal to pyarrow's take of the input column
    assert pa.types.is_binary(plain.column("geometry_left").type)
    assert plain.column("geometry_left").combine_chunks().equals(lhs.column("geometry").combine_chunks().take(pa.array(li)))
    valid_r = plain.column("geometry_right").combine_chunks().take(pa.array(np.nonzero(ri >= 0)[0]))
    assert valid_r.equals(rhs.column("geometry").combine_chunks().take(pa.array(ri[ri >= 0])))
