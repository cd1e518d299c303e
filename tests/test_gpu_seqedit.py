"""gpk_segmentize / gpk_remove_repeated_points / gpk_reverse / gpk_orient_polygons on the GPU (csrc/gpk_seqedit.hip) against the plain
Python of tests/seqedit_ref.py: every comparison is exact — offsets level by level, is_valid(), whether there is a bitmap at all, the
coordinates bit for bit.  The hand-built shapes sit on the strip of 1024 coordinates of the count passes and the fills."""
import ctypes as C

import numpy as np
import pytest

from geopolars_amd import _abi, synth
from geopolars_amd.geoarrow import DeviceGeoArray, GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from tests import geotake_cases as K
from tests import seqedit_ref as R
from tests.second_pass import same_bits

pytestmark = pytest.mark.gpu

COLUMNS = K.columns()
DEVICE_OPS = {
    "segmentize": lambda d: d.segmentize(7.5),
    "remove_repeated_points": lambda d: d.remove_repeated_points(),
    "reverse": lambda d: d.reverse(),
    "orient_polygons": lambda d: d.orient_polygons(),
    "orient_polygons cw": lambda d: d.orient_polygons(True),
}


def _on_device(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _check(got: DeviceGeoArray, want: GeoArrowArray, what):
    assert (got.n_geoms, got.n_coords) == (len(want), want.n_coords), what
    K.assert_same(got.download(), want, what)


def _all_ops(host: GeoArrowArray, what):
    dev = DeviceGeoArray.upload(host)
    for op, call in DEVICE_OPS.items():
        _check(call(dev), R.OPS[op](host), (what, op))


@pytest.fixture(scope="module")
def synth_20k():
    """20 000 polygons, some rings reversed, some coordinates repeated; the reference results, computed once"""
    base = synth.clustered_polygons(20_000, seed=17)
    flip = np.random.default_rng(3).uniform(size=base.n_rings) < 0.5
    host = _with_repeats(R.reverse(base, flip), seed=4)
    seglen = np.hypot(*np.diff(host.xy, axis=0).T)
    m = float(np.median(seglen[seglen > 0]))
    want = {"segmentize": R.segmentize(host, m), "remove_repeated_points": R.remove_repeated_points(host), "reverse": R.reverse(host),
            "orient_polygons": R.orient_polygons(host), "orient_polygons cw": R.orient_polygons(host, True)}
    return host, m, want


def _with_repeats(a: GeoArrowArray, seed: int, p: float = 0.1) -> GeoArrowArray:
    """`a` with a tenth of its coordinates doubled or tripled in place (every level above the sequences unchanged)"""
    rng = np.random.default_rng(seed)
    times = np.where(rng.uniform(size=a.n_coords) < p, rng.integers(2, 4, a.n_coords), 1)
    off = R._levels(a)[-1][1].astype(np.int64)
    before = np.concatenate([[0], np.cumsum(times)])
    return R._rebuilt(a, before[off], np.repeat(a.xy, times, axis=0))


# ---- every type, every operation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(COLUMNS))
def test_every_operation_on_every_type(gpk, name):
    """null rows, empty rows, parts without rings, sequences of one coordinate, NaN payloads and signed zeros; POINT and MULTIPOINT
    columns come back bit for bit"""
    _all_ops(COLUMNS[name], name)


@pytest.mark.parametrize("name", list(K.edge_columns()))
def test_every_operation_on_the_empty_runs(gpk, name):
    _all_ops(K.edge_columns()[name], name)


def test_every_operation_on_columns_without_rows(gpk):
    for name in ("point", "linestring", "multipolygon+nulls"):
        host = COLUMNS[name]
        none = DeviceGeoArray.upload(host).take(np.zeros(0, np.int64))
        want = host.take(np.zeros(0, np.int64))
        for op, call in DEVICE_OPS.items():
            _check(call(none), want, (name, op))


# ---- segmentize ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.segmentize_cases()))
def test_segmentize_at_the_strip_size(gpk, name):
    host, m = R.segmentize_cases()[name]
    want = R.segmentize(host, m)
    _check(DeviceGeoArray.upload(host).segmentize(m), want, name)
    if name == "m larger than every segment":
        assert same_bits(want.xy, host.xy)
    if name == "sequence boundary at the strip boundary":
        assert want.ring_offsets[1] == R.STRIP


@pytest.mark.parametrize("name", ["linestring", "polygon", "multilinestring", "multipolygon+nulls", "point"])
def test_segmentize_per_row_from_host_and_device(gpk, name):
    host = COLUMNS[name]
    per_row = np.random.default_rng(len(name)).uniform(1.0, 30.0, len(host))
    per_row[::5], per_row[1::7], per_row[2::9] = np.nan, 0.0, -3.0
    want = R.segmentize(host, per_row)
    dev = DeviceGeoArray.upload(host)
    _check(dev.segmentize(per_row), want, (name, "host"))
    _check(dev.segmentize(_on_device(per_row)), want, (name, "device"))
    _check(GeoSeries(host).segmentize(list(per_row)).device(), want, (name, "GeoSeries"))


def test_segmentize_overflow_is_a_clean_error(gpk):
    """one segment of 1e10 pieces: GPK_ERR_INVALID_ARGUMENT, *out untouched, and the next call works"""
    dev = DeviceGeoArray.upload(R.linestrings([[(0, 0), (1e10, 0)], [(0, 0), (3, 0)]]))
    out = C.c_void_p(7)
    rc = _abi.lib().gpk_segmentize(dev.handle, 1.0, None, _abi.MEM_HOST, None, C.byref(out))
    assert rc == _abi.GPK_ERR_INVALID_ARGUMENT and "2^31 - 1" in _abi.last_error() and out.value == 7
    with pytest.raises(_abi.GeopolarsHipError) as e:
        dev.segmentize(1.0)
    assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    host = R.linestrings([[(0, 0), (10, 0)]])
    _check(DeviceGeoArray.upload(host).segmentize(1.0), R.segmentize(host, 1.0), "after the refusal")
    # 2^31 pieces of one segment and 2^31 of the next: the sum is carried in 64 bits
    two = DeviceGeoArray.upload(R.linestrings([[(0, 0), (3e9, 0), (3e9, 3e9)]]))
    assert _abi.lib().gpk_segmentize(two.handle, 1.0, None, _abi.MEM_HOST, None, C.byref(out)) == _abi.GPK_ERR_INVALID_ARGUMENT and out.value == 7


# ---- remove_repeated_points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.dedup_cases()))
def test_remove_repeated_points_cases(gpk, name):
    host = R.dedup_cases()[name]
    want = R.remove_repeated_points(host)
    _check(DeviceGeoArray.upload(host).remove_repeated_points(), want, name)
    if name == "no repeats":
        assert same_bits(want.xy, host.xy)
    if name == "no coordinates":
        assert want.n_coords == 0


# ---- reverse -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.reverse_cases()))
def test_reverse_cases(gpk, name):
    host = R.reverse_cases()[name]
    dev = DeviceGeoArray.upload(host)
    once = dev.reverse()
    _check(once, R.reverse(host), name)
    _check(once.reverse(), host, (name, "twice"))
    if name == "closed rings":
        got = once.download()
        assert same_bits(got.xy[got.ring_offsets[:-1]], got.xy[got.ring_offsets[1:] - 1])


# ---- orient_polygons -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.orient_cases()))
def test_orient_cases(gpk, name):
    host = R.orient_cases()[name]
    dev = DeviceGeoArray.upload(host)
    for cw in (False, True):
        _check(dev.orient_polygons(cw), R.orient_polygons(host, cw), (name, cw))
    if name in ("spike", "NaN ring", "inf closing"):
        assert same_bits(dev.orient_polygons().download().xy, host.xy)


@pytest.mark.parametrize("name", ["squares and holes both ways", "smallest repeated", "spike", "3-coordinate ring", "unclosed"])
def test_orient_decisions_do_not_depend_on_the_placement(gpk, name):
    """integer coordinates moved by 2^30 and 2^31 (exact): the same rings are reversed"""
    host = R.orient_cases()[name]
    moved = GeoArrowArray(host.geom_type, host.xy + np.array([2.0**30, -(2.0**31)]), host.geom_offsets, ring_offsets=host.ring_offsets)
    assert np.array_equal(moved.xy - np.array([2.0**30, -(2.0**31)]), host.xy)
    for cw in (False, True):
        _check(DeviceGeoArray.upload(moved).orient_polygons(cw), R.reverse(moved, R.orient_decisions(host, cw)), (name, cw))


def _shells(a: GeoArrowArray) -> GeoArrowArray:
    """the first ring of every non-empty polygon of a POLYGON column as a column of single-ring polygons"""
    first = a.geom_offsets[:-1][np.diff(a.geom_offsets) > 0]
    return R.polygons([1] * len(first), [a.xy[a.ring_offsets[r]:a.ring_offsets[r + 1]] for r in first])


def test_oriented_shells_have_positive_signed_area(gpk):
    """agreement with the library itself: for every row gpk_validity calls valid, signed_area of the oriented shell is > 0 (and < 0
    with exterior_cw)"""
    base = synth.clustered_polygons(300, seed=23)
    host = _shells(R.reverse(base, np.random.default_rng(5).uniform(size=base.n_rings) < 0.5))
    s = GeoSeries(host)
    valid = s.is_valid()
    assert valid.sum() > 100 and (s.signed_area()[valid] < 0).any() and (s.signed_area()[valid] > 0).any()
    assert (s.orient_polygons().signed_area()[valid] > 0).all()
    assert (s.orient_polygons(exterior_cw=True).signed_area()[valid] < 0).all()


def _median_segment(a: GeoArrowArray) -> float:
    seglen = np.hypot(*np.diff(a.xy, axis=0).T)
    return float(np.median(seglen[seglen > 0]))


# ---- composition with the operators that exist ---------------------------------------------------------------------------------------------
def test_segmentize_keeps_length_and_area(gpk):
    lines = GeoSeries(synth.random_linestrings(300, seed=13))
    length = lines.euclidean_length()
    dense = lines.segmentize(_median_segment(lines.array) / 4)
    assert dense.device().n_coords > 2 * lines.array.n_coords
    assert np.all(np.abs(dense.euclidean_length() - length) <= 1e-12 * length)
    polys = GeoSeries(synth.clustered_polygons(300, seed=14))
    area = polys.area()
    dense = polys.segmentize(_median_segment(polys.array) / 4)
    assert dense.device().n_coords > 2 * polys.array.n_coords
    assert np.all(np.abs(dense.area() - area) <= 1e-9 * area)


def test_remove_repeated_points_and_validity(gpk):
    """gpk_validity drops zero-length segments, so repeated coordinates alone are no fault and the library has no reason code of their
    own: the codes of a valid column are the same with the repeats and without them, and removing them gives back the column bit for
    bit"""
    base = synth.clustered_polygons(300, seed=15)
    doubled = _with_repeats(base, seed=6)
    assert doubled.n_coords > base.n_coords + 300
    before = GeoSeries(base).is_valid_reason()
    assert (before == 0).sum() > 100
    cleaned = GeoSeries(doubled).remove_repeated_points()
    K.assert_same(cleaned.array, base, "repeats removed")
    assert np.array_equal(GeoSeries(doubled).is_valid_reason(), before) and np.array_equal(cleaned.is_valid_reason(), before)


def test_triangulate_reports_the_same_status_after_orient(gpk):
    base = synth.clustered_polygons(300, seed=16)
    host = R.reverse(base, np.random.default_rng(7).uniform(size=base.n_rings) < 0.5)
    s = GeoSeries(host)
    status = s.triangulate(return_status=True)[-1]
    assert (status == 0).sum() > 100
    assert np.array_equal(s.orient_polygons().triangulate(return_status=True)[-1], status)


# ---- at a moderate size, in full -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", list(DEVICE_OPS))
def test_20000_polygons_compared_in_full(gpk, synth_20k, op):
    host, m, want = synth_20k
    dev = DeviceGeoArray.upload(host)
    got = dev.segmentize(m) if op == "segmentize" else DEVICE_OPS[op](dev)
    _check(got, want[op], op)


# ---- ownership -----------------------------------------------------------------------------------------------------------------------------
def test_a_result_outlives_its_source(gpk):
    host = COLUMNS["multipolygon+nulls"]
    dev = DeviceGeoArray.upload(host)
    results = {op: call(dev) for op, call in DEVICE_OPS.items()}
    dev.free()
    again = results["reverse"].reverse()
    results["reverse"].free()
    for op, got in results.items():
        if op != "reverse":
            _check(got, R.OPS[op](host), op)
    _check(again, host, "reverse of a freed reverse")


def test_a_source_that_is_a_zero_copy_view_of_device_buffers(gpk):
    host = COLUMNS["polygon"]
    tensors = {k: _on_device(getattr(host, k)) for k in ("geom_offsets", "ring_offsets")}
    view = DeviceGeoArray.from_device_buffers(host.geom_type, _on_device(host.xy), **tensors)
    for op, call in DEVICE_OPS.items():
        _check(call(view), R.OPS[op](host), ("device view", op))


def test_geoseries_methods_return_device_resident_series(gpk):
    host = COLUMNS["polygon"]
    s = GeoSeries(host)
    for got, want in ((s.segmentize(7.5), R.segmentize(host, 7.5)), (s.segmentize(np.float32(7.5)), R.segmentize(host, 7.5)),
                      (s.remove_repeated_points(), R.remove_repeated_points(host)), (s.remove_repeated_points(tolerance=0), R.remove_repeated_points(host)),
                      (s.reverse(), R.reverse(host)), (s.orient_polygons(), R.orient_polygons(host)),
                      (s.orient_polygons(exterior_cw=True), R.orient_polygons(host, True))):
        assert got._array is None and got._dev is not None and len(got) == len(want)
        K.assert_same(got.array, want)
