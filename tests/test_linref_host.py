"""Linear referencing, host side: the C ABI symbols and the argument checks that refuse a call before any device is touched."""
import math

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries, interpolate_distance_arg
from tests.host_build import no_device  # noqa: F401  (no_device: a fixture)


@pytest.mark.parametrize("name,n_args", [("gpk_closest_point_rowwise", 7), ("gpk_line_locate_point", 7), ("gpk_line_interpolate_point", 8)])
def test_exported_symbols_name_the_linear_referencing_calls(name, n_args):
    assert name in _abi.EXPORTED_SYMBOLS
    restype, argtypes = _abi._PROTOS[name]
    assert len(argtypes) == n_args


def _series():
    pts = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0]]))
    lines = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)], [(0.0, 0.0), (2.0, 0.0)]]))
    polys = GeoSeries(GeoArrowArray.from_polygons([[[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0)]], [[(0.0, 0.0), (2.0, 0.0), (2.0, 2.0)]]]))
    return pts, lines, polys


def _untouched(*series):
    return all(s._dev is None for s in series)


def test_wrong_families_raise_mismatched_geometry_before_the_device(no_device):
    pts, lines, polys = _series()
    with pytest.raises(_abi.MismatchedGeometry):
        lines.closest_point(pts)  # the POINT column comes first
    with pytest.raises(_abi.MismatchedGeometry):
        polys.closest_point(lines)
    with pytest.raises(_abi.MismatchedGeometry):
        lines.shortest_line(polys)
    with pytest.raises(_abi.MismatchedGeometry):
        polys.project(pts)  # project needs a lineal column ...
    with pytest.raises(_abi.MismatchedGeometry):
        pts.project(pts)
    with pytest.raises(_abi.MismatchedGeometry):
        lines.project(lines)  # ... and points to locate
    with pytest.raises(_abi.MismatchedGeometry):
        polys.interpolate(1.0)
    with pytest.raises(_abi.MismatchedGeometry):
        pts.interpolate(1.0)
    assert _untouched(pts, lines, polys)


def test_row_counts_and_row_maps_are_checked_before_the_device(no_device):
    pts, lines, polys = _series()
    one = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)]]))
    for call in (lambda: pts.closest_point(one), lambda: one.project(pts), lambda: pts.closest_point(lines, other_rows=[0]),
                 lambda: lines.project(pts, rows=[0, 1, 0]), lambda: pts.closest_point(lines, other_rows=[[0, 1]]),
                 lambda: pts.closest_point(lines, other_rows=["a", "b"])):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            call()
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    assert _untouched(pts, lines, one)


@pytest.mark.parametrize("bad", [[1.0], [1.0, 2.0, 3.0], [[1.0, 2.0]], "far", None, [1.0, "x"], object()])
def test_bad_interpolate_distances_are_refused_before_the_device(no_device, bad):
    pts, lines, polys = _series()
    with pytest.raises(_abi.GeopolarsHipError) as e:
        lines.interpolate(bad)
    assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    assert _untouched(lines)


def test_interpolate_distance_forms():
    pts, lines, polys = _series()
    d = interpolate_distance_arg(lines, 2)
    assert d.dtype == np.float64 and d.shape == (1,) and d[0] == 2.0  # a scalar stays one value: it is not expanded to n
    d = interpolate_distance_arg(lines, np.float32(0.5))
    assert d.shape == (1,) and d[0] == 0.5
    d = interpolate_distance_arg(lines, [1, -2])
    assert d.dtype == np.float64 and d.tolist() == [1.0, -2.0]
    assert math.isnan(interpolate_distance_arg(lines, math.nan)[0])  # NaN is a value: the row comes back null
    assert interpolate_distance_arg(lines, (0.25, math.inf)).tolist() == [0.25, math.inf]
