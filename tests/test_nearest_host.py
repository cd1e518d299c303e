"""Nearest-neighbour join, host side: argument checks that refuse a call before any device is touched, the options' defaults, and
the C ABI symbol."""
import math

import pytest

from geopolars_amd import _abi, spatial_index
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import SpatialJoinNearestArgs, nearest_pairs, spatial_join_nearest
from tests.host_build import no_device  # noqa: F401  (no_device: a fixture)


def test_exported_symbols_name_the_nearest_join():
    assert "gpk_nearest_join" in _abi.EXPORTED_SYMBOLS
    restype, argtypes = _abi._PROTOS["gpk_nearest_join"]
    assert len(argtypes) == 12


def test_nearest_args_defaults():
    a = SpatialJoinNearestArgs()
    assert a.join_type == "inner" and a.max_distance is None and a.distance_col is None
    assert a.l_suffix == "_left" and a.r_suffix == "_right" and a.r_index is None
    assert a.l_geom_type == -1 and a.r_geom_type == -1


def _series():
    pts = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0]]))
    lines = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)]]))
    return pts, lines


@pytest.mark.parametrize("md", [-1.0, -0.0 - 1e-300, math.nan])
def test_bad_max_distance_is_refused_before_the_device(no_device, md):
    pts, lines = _series()
    with pytest.raises(_abi.GeopolarsHipError) as e:
        nearest_pairs(pts, lines, max_distance=md)
    assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    assert pts._dev is None and lines._dev is None


def test_non_point_left_side_is_refused_before_the_device(no_device):
    pts, lines = _series()
    with pytest.raises(_abi.MismatchedGeometry):
        nearest_pairs(lines, pts)
    assert pts._dev is None and lines._dev is None


def test_table_join_checks_its_options_first(no_device):
    pa = pytest.importorskip("pyarrow")
    t = pa.table({"id": pa.array([0]), "geometry": pa.array([b"\x00"], type=pa.binary())})
    with pytest.raises(_abi.GeopolarsHipError) as e:
        spatial_join_nearest(t, t, SpatialJoinNearestArgs(join_type="outer"))
    assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    for md in (-2.0, math.nan):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            spatial_join_nearest(t, t, SpatialJoinNearestArgs(max_distance=md))
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT


def test_zero_and_infinite_max_distance_are_accepted():
    assert spatial_index._max_distance_arg(None) == math.inf
    assert spatial_index._max_distance_arg(0.0) == 0.0
    assert spatial_index._max_distance_arg(math.inf) == math.inf
