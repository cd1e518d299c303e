"""Within-distance join, host side: the C ABI symbols (prototypes and the built library), the options' defaults, and the argument
checks that refuse a call before the library is opened."""
import math
import os

import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries, dwithin_distance_arg
from geopolars_amd.spatial_index import SpatialJoinDWithinArgs, dwithin_pairs, dwithin_pairs_device, spatial_join_dwithin
from tests.host_build import exported_symbols, no_device  # noqa: F401  (no_device: a fixture)


def test_exported_symbols_name_the_dwithin_calls():
    assert "gpk_dwithin_join" in _abi.EXPORTED_SYMBOLS and "gpk_dwithin_rowwise" in _abi.EXPORTED_SYMBOLS
    assert len(_abi._PROTOS["gpk_dwithin_join"][1]) == 12
    assert len(_abi._PROTOS["gpk_dwithin_rowwise"][1]) == 7
    assert "dwithin" not in _abi.PREDICATES  # gpk_spatial_join's predicate codes stay as they are


def test_built_library_exports_the_dwithin_calls():
    from geopolars_amd import build

    assert {"gpk_dwithin_join", "gpk_dwithin_rowwise"} <= exported_symbols()
    assert os.path.samefile(build.build(), _abi.LIB_PATH) or os.environ.get("GPK_LIB_PATH")


def test_dwithin_args_defaults():
    a = SpatialJoinDWithinArgs()
    assert a.distance is None and a.join_type == "inner" and a.distance_col is None
    assert a.l_suffix == "_left" and a.r_suffix == "_right" and a.r_index is None
    assert a.l_geom_type == -1 and a.r_geom_type == -1


def _series():
    pts = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0]]))
    lines = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)]]))
    return pts, lines


BAD = [-1.0, -1e-300, math.nan, math.inf, -math.inf, None, "near"]


@pytest.mark.parametrize("d", BAD)
def test_bad_distance_is_refused_before_the_device(no_device, d):
    pts, lines = _series()
    for call in (lambda: dwithin_pairs(lines, pts, d), lambda: lines.dwithin(pts, d), lambda: dwithin_pairs_device(None, None, None, d, None, None)):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            call()
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    assert pts._dev is None and lines._dev is None


def test_table_join_checks_its_options_first(no_device):
    pa = pytest.importorskip("pyarrow")
    t = pa.table({"id": pa.array([0]), "geometry": pa.array([b"\x00"], type=pa.binary())})
    with pytest.raises(_abi.GeopolarsHipError) as e:
        spatial_join_dwithin(t, t, SpatialJoinDWithinArgs(distance=1.0, join_type="outer"))
    assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    for d in BAD:
        with pytest.raises(_abi.GeopolarsHipError) as e:
            spatial_join_dwithin(t, t, SpatialJoinDWithinArgs(distance=d))
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    with pytest.raises(_abi.GeopolarsHipError):  # `distance` is required
        spatial_join_dwithin(t, t)


def test_zero_and_finite_distances_are_accepted():
    assert dwithin_distance_arg(0) == 0.0 and dwithin_distance_arg(0.0) == 0.0
    assert dwithin_distance_arg(2.5) == 2.5 and dwithin_distance_arg(1e300) == 1e300
