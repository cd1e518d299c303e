"""Any-family nearest join (gpk_nearest_join_any), host side: the argument checks that refuse a call before the library is opened, the C
ABI symbol, the seed walk's rule (csrc/gpk_nearwalk.h) run on the CPU by a stand-alone program against a brute-force minimum — plain
and under AddressSanitizer + UBSan — and the condition on the fixtures of the exact-reference GPU test."""
import math
import os
import subprocess

import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import (
    SpatialJoinNearestArgs,
    nearest_pairs,
    nearest_pairs_any,
    nearest_pairs_any_device,
    nearest_pairs_device,
    spatial_join_nearest,
)
from tests import nearest_any_ref as N
from tests.host_build import build_host_drivers, exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_documented():
    assert "gpk_nearest_join_any" in _abi.EXPORTED_SYMBOLS and len(_abi._PROTOS["gpk_nearest_join_any"][1]) == 12
    assert _abi._PROTOS["gpk_nearest_join_any"] == _abi._PROTOS["gpk_nearest_join"]
    assert "gpk_nearest_join_any" in exported_symbols()
    flat = " ".join(open(os.path.join(ROOT, "include", "geopolars_hip.h")).read().split())
    assert ("int32_t gpk_nearest_join_any(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, double max_distance, "
            "uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, double* out_dist, int64_t pair_capacity, int64_t* n_pairs, "
            "int32_t out_space, void* stream);") in flat
    for line in ("all 36 ordered pairs", "byte for byte those of gpk_nearest_join", "two calls give identical bytes"):
        assert line in flat, line
    assert "gpk_nearest_join_any" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---- Python: refusals before the library is opened ----------------------------------------------------------------------------------
def _series():
    pts = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0]]))
    lines = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)]]))
    return pts, lines


class _Dev:
    """what nearest_pairs_any_device reads of a DeviceGeoArray before it makes the call"""

    def __init__(self, geom_type):
        self.geom_type = geom_type


GEOMETRYCOLLECTION = 7  # (the WKB code: no column of this library holds one)


class _Column:
    """a series of a family the library has no column for, as far as nearest_pairs_any looks before it refuses"""

    def __init__(self, geom_type):
        self._t, self._dev = geom_type, None

    def _family(self):
        return self._t


@pytest.mark.parametrize("md", [-1.0, -1e-300, math.nan, -math.inf])
def test_bad_max_distance_is_refused_before_any_upload(no_device, md):
    pts, lines = _series()
    for call in (lambda: nearest_pairs_any(lines, pts, max_distance=md), lambda: nearest_pairs_any(pts, lines, max_distance=md),
                 lambda: nearest_pairs_any_device(_Dev(_abi.GEOM_LINESTRING), _Dev(_abi.GEOM_POINT), None, None, None, max_distance=md)):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            call()
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    assert pts._dev is None and lines._dev is None


def test_unsupported_families_are_refused_before_any_upload(no_device):
    pts, lines = _series()
    other = _Column(GEOMETRYCOLLECTION)
    for call in (lambda: nearest_pairs_any(other, pts), lambda: nearest_pairs_any(lines, other),
                 lambda: nearest_pairs_any_device(_Dev(GEOMETRYCOLLECTION), _Dev(_abi.GEOM_POINT), None, None, None),
                 lambda: nearest_pairs_any_device(_Dev(_abi.GEOM_POLYGON), _Dev(99), None, None, None)):
        with pytest.raises(_abi.MismatchedGeometry) as e:
            call()
        assert e.value.code == _abi.GPK_ERR_MISMATCHED_GEOMETRY
    assert pts._dev is None and lines._dev is None and other._dev is None


def test_the_point_entry_points_keep_refusing_other_left_sides(no_device):
    pts, lines = _series()
    with pytest.raises(_abi.MismatchedGeometry):
        nearest_pairs(lines, pts)
    with pytest.raises(_abi.MismatchedGeometry):
        nearest_pairs_device(_Dev(_abi.GEOM_LINESTRING), _Dev(_abi.GEOM_POINT), None, None, None)
    assert pts._dev is None and lines._dev is None


def test_table_join_still_checks_its_options_first(no_device):
    pa = pytest.importorskip("pyarrow")
    t = pa.table({"id": pa.array([0]), "geometry": pa.array([b"\x00"], type=pa.binary())})
    with pytest.raises(_abi.GeopolarsHipError) as e:
        spatial_join_nearest(t, t, SpatialJoinNearestArgs(join_type="outer"))
    assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    for md in (-2.0, math.nan):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            spatial_join_nearest(t, t, SpatialJoinNearestArgs(max_distance=md))
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT


# ---- the walk's rule on the CPU -------------------------------------------------------------------------------------------------------
CASES = ["grid_1x1", "grid_7x5", "lattice_borders", "zero_width_axis", "zero_extent", "left_outside", "left_covers_extent", "left_3x2_cells", "right_spans_cells",
         "right_spans_cells_sparse"]


@pytest.mark.parametrize("name", ["plain", "sanitized"], ids=["plain-extra0", "sanitized-extra1"])  # (the ids these cases have had)
def test_seed_walk_finds_the_nearest_box(tmp_path_factory, name):
    """tests/nearwalk_host_driver.cpp, a stand-alone executable built with the host compiler (nothing is preloaded, nothing is loaded
    into Python): per grid case, a few hundred left boxes whose seed must be the brute-force nearest box — same row, same distance bits"""
    built, _ = build_host_drivers(tmp_path_factory, "nearwalk", fp_contract_off=True, builds=(name,))
    r = subprocess.run([built[name]], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [ln[0] for ln in lines] == CASES
    for case, n_left, seeded, bad in lines:
        assert int(n_left) >= 300 and int(bad) == 0 and 0 < int(seeded) <= int(n_left), (case, n_left, seeded, bad)
    # every bound of the driver refuses some rows somewhere, and the all-covering cases seed every row
    assert any(int(s) < int(n) for _, n, s, _ in lines) and all(int(s) == int(n) for c, n, s, _ in lines if c in ("left_covers_extent", "left_3x2_cells"))


# ---- the fixtures of the exact-reference GPU test ------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["point", "g8", "g32", "large"])
def test_fixtures_leave_few_rows_undecided(group):
    """at most 5 % of the usable left rows of every fixture have an exact runner-up within 1e-6 relative of an unshared exact best"""
    keys = [(k, s) for k, s in N.EXACT_FIXTURES if (k[2] if not isinstance(k[0], str) else "point") == group]
    assert len(keys) >= 25
    for key, seed in keys:
        left, _ = N.fixture(key, seed)
        rows = N.exact_nearest(N.fixture_table(key, seed), len(left[1]))
        assert len(rows) >= 2, key
        undecided = [l for l, (_, _, decided, _) in rows.items() if not decided]
        assert len(undecided) <= N.MAX_UNDECIDED * len(rows), (key, undecided, len(rows))
