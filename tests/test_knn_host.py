"""k-nearest-neighbours join (gpk_knn_join), host side: the C ABI symbol, the argument checks that refuse a call before the library is
opened, the k-seed walk's rule (csrc/gpk_knnwalk.h) run on the CPU by a stand-alone program against brute force — plain and under
AddressSanitizer + UBSan — and the condition on the fixtures of the exact-reference GPU test."""
import math
import os
import subprocess

import pytest

from geopolars_amd import _abi
from geopolars_amd.spatial_index import SpatialJoinKnnArgs, knn_pairs, knn_pairs_device, spatial_join_knn
from tests import knn_ref as K
from tests import nearest_any_ref as N
from tests.host_build import build_host_drivers, exported_symbols, no_device  # noqa: F401  (no_device: a fixture)
from tests.test_nearest_any_host import GEOMETRYCOLLECTION, _Column, _Dev, _series

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_documented():
    assert "gpk_knn_join" in _abi.EXPORTED_SYMBOLS and len(_abi._PROTOS["gpk_knn_join"][1]) == 14
    assert _abi.GPK_KNN_MAX_K == 64 and _abi.GPK_KNN_EXCLUDE_SELF == 1
    assert "gpk_knn_join" in exported_symbols()
    flat = " ".join(open(os.path.join(ROOT, "include", "geopolars_hip.h")).read().split())
    assert ("int32_t gpk_knn_join(const gpk_geoarray* left, const gpk_geoarray* right, const gpk_index* right_index, int32_t k, double max_distance, "
            "uint32_t flags, uint32_t left_row_base, uint32_t* out_counts, uint32_t* out_pairs, double* out_dist, int64_t pair_capacity, "
            "int64_t* n_pairs, int32_t out_space, void* stream);") in flat
    for line in ("#define GPK_KNN_MAX_K 64", "#define GPK_KNN_EXCLUDE_SELF 1u", "all 36 ordered pairs", "sorted by (l, d, r)",
                 "goes to the lower right row", "live in LDS"):
        assert line in flat, line
    assert "gpk_knn_join" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---- Python: refusals before the library is opened ----------------------------------------------------------------------------------
def _refused(call, code=_abi.GPK_ERR_INVALID_ARGUMENT, exc=_abi.GeopolarsHipError):
    with pytest.raises(exc) as e:
        call()
    assert e.value.code == code


@pytest.mark.parametrize("k", [0, -1, 65, 2.5, None, True])
def test_bad_k_is_refused_before_any_upload(no_device, k):
    pts, lines = _series()
    _refused(lambda: knn_pairs(lines, pts, k))
    _refused(lambda: knn_pairs(pts, lines, k, exclude_self=True))
    _refused(lambda: knn_pairs_device(_Dev(_abi.GEOM_LINESTRING), _Dev(_abi.GEOM_POINT), None, k, None, None))
    assert pts._dev is None and lines._dev is None


@pytest.mark.parametrize("md", [-1.0, -1e-300, math.nan, -math.inf])
def test_bad_max_distance_is_refused_before_any_upload(no_device, md):
    pts, lines = _series()
    _refused(lambda: knn_pairs(lines, pts, 3, max_distance=md))
    _refused(lambda: knn_pairs_device(_Dev(_abi.GEOM_LINESTRING), _Dev(_abi.GEOM_POINT), None, 3, None, None, max_distance=md))
    assert pts._dev is None and lines._dev is None


def test_unsupported_families_are_refused_before_any_upload(no_device):
    pts, lines = _series()
    other = _Column(GEOMETRYCOLLECTION)
    for call in (lambda: knn_pairs(other, pts, 2), lambda: knn_pairs(lines, other, 2),
                 lambda: knn_pairs_device(_Dev(GEOMETRYCOLLECTION), _Dev(_abi.GEOM_POINT), None, 2, None, None),
                 lambda: knn_pairs_device(_Dev(_abi.GEOM_POLYGON), _Dev(99), None, 2, None, None)):
        _refused(call, _abi.GPK_ERR_MISMATCHED_GEOMETRY, _abi.MismatchedGeometry)
    assert pts._dev is None and lines._dev is None and other._dev is None


def test_table_join_checks_its_options_first(no_device):
    pa = pytest.importorskip("pyarrow")
    t = pa.table({"id": pa.array([0]), "geometry": pa.array([b"\x00"], type=pa.binary())})
    for bad in (SpatialJoinKnnArgs(join_type="outer"), SpatialJoinKnnArgs(k=0), SpatialJoinKnnArgs(k=65), SpatialJoinKnnArgs(k=2, max_distance=-2.0),
                SpatialJoinKnnArgs(k=2, max_distance=math.nan)):
        _refused(lambda: spatial_join_knn(t, t, bad))


# ---- the walk's rule on the CPU -------------------------------------------------------------------------------------------------------
CASES = ["grid_1x1", "grid_7x5", "grid_23x19", "lattice_points", "long_boxes", "zero_width_axis", "zero_extent", "left_outside", "left_spans_cells",
         "few_rights"]


@pytest.mark.parametrize("name", ["plain", "sanitized"], ids=["plain-extra0", "sanitized-extra1"])  # (the ids these cases have had)
def test_k_seed_walk_finds_the_k_lowest_keys(tmp_path_factory, name):
    """tests/knnwalk_host_driver.cpp, a stand-alone executable built with the host compiler (nothing is preloaded, nothing is loaded
    into Python): per grid case, 360 left boxes whose K slots must be the brute-force K lowest (far distance, row) keys within max_d —
    same rows, same distance bits, no row twice"""
    built, _ = build_host_drivers(tmp_path_factory, "knnwalk", fp_contract_off=True, builds=(name,))
    r = subprocess.run([built[name]], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [ln[0] for ln in lines] == CASES
    for case, n_left, full, fewer, bad in lines:
        # every case fills some lists and leaves some short (max_d, or K above the usable rows)
        assert int(n_left) >= 300 and int(bad) == 0 and int(full) > 0 and int(fewer) > 0 and int(full) + int(fewer) == int(n_left), (case, full, fewer, bad)


# ---- the fixtures of the exact-reference GPU test ------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["point", "pair"])
def test_fixtures_leave_few_rows_undecided(group):
    """over the point fixtures together and over the pair fixtures together, at k = 2, 3 and 5: at most 10 % of the left rows with more
    than k usable partners are undecided"""
    keys = [(key, seed) for key, seed in N.EXACT_FIXTURES if isinstance(key[0], str) == (group == "point")]
    assert len(keys) >= 10
    for k in (2, 3, 5):
        undecided = total = 0
        for key, seed in keys:
            table = N.fixture_table(key, seed)
            rows, many = K.exact_knn(table, k), K.more_than_k(table, k)
            assert all(decided for l, (_, decided) in rows.items() if l not in many)
            undecided += sum(1 for l in many if not rows[l][1])
            total += len(many)
        print(group, k, undecided, total)
        assert total >= 300 and undecided <= K.MAX_UNDECIDED * total, (group, k, undecided, total)
