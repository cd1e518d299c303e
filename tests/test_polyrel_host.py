"""Polygon x polygon relations, host side: the C ABI symbols, the header's bits and ids, the mask -> predicate table for all 16 masks,
the argument checks that refuse a call before the library is opened, and the older surfaces that must not move."""
import os
import re

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import MASK_PREDICATES, POLYGON_MASK_PREDICATES, GeoSeries, mask_predicate, polygon_mask_predicate
from geopolars_amd.spatial_index import (
    POLYGON_RELATION_PREDICATES,
    RELATION_PREDICATES,
    SpatialJoinRelationArgs,
    polygon_relation_pairs,
    polygon_relation_pairs_device,
    polygon_relation_predicate_arg,
    relation_pairs,
    spatial_join_polygon_relation,
)
from tests.host_build import exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

LS, PG, MPG, PT = _abi.GEOM_LINESTRING, _abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON, _abi.GEOM_POINT


def test_exported_symbols_name_the_polygon_relation_calls():
    assert "gpk_polygon_relation" in _abi.EXPORTED_SYMBOLS and "gpk_polygon_relation_join" in _abi.EXPORTED_SYMBOLS
    assert len(_abi._PROTOS["gpk_polygon_relation"][1]) == 6
    assert len(_abi._PROTOS["gpk_polygon_relation_join"][1]) == 12
    assert (_abi.PP_INTERIORS, _abi.PP_BOUNDARIES, _abi.PP_A_OUTSIDE, _abi.PP_B_OUTSIDE) == (1, 2, 4, 8)
    assert set(_abi.PREDICATES) == {"intersects", "contains", "within"}  # gpk_spatial_join's predicate codes stay as they are


def test_built_library_exports_the_polygon_relation_calls():
    names = exported_symbols()
    assert {"gpk_polygon_relation", "gpk_polygon_relation_join"} <= names


def test_header_states_the_mask_bits_and_predicate_ids():
    text = open(os.path.join(os.path.dirname(_abi.HERE), "include", "geopolars_hip.h")).read()
    defs = dict(re.findall(r"#define (GPK_PP_\w+) (\d+)", text))
    assert defs == {"GPK_PP_INTERIORS": "1", "GPK_PP_BOUNDARIES": "2", "GPK_PP_A_OUTSIDE": "4", "GPK_PP_B_OUTSIDE": "8",
                    "GPK_PP_PRED_INTERSECTS": "0", "GPK_PP_PRED_WITHIN": "1", "GPK_PP_PRED_CONTAINS": "2", "GPK_PP_PRED_TOUCHES": "3",
                    "GPK_PP_PRED_OVERLAPS": "4", "GPK_PP_PRED_EQUALS": "5", "GPK_PP_PRED_CONTAINS_PROPERLY": "6"}
    assert (_abi.PP_PRED_INTERSECTS, _abi.PP_PRED_WITHIN, _abi.PP_PRED_CONTAINS, _abi.PP_PRED_TOUCHES, _abi.PP_PRED_OVERLAPS,
            _abi.PP_PRED_EQUALS, _abi.PP_PRED_CONTAINS_PROPERLY) == (0, 1, 2, 3, 4, 5, 6)
    for line in ("intersects                 mask & 3", "disjoint             mask != 0 && !(mask & 3)", "touches                    (mask & 2) && !(mask & 1)",
                 "overlaps             (mask & 13) == 13", "within / covered_by        (mask & 1) && !(mask & 4)",
                 "contains / covers    (mask & 1) && !(mask & 8)", "equals                     (mask & 1) && !(mask & 12)",
                 "contains_properly    (mask & 11) == 1"):
        assert line in text, line


# the header's table, written out independently: predicate -> the masks (of all 16) that satisfy it
SATISFIED = {
    "intersects": {1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 14, 15},
    "disjoint": {4, 8, 12},
    "touches": {2, 6, 10, 14},
    "overlaps": {13, 15},
    "within": {1, 3, 9, 11},
    "covered_by": {1, 3, 9, 11},
    "contains": {1, 3, 5, 7},
    "covers": {1, 3, 5, 7},
    "equals": {1, 3},
    "contains_properly": {1, 5},
    "crosses": set(),
}


def test_mask_to_predicate_table_for_all_16_masks():
    masks = np.arange(16, dtype=np.uint8)
    assert set(POLYGON_MASK_PREDICATES) == set(SATISFIED)
    for name, want in SATISFIED.items():
        got = polygon_mask_predicate(masks, name)
        assert got.dtype == bool and set(np.nonzero(got)[0].tolist()) == want, name
    with pytest.raises(_abi.GeopolarsHipError) as e:
        polygon_mask_predicate(masks, "dwithin")
    assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT


def test_predicate_names_of_the_join():
    assert set(POLYGON_RELATION_PREDICATES) == {"intersects", "within", "contains", "covers", "covered_by", "touches", "overlaps", "contains_properly", "equals"}
    assert POLYGON_RELATION_PREDICATES["covers"] == POLYGON_RELATION_PREDICATES["contains"] == _abi.PP_PRED_CONTAINS
    assert POLYGON_RELATION_PREDICATES["covered_by"] == POLYGON_RELATION_PREDICATES["within"] == _abi.PP_PRED_WITHIN
    for a in (PG, MPG):
        for b in (PG, MPG):
            for name, pred in POLYGON_RELATION_PREDICATES.items():
                assert polygon_relation_predicate_arg(name, a, b) == pred
    for a, b in ((LS, PG), (PG, LS), (PT, PG), (MPG, _abi.GEOM_MULTIPOINT)):
        with pytest.raises(_abi.MismatchedGeometry):
            polygon_relation_predicate_arg("touches", a, b)
    for name in ("crosses", "disjoint", "dwithin"):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            polygon_relation_predicate_arg(name, PG, PG)
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT


def _series():
    pts = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0]]))
    lines = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)]]))
    sq = [[(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0), (0.0, 0.0)]]
    return pts, lines, GeoSeries(GeoArrowArray.from_polygons([sq, sq, sq])), GeoSeries(GeoArrowArray.from_polygons([sq, sq]))


def test_argument_errors_come_before_the_device(no_device):
    pts, lines, polys, two = _series()
    for call in (lambda: polys.polygon_relation(lines), lambda: lines.polygon_relation(polys), lambda: pts.polygon_relation(polys),
                 lambda: polygon_relation_pairs(lines, polys), lambda: polygon_relation_pairs(polys, pts, "touches"),
                 lambda: polygon_relation_pairs_device(polys, lines, None, "touches", None, None)):
        with pytest.raises(_abi.MismatchedGeometry):
            call()
    for call in (
        lambda: polys.polygon_relation(two),  # 3 rows against 2
        lambda: polys.polygon_relation(two, other_rows=[0, 1]),  # one entry per row of self
        lambda: polys.polygon_relation(two, other_rows=[[0, 1, 0]]),
        lambda: polys.polygon_relation(two, other_rows=["a", "b", "c"]),
        lambda: polygon_relation_pairs(polys, two, "crosses"),
        lambda: polygon_relation_pairs(polys, two, "disjoint"),
        lambda: polygon_relation_pairs_device(polys, two, None, "dwithin", None, None),
    ):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            call()
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    for name in ("overlaps", "geom_equals", "contains_properly"):
        with pytest.raises(NotImplementedError, match="Point"):
            getattr(pts, name)(polys)
        with pytest.raises(NotImplementedError, match="LineString x Polygon"):
            getattr(lines, name)(polys)
    assert pts._dev is None and lines._dev is None and polys._dev is None and two._dev is None


def test_table_join_checks_its_options_first(no_device):
    pa = pytest.importorskip("pyarrow")
    t = pa.table({"id": pa.array([0]), "geometry": pa.array([b"\x00"], type=pa.binary())})
    for opts in (SpatialJoinRelationArgs(join_type="outer"), SpatialJoinRelationArgs(predicate="crosses"), SpatialJoinRelationArgs(predicate="disjoint")):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            spatial_join_polygon_relation(t, t, opts)
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT


def test_older_surfaces_stay_as_they_are(no_device):
    pts, lines, polys, _ = _series()
    assert set(MASK_PREDICATES) == {"intersects", "disjoint", "covered_by", "covers", "within", "contains", "crosses", "touches"}
    with pytest.raises(_abi.GeopolarsHipError):
        mask_predicate(np.arange(8, dtype=np.uint8), "overlaps")
    assert set(RELATION_PREDICATES) == {"intersects", "within", "contains", "covers", "covered_by", "crosses", "touches"}
    with pytest.raises(_abi.MismatchedGeometry):
        relation_pairs(polys, polys, "touches")
    for name in ("crosses", "touches", "covered_by", "covers", "disjoint"):
        with pytest.raises(NotImplementedError, match="Point"):
            getattr(pts, name)(polys)
        with pytest.raises(NotImplementedError, match="LineString x LineString"):
            getattr(lines, name)(lines)
