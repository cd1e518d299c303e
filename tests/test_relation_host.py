"""Line x polygon relations, host side: the C ABI symbols, the mask -> predicate table, the predicate-name / side rules of the join and
the argument checks that refuse a call before the library is opened."""

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import MASK_PREDICATES, GeoSeries, mask_predicate
from geopolars_amd.spatial_index import (
    RELATION_PREDICATES,
    SpatialJoinRelationArgs,
    relation_pairs,
    relation_pairs_device,
    relation_predicate_arg,
    spatial_join_relation,
)
from tests.host_build import exported_symbols, no_device  # noqa: F401  (no_device: a fixture)

LS, MLS, PG, MPG, PT = _abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON, _abi.GEOM_POINT


def test_exported_symbols_name_the_relation_calls():
    assert "gpk_line_polygon_relation" in _abi.EXPORTED_SYMBOLS and "gpk_line_polygon_join" in _abi.EXPORTED_SYMBOLS
    assert len(_abi._PROTOS["gpk_line_polygon_relation"][1]) == 6
    assert len(_abi._PROTOS["gpk_line_polygon_join"][1]) == 12
    assert (_abi.LP_INTERIOR, _abi.LP_BOUNDARY, _abi.LP_EXTERIOR) == (1, 2, 4)
    assert set(_abi.PREDICATES) == {"intersects", "contains", "within"}  # gpk_spatial_join's predicate codes stay as they are


def test_built_library_exports_the_relation_calls():
    names = exported_symbols()
    assert {"gpk_line_polygon_relation", "gpk_line_polygon_join"} <= names


def test_header_states_the_mask_bits_and_predicate_ids():
    import os
    import re

    text = open(os.path.join(os.path.dirname(_abi.HERE), "include", "geopolars_hip.h")).read()
    defs = dict(re.findall(r"#define (GPK_LP_\w+) (\d+)", text))
    assert defs == {"GPK_LP_INTERIOR": "1", "GPK_LP_BOUNDARY": "2", "GPK_LP_EXTERIOR": "4", "GPK_LP_PRED_INTERSECTS": "0", "GPK_LP_PRED_WITHIN": "1",
                    "GPK_LP_PRED_COVERED_BY": "2", "GPK_LP_PRED_CROSSES": "3", "GPK_LP_PRED_TOUCHES": "4"}
    assert (_abi.LP_PRED_INTERSECTS, _abi.LP_PRED_WITHIN, _abi.LP_PRED_COVERED_BY, _abi.LP_PRED_CROSSES, _abi.LP_PRED_TOUCHES) == (0, 1, 2, 3, 4)


# mask: (intersects, disjoint, covered_by, within, crosses, touches)
TABLE = {
    0: (0, 0, 0, 0, 0, 0),
    1: (1, 0, 1, 1, 0, 0),
    2: (1, 0, 1, 0, 0, 1),
    3: (1, 0, 1, 1, 0, 0),
    4: (0, 1, 0, 0, 0, 0),
    5: (1, 0, 0, 0, 1, 0),
    6: (1, 0, 0, 0, 0, 1),
    7: (1, 0, 0, 0, 1, 0),
}


def test_mask_to_predicate_table():
    masks = np.arange(8, dtype=np.uint8)
    for k, name in enumerate(("intersects", "disjoint", "covered_by", "within", "crosses", "touches")):
        assert mask_predicate(masks, name).tolist() == [bool(TABLE[m][k]) for m in range(8)], name
    assert np.array_equal(mask_predicate(masks, "covers"), mask_predicate(masks, "covered_by"))
    assert np.array_equal(mask_predicate(masks, "contains"), mask_predicate(masks, "within"))
    assert set(MASK_PREDICATES) == {"intersects", "disjoint", "covered_by", "covers", "within", "contains", "crosses", "touches"}
    with pytest.raises(_abi.GeopolarsHipError):
        mask_predicate(masks, "overlaps")


def test_predicate_names_are_checked_against_the_side_of_the_lines():
    assert set(RELATION_PREDICATES) == {"intersects", "within", "contains", "covers", "covered_by", "crosses", "touches"}
    for lines in (LS, MLS):
        for polys in (PG, MPG):
            for name in ("intersects", "crosses", "touches"):
                assert relation_predicate_arg(name, lines, polys) == relation_predicate_arg(name, polys, lines) == RELATION_PREDICATES[name][0]
            assert relation_predicate_arg("within", lines, polys) == _abi.LP_PRED_WITHIN == relation_predicate_arg("contains", polys, lines)
            assert relation_predicate_arg("covered_by", lines, polys) == _abi.LP_PRED_COVERED_BY == relation_predicate_arg("covers", polys, lines)
            for name, a, b in (("within", polys, lines), ("covered_by", polys, lines), ("contains", lines, polys), ("covers", lines, polys)):
                with pytest.raises(_abi.GeopolarsHipError) as e:
                    relation_predicate_arg(name, a, b)
                assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    for a, b in ((LS, LS), (PG, PG), (PT, PG), (LS, PT), (MLS, _abi.GEOM_MULTIPOINT)):
        with pytest.raises(_abi.MismatchedGeometry):
            relation_predicate_arg("intersects", a, b)
    with pytest.raises(_abi.GeopolarsHipError) as e:
        relation_predicate_arg("dwithin", LS, PG)
    assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT


def test_relation_args_defaults():
    a = SpatialJoinRelationArgs()
    assert a.predicate == "intersects" and a.join_type == "inner" and a.relation_col is None
    assert a.l_suffix == "_left" and a.r_suffix == "_right" and a.r_index is None and a.l_geom_type == -1 and a.r_geom_type == -1


def _series():
    pts = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0]]))
    lines = GeoSeries(GeoArrowArray.from_linestrings([[(0.0, 0.0), (1.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)]]))
    sq = [[(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0), (0.0, 0.0)]]
    polys = GeoSeries(GeoArrowArray.from_polygons([sq, sq, sq]))
    return pts, lines, polys


def test_argument_errors_come_before_the_device(no_device):
    pts, lines, polys = _series()
    for call in (lambda: lines.line_polygon_relation(pts), lambda: pts.line_polygon_relation(polys), lambda: lines.line_polygon_relation(lines),
                 lambda: relation_pairs(lines, pts), lambda: relation_pairs(polys, polys, "touches")):
        with pytest.raises(_abi.MismatchedGeometry):
            call()
    for call in (
        lambda: lines.line_polygon_relation(polys),  # 2 rows against 3
        lambda: polys.line_polygon_relation(lines),
        lambda: lines.line_polygon_relation(polys, other_rows=[0, 1, 2]),  # one entry per row of self
        lambda: lines.line_polygon_relation(polys, other_rows=[[0, 1]]),
        lambda: lines.line_polygon_relation(polys, other_rows=["a", "b"]),
        lambda: polys.line_polygon_relation(lines, other_rows=[1, 0, 1]),  # a row map needs the lines in self
        lambda: relation_pairs(lines, polys, "overlaps"),
        lambda: relation_pairs(lines, polys, "contains"),
        lambda: relation_pairs(polys, lines, "within"),
        lambda: relation_pairs(lines, polys, "covers"),
    ):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            call()
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
    for name in ("crosses", "touches", "covered_by", "covers", "disjoint"):
        with pytest.raises(NotImplementedError, match="Point"):
            getattr(pts, name)(polys)
        with pytest.raises(NotImplementedError, match="LineString x LineString"):
            getattr(lines, name)(lines)
    assert pts._dev is None and lines._dev is None and polys._dev is None


def test_table_join_checks_its_options_first(no_device):
    pa = pytest.importorskip("pyarrow")
    t = pa.table({"id": pa.array([0]), "geometry": pa.array([b"\x00"], type=pa.binary())})
    for opts in (SpatialJoinRelationArgs(join_type="outer"), SpatialJoinRelationArgs(predicate="dwithin"), SpatialJoinRelationArgs(predicate="disjoint")):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            spatial_join_relation(t, t, opts)
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT
