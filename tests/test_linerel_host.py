"""Line x line relations, host side: the C ABI symbols, the header's bits and ids, the mask -> predicate table for all 128 masks, the
argument checks that refuse a call before the library is opened, and the older surfaces that must not move."""
import os
import re

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import LINE_MASK_PREDICATES, MASK_PREDICATES, POLYGON_MASK_PREDICATES, GeoSeries, line_mask_predicate, line_relation_args
from geopolars_amd.spatial_index import (
    LINE_RELATION_PREDICATES,
    POLYGON_RELATION_PREDICATES,
    RELATION_PREDICATES,
    SpatialJoinRelationArgs,
    line_relation_pairs,
    line_relation_pairs_device,
    line_relation_predicate_arg,
    polygon_relation_pairs,
    relation_pairs,
    spatial_join_line_relation,
)
from tests import linerel_ref as L
from tests.host_build import no_device  # noqa: F401  (no_device: a fixture)

LS, MLS, PG, PT = _abi.GEOM_LINESTRING, _abi.GEOM_MULTILINESTRING, _abi.GEOM_POLYGON, _abi.GEOM_POINT


def test_exported_symbols_name_the_line_relation_calls():
    assert "gpk_line_relation" in _abi.EXPORTED_SYMBOLS and "gpk_line_relation_join" in _abi.EXPORTED_SYMBOLS
    assert _abi._PROTOS["gpk_line_relation"] == _abi._PROTOS["gpk_polygon_relation"]
    assert _abi._PROTOS["gpk_line_relation_join"] == _abi._PROTOS["gpk_polygon_relation_join"]
    assert (_abi.LL_INTERIORS, _abi.LL_SHARED_PIECE, _abi.LL_INT_BND, _abi.LL_BND_INT, _abi.LL_BND_BND, _abi.LL_A_OUTSIDE, _abi.LL_B_OUTSIDE) == (1, 2, 4, 8, 16, 32, 64)


def test_header_states_the_mask_bits_and_predicate_ids():
    text = open(os.path.join(os.path.dirname(_abi.HERE), "include", "geopolars_hip.h")).read()
    defs = dict(re.findall(r"#define (GPK_LL_\w+) (\d+)", text))
    assert defs == {"GPK_LL_INTERIORS": "1", "GPK_LL_SHARED_PIECE": "2", "GPK_LL_INT_BND": "4", "GPK_LL_BND_INT": "8", "GPK_LL_BND_BND": "16",
                    "GPK_LL_A_OUTSIDE": "32", "GPK_LL_B_OUTSIDE": "64", **{f"GPK_LL_PRED_{n.upper()}": str(i) for n, i in L.PRED_IDS.items()}}
    assert {n: getattr(_abi, f"LL_PRED_{n.upper()}") for n in L.PRED_IDS} == L.PRED_IDS
    assert LINE_RELATION_PREDICATES == L.PRED_IDS
    for line in ("intersects     mask & 31", "disjoint       mask != 0 && !(mask & 31)", "touches        (mask & 28) && !(mask & 1)",
                 "crosses        (mask & 1) && !(mask & 2)", "overlaps       (mask & 2) && (mask & 32) && (mask & 64)",
                 "within         (mask & 1) && !(mask & 32)", "contains       (mask & 1) && !(mask & 64)",
                 "covered_by     (mask & 31) && !(mask & 32)", "covers         (mask & 31) && !(mask & 64)", "equals         (mask & 1) && !(mask & 96)"):
        assert line in text, line


def test_mask_to_predicate_table_for_all_128_masks():
    masks = np.arange(128, dtype=np.uint8)
    assert set(LINE_MASK_PREDICATES) == set(L.PREDICATES)
    for name, f in L.PREDICATES.items():
        got = line_mask_predicate(masks, name)
        assert got.dtype == bool and got.tolist() == [f(int(m)) for m in masks], name
    assert not any(line_mask_predicate(np.zeros(1, dtype=np.uint8), n)[0] for n in LINE_MASK_PREDICATES)
    with pytest.raises(_abi.GeopolarsHipError) as e:
        line_mask_predicate(masks, "contains_properly")
    assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT


def test_predicate_names_of_the_join():
    for a in (LS, MLS):
        for b in (LS, MLS):
            for name, pred in LINE_RELATION_PREDICATES.items():
                assert line_relation_predicate_arg(name, a, b) == pred
    for a, b in ((LS, PG), (PG, LS), (PT, LS), (MLS, _abi.GEOM_MULTIPOINT)):
        with pytest.raises(_abi.MismatchedGeometry):
            line_relation_predicate_arg("touches", a, b)
    for name in ("disjoint", "dwithin", "contains_properly"):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            line_relation_predicate_arg(name, PG, PG)  # the ABI's order: the predicate first
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT and not isinstance(e.value, _abi.MismatchedGeometry)


def _series():
    pts = GeoSeries(GeoArrowArray.from_points([[0.0, 0.0], [1.0, 1.0]]))
    line = [(0.0, 0.0), (1.0, 1.0)]
    sq = [[(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0), (0.0, 0.0)]]
    return pts, GeoSeries(GeoArrowArray.from_linestrings([line] * 3)), GeoSeries(GeoArrowArray.from_linestrings([line] * 2)), GeoSeries(GeoArrowArray.from_polygons([sq] * 3))


def test_argument_errors_come_before_the_device(no_device):
    pts, lines, two, polys = _series()
    for call in (lambda: lines.line_relation(polys), lambda: polys.line_relation(lines), lambda: pts.line_relation(lines), lambda: polys.line_relation(polys),
                 lambda: lines.line_predicate(polys, "touches"), lambda: line_relation_pairs(lines, polys), lambda: line_relation_pairs(pts, lines, "touches"),
                 lambda: line_relation_pairs_device(lines, polys, None, "touches", None, None)):
        with pytest.raises(_abi.MismatchedGeometry):
            call()
    for call in (
        lambda: lines.line_relation(two),  # 3 rows against 2
        lambda: lines.line_relation(two, other_rows=[0, 1]),  # one entry per row of self
        lambda: lines.line_relation(two, other_rows=[[0, 1, 0]]),
        lambda: lines.line_relation(two, other_rows=["a", "b", "c"]),
        lambda: lines.line_predicate(lines, "contains_properly"),
        lambda: line_relation_pairs(lines, two, "disjoint"),
        lambda: line_relation_pairs(lines, polys, "disjoint"),  # the predicate before the families
        lambda: line_relation_pairs_device(lines, two, None, "dwithin", None, None),
    ):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            call()
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT and not isinstance(e.value, _abi.MismatchedGeometry)
    assert line_relation_args("line_relation", lines, two, [1, 0, 7]).dtype == np.uint32
    assert line_relation_args("line_relation", lines, lines, None) is None
    assert all(s._dev is None for s in (pts, lines, two, polys))


def test_table_join_checks_its_options_first(no_device):
    pa = pytest.importorskip("pyarrow")
    t = pa.table({"id": pa.array([0]), "geometry": pa.array([b"\x00"], type=pa.binary())})
    for opts in (SpatialJoinRelationArgs(join_type="outer"), SpatialJoinRelationArgs(predicate="contains_properly"), SpatialJoinRelationArgs(predicate="disjoint")):
        with pytest.raises(_abi.GeopolarsHipError) as e:
            spatial_join_line_relation(t, t, opts)
        assert e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT


def test_older_surfaces_stay_as_they_are(no_device):
    pts, lines, _, polys = _series()
    assert set(MASK_PREDICATES) == {"intersects", "disjoint", "covered_by", "covers", "within", "contains", "crosses", "touches"}
    assert set(RELATION_PREDICATES) == {"intersects", "within", "contains", "covers", "covered_by", "crosses", "touches"}
    assert set(POLYGON_MASK_PREDICATES) == {"intersects", "disjoint", "touches", "overlaps", "within", "contains", "equals", "contains_properly", "crosses", "covered_by", "covers"}
    assert "crosses" not in POLYGON_RELATION_PREDICATES
    for join in (relation_pairs, polygon_relation_pairs):
        with pytest.raises(_abi.MismatchedGeometry):
            join(lines, lines, "touches")
    for name in ("crosses", "touches", "covered_by", "covers", "disjoint"):
        with pytest.raises(NotImplementedError, match="LineString x LineString"):
            getattr(lines, name)(lines)
    for name in ("overlaps", "geom_equals", "contains_properly"):
        with pytest.raises(NotImplementedError, match="LineString x LineString"):
            getattr(lines, name)(lines)
