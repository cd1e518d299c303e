"""The row pairing of every row-wise method that takes a row map, before the library is opened: a map that is not a 1-D array of one row
number per row, or — without a map — unequal row counts, is refused with GPK_ERR_INVALID_ARGUMENT and one of three messages
(geoseries.row_map_arg, paired_rows_arg), and neither series has been uploaded.  No device is needed."""
import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries, point_relation_rows_arg, relation_rows_arg
from tests.host_build import no_device  # noqa: F401  (a fixture)


def _series():
    """three rows of every family, and two-row columns for the count checks"""
    sq = [[(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0), (0.0, 0.0)]]
    ln = [[(0.0, 0.0), (1.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)], [(2.0, 0.0), (3.0, 1.0)]]
    xy = [[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]]
    return {
        "pts": GeoSeries(GeoArrowArray.from_points(xy)), "lines": GeoSeries(GeoArrowArray.from_linestrings(ln)),
        "polys": GeoSeries(GeoArrowArray.from_polygons([sq, sq, sq])), "pts2": GeoSeries(GeoArrowArray.from_points(xy[:2])),
        "lines2": GeoSeries(GeoArrowArray.from_linestrings(ln[:2])), "polys2": GeoSeries(GeoArrowArray.from_polygons([sq, sq])),
    }


# (the op of the messages, the mapped side whose rows the map has one entry for, the side it maps into, the noun of the count message,
#  the call).  distance, contains, within, intersects and dwithin leave the count check without a map to the library.
METHODS = [
    ("distance", "pts", "lines", "rows", lambda a, b, r: a.distance(b, other_rows=r)),
    ("hausdorff_distance", "lines", "polys", "rows", lambda a, b, r: a.hausdorff_distance(b, other_rows=r)),
    ("frechet_distance", "lines", "lines", "rows", lambda a, b, r: a.frechet_distance(b, other_rows=r)),
    ("contains", "polys", "pts", "rows", lambda a, b, r: a.contains(b, other_rows=r)),
    ("within", "pts", "polys", "rows", lambda a, b, r: a.within(b, other_rows=r)),
    ("intersects", "lines", "polys", "rows", lambda a, b, r: a.intersects(b, other_rows=r)),
    ("dwithin", "pts", "lines", "rows", lambda a, b, r: a.dwithin(b, 1.0, other_rows=r)),
    ("line_polygon_relation", "lines", "polys", "rows", lambda a, b, r: a.line_polygon_relation(b, other_rows=r)),
    ("polygon_relation", "polys", "polys", "rows", lambda a, b, r: a.polygon_relation(b, other_rows=r)),
    ("line_relation", "lines", "lines", "rows", lambda a, b, r: a.line_relation(b, other_rows=r)),
    ("point_relation", "pts", "polys", "rows", lambda a, b, r: a.point_relation(b, other_rows=r)),
    ("intersection_area", "polys", "polys", "rows", lambda a, b, r: a.intersection_area(b, other_rows=r)),
    ("intersection_length", "lines", "polys", "rows", lambda a, b, r: a.intersection_length(b, other_rows=r)),
    ("intersection", "lines", "polys", "rows", lambda a, b, r: a.intersection(b, other_rows=r)),
    ("difference", "lines", "polys", "rows", lambda a, b, r: a.difference(b, other_rows=r)),
    ("polygon_intersection", "polys", "polys", "rows", lambda a, b, r: a.polygon_intersection(b, other_rows=r)),
    ("polygon_difference", "polys", "polys", "rows", lambda a, b, r: a.polygon_difference(b, other_rows=r)),
    ("polygon_union", "polys", "polys", "rows", lambda a, b, r: a.polygon_union(b, other_rows=r)),
    ("closest_point", "pts", "lines", "points", lambda a, b, r: a.closest_point(b, other_rows=r)),
    ("project", "pts", "lines", "points", lambda a, b, r: b.project(a, rows=r)),  # (the points are `other`, the map goes into the lines)
    ("geodesic_distance", "pts", "pts", "rows", lambda a, b, r: a.geodesic_distance(b, other_rows=r)),
]
COUNT_CHECK_IS_THE_LIBRARYS = ("distance", "contains", "within", "intersects", "dwithin")


def _refused(call, a, b, message):
    with pytest.raises(_abi.GeopolarsHipError) as e:
        call()
    assert type(e.value) is _abi.GeopolarsHipError and e.value.code == _abi.GPK_ERR_INVALID_ARGUMENT == 6
    assert str(e.value) == "[gpk status 6] " + message
    assert a._dev is None and b._dev is None


@pytest.mark.parametrize("op,left,right,noun,call", METHODS, ids=[m[0] for m in METHODS])
def test_a_bad_row_map_is_refused_before_the_library_is_opened(no_device, op, left, right, noun, call):
    for rows, message in (
        ([[0, 1, 0]], f"{op}: 3 row numbers for 3 {noun}"),  # 2-D
        (["a", "b", "c"], f"{op}: the row map must be an array of row numbers"),
        ([0, 1], f"{op}: 2 row numbers for 3 {noun}"),
    ):
        s = _series()
        _refused(lambda: call(s[left], s[right], rows), s[left], s[right], message)


@pytest.mark.parametrize("op,left,right,noun,call", [m for m in METHODS if m[0] not in COUNT_CHECK_IS_THE_LIBRARYS],
                         ids=[m[0] for m in METHODS if m[0] not in COUNT_CHECK_IS_THE_LIBRARYS])
def test_unequal_row_counts_without_a_map_are_refused_before_the_library_is_opened(no_device, op, left, right, noun, call):
    s = _series()
    _refused(lambda: call(s[left], s[right + "2"], None), s[left], s[right + "2"], f"{op}: row counts differ (3 vs 2)")


@pytest.mark.parametrize("op,args,mapped,needs", [
    ("line_polygon_relation", relation_rows_arg, "lines", "a row map needs the lineal column on the left (it maps line rows to polygon rows)"),
    ("point_relation", point_relation_rows_arg, "pts", "a row map needs the punctual column on the left (it maps point rows to rows of the other column)"),
], ids=["line_polygon_relation", "point_relation"])
def test_either_order_relations_take_a_map_only_from_the_mapped_side(no_device, op, args, mapped, needs):
    s = _series()
    a, polys = s[mapped], s["polys"]
    _refused(lambda: getattr(polys, op)(a, other_rows=[2, 1, 0]), polys, a, f"{op}: {needs}")
    _refused(lambda: args(op, polys, a, [2, 1, 0], False), polys, a, f"{op}: {needs}")
    assert args(op, polys, a, [0, 1, 2], False) is None  # the identity is no map
    assert args(op, polys, a, None, False) is None
    good = args(op, a, polys, [2, 1, 0], True)
    assert good.dtype == np.uint32 and good.flags.c_contiguous and good.tolist() == [2, 1, 0]
    _refused(lambda: args(op, polys, s[mapped + "2"], [0, 1, 2], False), polys, s[mapped + "2"], f"{op}: row counts differ (3 vs 2)")
