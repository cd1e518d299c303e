"""CPU: the exact point -> geometry distance of tests/exact_ref.py, held to account on the fixture of every (family, G) instance of
the distance kernels (distance_kernel<G, KIND>, nearest_best_kernel<G, KIND>, nearest_emit_kernel<G, KIND>).

Each fixture must select the G it was built for under the restated group-size rule; the oracle's row-wise distance must be within
distance_bound of the exact value; zeros must agree.  For POINT, MULTIPOINT and the polygonal families the oracle is zero exactly
where the exact distance is.  For linestrings geo's line_string_contains_point also counts a point whose |tx - ty| is within
f64::EPSILON of a segment's line as on it (a distance of a few ulps of the segment's length becomes 0), so there the oracle's zeros
must include the exact ones."""
from decimal import Decimal

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from tests import exact_ref as X

BANDS = {1: (0.0, 16.0), 8: (16.0, 128.0), 32: (128.0, float("inf"))}


def test_group_size_rule_at_its_thresholds():
    for mean_x8, G in ((1, 1), (127, 1), (128, 8), (8 * 127 + 7, 8), (8 * 128, 32), (8 * 4096, 32)):
        assert X.distance_group_size(_abi.GEOM_LINESTRING, mean_x8, 8) == G, mean_x8
    assert X.distance_group_size(_abi.GEOM_POINT, 10**6, 10) == 1
    assert X.distance_group_size(_abi.GEOM_POLYGON, 0, 0) == 1


@pytest.mark.parametrize("family,G", X.INSTANCES)
def test_fixture_selects_the_instance_it_was_built_for(family, G):
    fx = X.instance_fixture(family, G)
    a = fx["array"]
    assert a.geom_type == X.FAMILIES[family] and X.group_size_of(a) == G
    if family != "point":  # well inside the band: a mean at a threshold would make the fixture's G fragile
        lo, hi = BANDS[G]
        mean = a.n_coords / a.n_geoms
        assert 1.5 * lo <= mean <= hi / 1.5, mean
    valid, usable = np.asarray(fx["validity"]), fx["usable"]
    assert (~valid).any() and (valid & ~usable).any(), "null and empty rows"
    if X.FAMILIES[family] in X.POLYGONAL:
        assert sum(m["hole"] is not None for m in fx["meta"]) >= 5 and sum(m["edge"] is not None for m in fx["meta"]) >= 5


@pytest.mark.parametrize("family,G", X.INSTANCES)
def test_oracle_rowwise_distance_within_the_exact_bound(oracle, family, G):
    fx = X.instance_fixture(family, G)
    kind = fx["kind"]
    od = oracle.distance_rowwise(GeoArrowArray.from_points(fx["queries"]), fx["array"])
    ex = X.exact_rowwise(fx)
    n_zero = 0
    for i, (d, b) in enumerate(ex):
        if not fx["validity"][i]:
            assert np.isnan(od[i]), i
            continue
        if d is None:  # an empty row
            e = X.EMPTY_DISTANCE[kind]
            assert (np.isnan(od[i]) and np.isnan(e)) or od[i] == e, (i, od[i])
            continue
        assert X.abs_err(od[i], d) <= b, (i, od[i], d, b)
        if kind == _abi.GEOM_LINESTRING or kind == _abi.GEOM_MULTILINESTRING:
            assert od[i] == 0.0 or d > 0, (i, od[i])
        else:
            assert (od[i] == 0.0) == (d == 0), (i, od[i], d)
        n_zero += d == 0
    assert n_zero >= 5, "the fixture reaches points on the geometries"
    assert np.count_nonzero(od > 0) >= len(od) // 3


@pytest.mark.parametrize("family,G", X.INSTANCES)
def test_exact_minimum_equals_the_unfiltered_minimum(family, G):
    """the f64 pre-filter of exact_min_distance never drops the nearest row (checked against every usable row, exactly)"""
    fx = X.instance_fixture(family, G)
    got = X.exact_nearest_minima(fx)
    for l in range(0, len(fx["left"]), 15):
        p = fx["left"][l]
        d2s = [X.exact_row_distance2(p, fx["kind"], r)[0] for r, u in zip(fx["rows"], fx["usable"]) if u]
        assert got[l][0] == X.dec_sqrt(min(d2s)), l


def test_exact_distance_of_hand_made_cases():
    sq = [np.array([(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0), (0.0, 0.0)]), np.array([(1.0, 1.0), (1.0, 3.0), (3.0, 3.0), (3.0, 1.0), (1.0, 1.0)])]
    P = _abi.GEOM_POLYGON
    assert X.exact_row_distance((2.0, 2.0), P, sq)[0] == 1  # inside the hole: to the hole's ring
    assert X.exact_row_distance((0.5, 0.5), P, sq)[0] == 0
    assert X.exact_row_distance((1.0, 2.0), P, sq)[0] == 0  # on the hole's boundary
    assert X.exact_row_distance((7.0, 8.0), P, sq)[0] == 5
    assert X.exact_row_distance((3.0, 4.0), _abi.GEOM_MULTIPOINT, [(0.0, 0.0), (3.0, 5.0)])[0] == 1
    assert X.exact_row_distance((0.0, 1.0), _abi.GEOM_MULTILINESTRING, [[(5.0, 5.0), (6.0, 5.0)], [(-1.0, 0.0), (1.0, 0.0)]])[0] == 1
    assert X.exact_row_distance((0.0, 1.0), _abi.GEOM_LINESTRING, [])[0] is None
    m = X.f64_distance_matrix([(2.0, 2.0), (0.5, 0.5), (9.0, 4.0)], P, [sq, [], sq], usable=[True, True, False])
    assert m[:, 0].tolist() == [1.0, 0.0, 5.0] and np.isinf(m[:, 1:]).all()
    assert X.exact_row_distance((1.0, 1.0), _abi.GEOM_POINT, (4.0, 5.0))[0] == Decimal(5)
    # overlapping parts of a multipolygon: inside either part is inside (an even-odd count over the whole row would say outside)
    moved = [r + 2.0 for r in sq[:1]]
    m = X.f64_distance_matrix([(3.0, 3.5)], _abi.GEOM_MULTIPOLYGON, [[sq[:1], moved]])
    assert m[0, 0] == 0.0 and X.exact_row_distance((3.0, 3.5), _abi.GEOM_MULTIPOLYGON, [sq[:1], moved])[0] == 0
