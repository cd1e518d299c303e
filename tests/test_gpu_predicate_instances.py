"""GPU: every polygon predicate kernel path against exact answers (tests/exact_predicates.py), bit for bit.

Row-wise point x polygonal predicates run point_poly_predicate_kernel<G> for G = 1 .. 64 (one fixture per G and family, with
identity, shuffled and out-of-range b_rows and the mirrored calls); polygon x polygon intersects runs the general routine
row-wise and both forms in the join's refine (ring sizes across the small / general switch, lists flushed in chunks,
containment-decided pairs, degenerate rings held to geo's algorithm); the join at scale gives every refine group at least four
candidates (the staged-ring reuse) on single-ring columns and on columns with a hole; three joins reach the three candidate
regimes; contains / within run row-wise and through the contains join.  test_exact_predicate_ref.py checks which path each
fixture selects."""
import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from geopolars_amd.geoseries import GeoSeries
from geopolars_amd.spatial_index import join_pairs
from tests import exact_predicates as E
from tests.exact_ref import column

from .test_exact_predicate_ref import scale_tiles

pytestmark = pytest.mark.gpu
P, MP = _abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON


@pytest.mark.parametrize("kind,G", E.POINT_POLY_INSTANCES)
def test_point_poly_instance_against_exact_positions(gpk, kind, G):
    fx = E.point_poly_fixture(kind, G)
    polys = GeoSeries(fx["array"])
    pts, rows_of = fx["points"], fx["rows_of"]
    n_rows = len(fx["rows"])
    rng = np.random.default_rng(G + kind)
    perm = rng.permutation(len(pts))
    q = GeoSeries(GeoArrowArray.from_points(np.concatenate([pts[perm], [[1.0, 1.0], [2.0, 2.0]]])))
    rows = np.concatenate([rows_of[perm], [n_rows, 0xFFFFFFFF]]).astype(np.uint32)
    for pred, key in (("within", "inside"), ("intersects", "not_outside")):
        got = q.within(polys, other_rows=rows) if pred == "within" else q.intersects(polys, other_rows=rows)
        assert np.array_equal(got[: len(perm)], fx[key][perm]), pred
        assert not got[len(perm) :].any(), "out-of-range rows"
    # identity rows: point i asks about row i (one probe a row, kinds cycling); the mirrored calls
    first = np.array([np.flatnonzero(rows_of == i)[i % np.count_nonzero(rows_of == i)] for i in range(n_rows)])
    ident = GeoSeries(GeoArrowArray.from_points(pts[first]))
    inside, touch = fx["inside"][first], fx["not_outside"][first]
    assert np.array_equal(ident.within(polys), inside)
    assert np.array_equal(polys.contains(ident), inside)
    assert np.array_equal(ident.intersects(polys), touch)
    assert np.array_equal(polys.intersects(ident), touch)
    # polygon on the left with b_rows into the points
    pick = rng.permutation(n_rows)
    assert np.array_equal(polys.contains(ident, other_rows=pick.astype(np.uint32)), np.array(
        [E.point_predicate(pts[first][pick[i]], E.row_members(kind, fx["rows"][i]), "contains") and fx["validity"][i] for i in range(n_rows)]))


def _cols(pairs, kb=P):
    return column(P, [A for _, A, _ in pairs]), column(kb, [B for _, _, B in pairs])


def test_polygon_intersects_rowwise_and_joined(gpk):
    """row-wise (general routine) and the join's refine (small form for single-ring pairs up to 66 coordinates) against geo's
    algorithm restated exactly"""
    pairs = E.intersects_pairs()
    exp = np.array([E.intersects([A], [B]) for _, A, B in pairs])
    a, b = _cols(pairs)
    ga, gb = GeoSeries(a), GeoSeries(b)
    names = [n for n, _, _ in pairs]
    for got in (ga.intersects(gb), gb.intersects(ga)):
        bad = [names[i] for i in np.flatnonzero(got != exp)]
        assert not bad, bad
    perm = np.random.default_rng(1).permutation(len(pairs))
    assert np.array_equal(ga.intersects(gb, other_rows=perm.astype(np.uint32)), np.array([E.intersects([pairs[i][1]], [pairs[p][2]]) for i, p in enumerate(perm)]))
    # the join: each pair on its own tile, so a left row's candidates are its own right row and nothing else
    shift = np.arange(len(pairs), dtype=np.float64)[:, None] * [1024.0, 0.0]
    la = column(P, [[r + s for r in A] for (_, A, _), s in zip(pairs, shift)])
    rb = column(P, [[r + s for r in B] for (_, _, B), s in zip(pairs, shift)])
    for left, right in ((la, rb), (rb, la)):
        got, counts = join_pairs(GeoSeries(left), GeoSeries(right), "intersects")
        want = np.flatnonzero(exp)
        bad = sorted(set(names[i] for i in set(want) ^ set(got[:, 0].tolist())))
        assert not bad, bad
        assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(counts, exp.astype(np.uint32))


def test_polygon_multipolygon_intersects(gpk):
    pairs = E.polygon_multi_pairs()
    exp = np.array([E.intersects([A], B) for _, A, B in pairs])
    a, b = _cols(pairs, MP)
    assert np.array_equal(GeoSeries(a).intersects(GeoSeries(b)), exp)
    assert np.array_equal(GeoSeries(b).intersects(GeoSeries(a)), exp)


@pytest.mark.parametrize("hole", [False, True], ids=["single_ring", "one_row_with_hole"])
def test_intersects_join_at_scale(gpk, hole):
    _, cus = _abi.device_info()
    tpl = E.join_templates()
    left, right, pairs, counts, ccounts = E.tiled_join(tpl, scale_tiles(tpl, cus), hole_row=hole)
    assert E.refine_per(int(ccounts.sum()), cus) >= 4
    got, gc = join_pairs(GeoSeries(left), GeoSeries(right), "intersects")
    assert np.array_equal(gc, counts)
    assert np.array_equal(got, pairs)


@pytest.mark.parametrize("counts", [(16, 17, 48), (16, 17, 48, 49)], ids=["compact", "sorted"])
def test_candidate_regimes(gpk, counts):
    left, right = E.regime_join(counts)
    cands = E.box_candidates([E.geom_box([l]) for l in left], [E.geom_box([r]) for r in right])
    exp = [(i, j) for i, c in enumerate(cands) for j in c if E.intersects([left[i]], [right[j]])]
    got, gc = join_pairs(GeoSeries(column(P, left)), GeoSeries(column(P, right)), "intersects")
    assert [tuple(p) for p in got.tolist()] == exp


def test_contains_rowwise_and_joined(gpk):
    cases = E.contains_pairs()
    exp = np.array([E.contains(A, B) for _, A, B in cases])
    a, b = GeoSeries(column(MP, [A for _, A, _ in cases])), GeoSeries(column(P, [B[0] for _, _, B in cases]))
    assert np.array_equal(a.contains(b), exp)
    assert np.array_equal(b.within(a), exp)
    # the contains join: each case on its own tile
    shift = np.arange(len(cases), dtype=np.float64)[:, None] * [1024.0, 0.0]
    la = column(MP, [[[r + s for r in p] for p in A] for (_, A, _), s in zip(cases, shift)])
    rb = column(P, [[r + s for r in B[0]] for (_, _, B), s in zip(cases, shift)])
    got, counts = join_pairs(GeoSeries(la), GeoSeries(rb), "contains")
    assert np.array_equal(counts, exp.astype(np.uint32))
    assert np.array_equal(got[:, 0], np.flatnonzero(exp)) and np.array_equal(got[:, 0], got[:, 1])
