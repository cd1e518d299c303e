"""CPU: the exact polygon predicates of tests/exact_predicates.py, held to account, and the paths their fixtures select.

The exact reference must reproduce the committed lattice golden and the rational brute force of test_oracle_rational.py; the
oracle must agree with it on every new fixture; each fixture must select the kernel path it is named for under the restated
rules (pick_group_rows, the small-form condition, the per-row candidate counts and the refine's candidates per group)."""
from fractions import Fraction

import numpy as np
import pytest

from geopolars_amd import _abi
from geopolars_amd.geoarrow import GeoArrowArray
from tests import exact_predicates as E
from tests.exact_ref import column

from .lattice import load_contains_golden
from .test_oracle_rational import contains_bruteforce, intersects_bruteforce

P, MP = _abi.GEOM_POLYGON, _abi.GEOM_MULTIPOLYGON
CUS = (64, 256, 304)  # CU counts the join-at-scale sizing is checked for (the MI355X has 256)


def _open(poly):
    return [[(Fraction(float(x)), Fraction(float(y))) for x, y in r[:-1]] for r in poly]


def test_reference_reproduces_the_lattice_golden():
    a, b, exp = load_contains_golden()
    exp_i = load_contains_golden(key="intersects")[2]
    ga, gb = [], []
    for arr, out in ((a, ga), (b, gb)):
        for g in range(arr.n_geoms):
            r0, r1 = arr.geom_offsets[g], arr.geom_offsets[g + 1]
            out.append([arr.xy[arr.ring_offsets[r] : arr.ring_offsets[r + 1]] for r in range(r0, r1)])
    idx = range(0, len(exp), 4)
    assert all(E.contains([ga[i]], [gb[i]]) == exp[i] for i in idx)
    assert all(E.intersects([ga[i]], [gb[i]]) == exp_i[i] for i in idx)


def test_reference_agrees_with_the_rational_brute_force():
    import random

    from .lattice import concentric_pair, random_pair

    rng = random.Random(3)
    for _ in range(150):
        pa, pb = concentric_pair(rng) if rng.random() < 0.5 else random_pair(rng)
        A = [np.array(r + r[:1], dtype=np.float64) for r in pa]
        B = [np.array(r + r[:1], dtype=np.float64) for r in pb]
        assert E.intersects([A], [B]) == intersects_bruteforce(pa, pb)
        assert E.contains([A], [B]) == contains_bruteforce(pa, pb)


def test_exact_integers_and_positions_by_hand():
    a, b = E.scaled_ints(np.array([0.5, 3.0]), np.array([2.0**-40]))
    assert a.dtype == object and a.tolist() == [2**39, 3 * 2**40] and b.tolist() == [1]
    a, = E.scaled_ints(np.array([0.0625, 1024.0]))
    assert a.dtype == np.int64 and a.tolist() == [1, 16384]
    sq = [np.array([(0.0, 0.0), (4.0, 0.0), (4.0, 4.0), (0.0, 4.0), (0.0, 0.0)]), np.array([(1.0, 1.0), (1.0, 3.0), (3.0, 3.0), (3.0, 1.0), (1.0, 1.0)])]
    pos = E.point_positions([(0.5, 0.5), (2.0, 2.0), (1.0, 2.0), (4.0, 2.0), (5.0, 5.0), (np.nextafter(4.0, 5.0), 2.0)], [sq])[:, 0]
    assert pos.tolist() == [E.INSIDE, E.OUTSIDE, E.BOUNDARY, E.BOUNDARY, E.OUTSIDE, E.OUTSIDE]
    one = [np.array([(2.0, 2.0)])]
    assert not E.intersects([[sq[0]]], [one]) and E.intersects([[sq[0]]], [[np.array([(4.0, 4.0)])]])


@pytest.mark.parametrize("kind,G", E.POINT_POLY_INSTANCES)
def test_point_poly_fixture_selects_its_group_size(oracle, kind, G):
    fx = E.point_poly_fixture(kind, G)
    a = fx["array"]
    assert a.geom_type == kind and E.pick_group_rows(a.n_coords, a.n_geoms) == G
    lens = np.diff(a.ring_offsets)
    edges = lens[lens > 1] - 1
    if G > 1:
        assert {0, 1, G - 1} <= set((edges % G).tolist()), "ring edge counts 0, 1 and G - 1 modulo G"
    if G > 4:
        assert (lens[lens > 0] < G).any(), "rows shorter than G"
    assert 0.2 < fx["inside"].mean() and (fx["not_outside"] & ~fx["inside"]).sum() >= 20, "boundary points"
    pts = GeoArrowArray.from_points(fx["points"])
    for pred, key in (("within", "inside"), ("intersects", "not_outside")):
        got = oracle.predicate_rowwise(pts, a, pred, b_rows=fx["rows_of"])
        assert np.array_equal(got, fx[key]), pred


def _pairs_cols(pairs, kb=P):
    a = column(P, [A for _, A, _ in pairs])
    b = column(kb, [B for _, _, B in pairs])
    return a, b


def test_intersects_pairs_cross_every_switch(oracle):
    pairs = E.intersects_pairs()
    exp = np.array([E.intersects([A], [B]) for _, A, B in pairs])
    a, b = _pairs_cols(pairs)
    assert np.array_equal(oracle.predicate_rowwise(a, b, "intersects"), exp)
    assert np.array_equal(oracle.predicate_rowwise(b, a, "intersects"), exp)
    sizes = {(len(A[0]), len(B[0])) for _, A, B in pairs if len(A) == 1 and len(B) == 1}
    small = {s for s in sizes if E.small_form(1, s[0], 1, s[1])}
    assert {(66, 66), (1, 66), (66, 1)} <= small and (67, 66) in sizes - small and (66, 67) in sizes - small
    named = dict((n, e) for (n, _, _), e in zip(pairs, exp))
    assert named["comb:last_chunk:cross"] and named["comb:second_chunk:touch"] and not named["comb:last_chunk:ulp_below"]
    assert not named["comb:none:cross"] and not named["in_hole"] and named["in_polygon"] and not named["around"]
    assert not named["1x4:nested"] and not named["4x1:nested"], "geo: a one-coordinate ring has no segment endpoint"
    for n in ("comb:none:cross", "comb:last_chunk:cross"):  # more than PP_LIST in-window segments on both sides
        A, B = [p for p in pairs if p[0] == n][0][1:]
        assert min(len(A[0]), len(B[0])) > 3 * E.PP_LIST
    # valid pairs: geo's algorithm is the closed-set statement
    for name, A, B in pairs:
        if all(len(r) >= 4 and np.array_equal(r[0], r[-1]) for r in A + B) and len(A[0]) and "poking" not in name:
            assert E.intersects([A], [B]) == intersects_bruteforce(_open(A), _open(B)), name


def test_polygon_multipolygon_pairs(oracle):
    pairs = E.polygon_multi_pairs()
    exp = np.array([E.intersects([A], B) for _, A, B in pairs])
    assert exp.any() and not exp.all()
    a, b = _pairs_cols(pairs, MP)
    assert np.array_equal(oracle.predicate_rowwise(a, b, "intersects"), exp)
    assert np.array_equal(oracle.predicate_rowwise(b, a, "intersects"), exp)


@pytest.mark.parametrize("cus", CUS)
def test_join_at_scale_runs_four_candidates_a_group(cus):
    tpl = E.join_templates()
    per_tile = sum(sum(len(c) for c in t[2]) for t in tpl) / len(tpl)
    n_tiles = scale_tiles(tpl, cus)
    assert E.refine_per(int(per_tile * n_tiles), cus) >= 4
    for left, right, cands, hits in tpl:
        assert max(len(c) for c in cands) <= E.CAND_STAGE
        ring = [len(r[0]) for r in right]
        forms = [E.small_form(1, len(left[0][0]), 1, n) for n in ring]
        assert any(forms) and not all(forms)
        # some left row's run goes small -> general -> small
        for i, c in enumerate(cands):
            f = [E.small_form(1, len(left[i][0]), 1, ring[j]) for j in c]
            if any(not x and y for x, y in zip(f, f[1:])) and f[0]:
                break
        else:
            raise AssertionError("no run switches forms and back")
        assert any(h.any() for h in hits) and not all(h.all() for h in hits)


def scale_tiles(tpl, cus):
    """tiles for at least 4 candidates a refine group at this CU count"""
    per_tile = sum(sum(len(c) for c in t[2]) for t in tpl) / len(tpl)
    return int(np.ceil(4 * cus * 64 * 16 / per_tile)) + len(tpl)


def test_join_templates_against_the_oracle(oracle):
    tpl = E.join_templates()
    for hole in (False, True):
        left, right, pairs, counts, ccounts = E.tiled_join(tpl, 2 * len(tpl), hole_row=hole)
        got, gc, _ = oracle.spatial_join(left, right, "intersects")
        assert np.array_equal(got, pairs) and np.array_equal(gc, counts), hole
        assert E.cand_regime(int(ccounts.max())) == "staged"


def test_regime_join_counts(oracle):
    for counts, regime in (((16, 17, 48), "compact"), ((16, 17, 48, 49), "sorted")):
        left, right = E.regime_join(counts)
        cands = E.box_candidates([E.geom_box([l]) for l in left], [E.geom_box([r]) for r in right])
        assert [len(c) for c in cands] == list(counts) and E.cand_regime(max(counts)) == regime
        exp = [(i, j) for i, c in enumerate(cands) for j in c if E.intersects([left[i]], [right[j]])]
        got, _, _ = oracle.spatial_join(column(P, left), column(P, right), "intersects")
        assert [tuple(p) for p in got.tolist()] == exp


def test_contains_pairs(oracle):
    cases = E.contains_pairs()
    exp = {n: E.contains(A, B) for n, A, B in cases}
    assert exp["equal"] and exp["touch_exterior_inside"] and exp["touch_hole_outside"] and exp["around_hole_with_it"]
    assert not exp["is_the_hole"] and not exp["across_hole"] and not exp["around_hole"] and not exp["spans_members"]
    assert exp["inside_member_2"] and exp["member_hole"] is False
    a = column(MP, [A for _, A, _ in cases])
    b = column(P, [B[0] for _, _, B in cases])
    assert all(len(B) == 1 for _, _, B in cases)
    e = np.array([exp[n] for n, _, _ in cases])
    assert np.array_equal(oracle.predicate_rowwise(a, b, "contains"), e)
    assert np.array_equal(oracle.predicate_rowwise(b, a, "within"), e)
    ring_lens = {len(r) for _, A, B in cases for p in A + B for r in p}
    assert min(ring_lens) >= 33 and max(ring_lens) >= 200
