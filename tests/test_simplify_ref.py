"""CPU: the oracle's simplify (oracle/gpk_oracle.c, the kernel's algorithm written a second time) against the exact reference of
tests/simplify_ref.py — geo 0.27's compute_rdp on rationals — for all four families, on randomized lattice columns (unsettled share
asserted first), on the deliberate tie families (nothing excluded: every float decision there is exact), on rings whose answer
depends on the order of the walk, and against properties that owe nothing to the recursion."""
import math

import numpy as np
import pytest

from geopolars_amd import synth
from tests import simplify_ref as R

LS, MLS, PG, MPG = R.LS, R.MLS, R.PG, R.MPG


def _both(oracle, a, eps, cap=R.CAP, what="", every=1):
    xy, off = oracle.simplify(a, eps)
    share, res = R.compare_exact(a, eps, xy, off, cap=cap, what=what)
    R.check_properties(a, eps, xy, off, every=every, what=what)
    return xy, off, share, res


def test_the_two_f64_evaluations_are_the_same_operations():
    rng = np.random.default_rng(5)
    for scale in (1.0, 2.0**30, 2.0**-60):
        p = rng.integers(-50, 51, (400, 2)).astype(np.float64) * scale
        for s, e in ((p[0], p[1]), (p[2], p[2]), (p[3], p[3] + scale), (rng.normal(0, 1, 2), rng.normal(0, 1, 2))):
            q = np.concatenate([p, rng.normal(0, 30, (100, 2)) * scale, [s, e, (s + e) / 2]])
            many = R.seg_dist_f64_many(q, s, e)
            one = [R.seg_dist_f64(float(x), float(y), float(s[0]), float(s[1]), float(e[0]), float(e[1])) for x, y in q]
            assert many.tolist() == one


def test_group_size_mirrors_the_dispatch():
    assert [R.simplify_group_size(c, s) for c, s in ((0, 0), (0, 5), (48, 1), (49, 1), (480, 10), (481, 10), (20_000, 1))] == [0, 8, 8, 64, 8, 64, 64]
    for G in (8, 64):
        for seqs in ([R.tie_line(5, [1, 3])], [R.BALLAST], [[], [(0.0, 0.0)]]):
            assert R.group_size_of(R.as_column(LS, R.force_instance(seqs, G))) == G


@pytest.mark.parametrize("kind", [LS, MLS, PG, MPG])
def test_oracle_matches_the_rationals_on_lattice_columns(oracle, kind):
    a = R.lattice_column(kind, 120, seed=20 + kind)
    assert len(R.sequences(a)) == 120
    shares = {}
    for eps in R.LATTICE_EPS:
        _, _, shares[eps], res = _both(oracle, a, eps, what=f"lattice {kind}")
    print(f"lattice kind {kind}: unsettled share {shares}, sequences with an exact tie {sum(r.ties > 0 for r in res)} / {len(res)}")
    if kind in (PG, MPG):  # the ring rule is at work: some ring met the floor
        assert any(r.refused_ranges for r in [R.rdp_cached(s, 1e9, 4) for s in R.sequences(a)])


def test_lattice_columns_nest_every_family(oracle):
    mls, mpg = R.lattice_column(MLS, 40, 1), R.lattice_column(MPG, 40, 2)
    assert mls.ring_offsets is not None and np.any(np.diff(mls.geom_offsets) == 0) and np.any(np.diff(mls.geom_offsets) > 1)
    assert np.any(np.diff(mpg.geom_offsets) > 1) and np.any(np.diff(mpg.part_offsets) > 1)  # several members, holes
    null = R.as_column(MPG, R.lattice_sequences(40, 2, ring=True), null_every=3)
    assert not null.is_valid().all()
    a, b = oracle.simplify(mpg, 7.0), oracle.simplify(null, 7.0)  # null rows keep their coordinates and are simplified like the rest
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_oracle_on_the_tie_families(oracle):
    n_ties = n_eps = 0
    for kind, fam in ((LS, R.tie_family_lines()), (MLS, R.tie_family_lines()), (PG, R.tie_family_rings()), (MPG, R.tie_family_rings())):
        for eps in sorted({e for _, _, es in fam for e in es}):
            seqs = [s for _, s, es in fam if eps in es]
            _, _, share, res = _both(oracle, R.as_column(kind, seqs), eps, cap=0.0, what=f"ties {kind} {eps}")
            n_ties += sum(r.ties for r in res)
            n_eps += sum(r.eps_ties for r in res)
    assert n_ties > 400 and n_eps > 40  # the families do tie, with each other and with the threshold


def test_tie_lines_answer_as_designed(oracle):
    h = 0.25
    below = math.nextafter(h, 0.0)
    for n in (5, 9, 17, 40):
        for (k1, k2) in R.tie_pairs(n, 8).values():
            line = R.tie_line(n, [k1, k2])
            a = R.as_column(LS, [line])
            assert R.rdp_exact(line, h, 2).keep.nonzero()[0].tolist() == [0, n - 1]  # eps == d: closed threshold, no split
            assert R.rdp_exact(line, below, 2).keep.nonzero()[0].tolist() == [0, k2, n - 1]  # the LAST of the tied points
            assert oracle.simplify(a, h)[1].tolist() == [0, 2] and oracle.simplify(a, below)[0].tolist() == [list(line[0]), list(line[k2]), list(line[-1])]
    for eps in (math.inf, math.nan):  # nothing is `> eps`: cull down to min_pts
        xy, off = oracle.simplify(R.as_column(LS, [R.tie_line(9, [2, 5]), R.BALLAST]), eps)
        assert off.tolist() == [0, 2, 4]
        ring = R.circle_ring()
        xy, off, _, res = _both(oracle, R.as_column(PG, [ring, R.sliver_ring(5, 7)]), eps, cap=0.0)
        assert off.tolist() == [0, len(ring), len(ring) + 15] and res[0].refused_ranges == 1  # a ring cannot go below 4: the one range is refused
    for eps in (0.0, -1.0, -math.inf):
        xy, off = oracle.simplify(R.as_column(LS, [R.tie_line(9, [2, 5])]), eps)
        assert off.tolist() == [0, 9]


def test_rings_whose_answer_depends_on_the_order(oracle):
    differ = 0
    for name, ring in R.order_rings():
        outs = []
        for r in (ring, ring[::-1]):
            for kind in (PG, MPG):
                xy, off, _, res = _both(oracle, R.as_column(kind, [r, r]), R.ORDER_EPS, cap=0.0, what=name)
                _both(oracle, R.as_column(kind, [r]), 1e300, cap=0.0, what=name)
            outs.append((xy[: off[1]].tolist(), res[0]))
        (fwd, rf), (bwd, rb) = outs
        if name.startswith("sliver"):
            m_left, m_right = (int(v) for v in name.split()[1].split("+"))
            # the left range settles first and culls; the right one would leave 3 coordinates and is refused
            assert (rf.culled_ranges, rf.refused_ranges) == (1, 1) and len(fwd) == len(ring) - m_left
            assert (rb.culled_ranges, rb.refused_ranges) == (1, 1) and len(bwd) == len(ring) - m_right
        if fwd != bwd[::-1]:
            differ += 1
        if name in ("triangle", "five", "identical"):
            xy, off = oracle.simplify(R.as_column(PG, [ring]), 1e300)
            assert xy.tolist() == [list(p) for p in ring]  # a very large eps culls nothing from a ring this short
    assert differ >= 7
    # the doc example of Polygon::simplify and the sliver of test_oracle_lineal_ops
    _both(oracle, R.as_column(PG, [[(0, 0), (0, 10), (5, 11), (10, 10), (10, 0), (0, 0)]]), 2.0, cap=0.0)
    _both(oracle, R.as_column(PG, [[(0, 0), (10, 0), (10, 0.1), (5, 0.2), (0, 0.1), (0, 0)]]), 5.0, cap=0.0)


def test_hand_cases_of_geo_against_the_rationals(oracle):
    doc = [(0.0, 0.0), (5.0, 4.0), (11.0, 5.5), (17.3, 3.2), (27.8, 0.1)]
    assert R.rdp_exact(doc, 1.0, 2).keep.tolist() == [True, True, True, False, True]
    tie = [(0, 0), (2, 3), (4, 3), (6, 0)]
    assert R.rdp_exact(tie, 1.0, 2).keep.all() and R.rdp_exact(tie, 1.0, 2).ties == 1
    for seqs, eps in (([doc], 1.0), ([tie], 1.0), ([tie], 0.0), ([[(0, 0), (1, 1)], [(5, 5)], []], 10.0)):
        for kind in (LS, MLS):
            _both(oracle, R.as_column(kind, seqs), eps, cap=0.0)


def test_deep_walks(oracle):
    for n, eps, depth in ((50, 0.25, 48), (2000, 0.25, 1998), (2000, 250.0, 1000), (2000, 1e9, 0)):
        sp = R.square_spiral(n)
        _, _, _, res = _both(oracle, R.as_column(LS, [sp]), eps, cap=0.0)
        assert res[0].depth >= depth


@pytest.mark.parametrize("eps", [0.05, 4.0])
def test_properties_on_the_float_columns_of_the_gpu_test(oracle, eps):
    """the columns of test_simplify_parity: the oracle's output keeps the properties (a sample of the sequences); the exact
    reference judges those it is entitled to — on random floats that is nearly all of them"""
    for a, every in ((synth.random_linestrings(300), 3), (synth.clustered_polygons(300, seed=8), 3), (synth.powerlaw_multipolygons(150), 2)):
        xy, off = oracle.simplify(a, eps)
        R.check_properties(a, eps, xy, off, every=every)
        share, _ = R.compare_exact(a, eps, xy, off)
        assert share <= 0.01
