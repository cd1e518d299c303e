"""The exact reference of the Hausdorff and Frechet distances (tests/hausdorff_ref.py) pinned on known answers — the values PostGIS and
JTS document, checked with exact arithmetic — and the fixture tests/golden/hausdorff_lattice.npz (no GPU)."""
import math
import random
from fractions import Fraction as F

import numpy as np
import pytest

from tests import exact_ref as X
from tests import hausdorff_ref as H
from tests.golden import make_hausdorff_golden

LS = H.LS


def h(a, b, k=1):
    return float(X.dec_sqrt(H.hausdorff_exact(LS, a, LS, b, k)))


def f(a, b, k=1):
    return float(X.dec_sqrt(H.frechet_exact(a, b, k)))


def test_samples_are_the_contract_s_doubles():
    assert H.samples([(0, 0), (10, 7)], 1) == [(0.0, 0.0), (10.0, 7.0)]
    assert H.samples([(0, 0), (1, 7)], 3) == [(0.0, 0.0), (0.0 + 1.0 * (1.0 / 3.0), 0.0 + 1.0 * (7.0 / 3.0)), (0.0 + 2.0 * (1.0 / 3.0), 0.0 + 2.0 * (7.0 / 3.0)), (1.0, 7.0)]
    assert H.samples([(5, 5)], 4) == [(5.0, 5.0)] and H.samples([], 2) == []
    assert len(H.samples([(0, 0), (1, 0), (2, 0)], 7)) == 15
    assert len(H.row_samples(H.MLS, [[(0, 0), (1, 0)], [], [(3, 3)]], 4)) == 6 and len(H.row_samples(H.MPT, [(0, 0), (1, 1)], 4)) == 2


def test_known_answers():
    a, b = [(130, 0), (0, 0), (0, 150)], [(10, 10), (10, 150), (130, 10)]
    assert h(a, b) == 14.142135623730951 and h(a, b, H.densify_k(0.5)) == 70.0
    assert h([(0, 0), (100, 0), (10, 100), (10, 100)], [(0, 100), (0, 10), (80, 10)]) == 22.360679774997898
    assert f([(0, 0), (100, 0)], [(0, 0), (50, 50), (100, 0)]) == 70.71067811865476
    assert f([(0, 0), (100, 0)], [(0, 0), (50, 50), (100, 0)], H.densify_k(0.5)) == 50.0
    assert f([(0, 0), (10, 0)], [(10, 0), (0, 0)]) == 10.0 and h([(0, 0), (10, 0)], [(10, 0), (0, 0)]) == 0.0  # a line against its reverse
    assert H.directed_exact(LS, [(4, 1), (6, 1)], LS, [(0, 0), (10, 0)], 1) == 1
    assert float(X.dec_sqrt(H.directed_exact(LS, [(0, 0), (10, 0)], LS, [(4, 1), (6, 1)], 1))) == 4.123105625617661
    assert H.hausdorff_exact(LS, [], LS, [(0, 0)], 1) is None and H.frechet_exact([], [(0, 0)]) is None
    assert H.hausdorff_exact(H.PT, (3, 4), H.PT, (0, 0)) == 25 and H.hausdorff_exact(H.PT, None, H.PT, (0, 0)) is None


def test_frechet_is_at_least_hausdorff_and_the_two_tables_agree():
    rng = random.Random(3)
    for t in range(40):
        a = [(rng.randint(-20, 20), rng.randint(-20, 20)) for _ in range(rng.randint(1, 9))]
        b = [(rng.randint(-20, 20), rng.randint(-20, 20)) for _ in range(rng.randint(1, 9))]
        for k in (1, 2, 3):
            f2, h2 = H.frechet_exact(a, b, k), H.hausdorff_exact(LS, a, LS, b, k)
            assert f2 >= h2 and f2 == H.frechet_exact(b, a, k) and h2 == H.hausdorff_exact(LS, b, LS, a, k)
        assert H.frechet_exact(a, b, 1) == H.frechet_exact(a, b, 1, lattice=True)
        a2, b2 = [(2 * x, 2 * y) for x, y in a], [(2 * x, 2 * y) for x, y in b]
        assert H.frechet_exact(a2, b2, 2) == H.frechet_exact(a2, b2, 2, lattice=True) == 4 * H.frechet_exact(a, b, 2)
    z, y = H.zigzag(70, seed=1), H.zigzag(45, y0=3, seed=2)
    assert H.frechet_exact(z, y) == H.frechet_exact(z, y, lattice=True)


def test_preselection_agrees_with_brute_force():
    rng = random.Random(4)
    for kind_a, kind_b in ((H.PG, H.MLS), (H.MPG, H.MPT), (H.LS, H.PG)):
        for _ in range(5):
            ra, rb = H.random_row(rng, kind_a), H.random_row(rng, kind_b)
            for k in (1, 3):
                p = H.row_samples(kind_a, ra, k)
                s, e = H.P.segments(kind_b, rb)
                brute = max(min(X.point_segment_dist2(q, s[j], e[j]) for j in range(len(s))) for q in p)
                assert H.directed_exact(kind_a, ra, kind_b, rb, k) == brute


def test_densify_to_k():
    assert [H.densify_k(d) for d in (None, 1, 0.5, 0.25, 1 / 3, 1 / 7, 0.4, 1 / 4096)] == [1, 1, 2, 4, 3, 7, 2, 4096]  # 1 / 0.4 = 2.5 -> 2: half to even
    for bad in (0, -0.5, 1.5, float("nan"), float("inf"), 1 / 4097):
        with pytest.raises(ValueError):
            H.densify_k(bad)


def test_fixture_is_reproducible_byte_for_byte(tmp_path):
    out = tmp_path / "hausdorff_lattice.npz"
    make_hausdorff_golden.main(str(out))
    assert out.read_bytes() == open(H.GOLDEN, "rb").read()
    assert len(out.read_bytes()) < 64 * 1024


def test_recorded_answers_are_the_reference_s():
    z = np.load(H.GOLDEN)
    pairs = H.load_pairs(z)
    assert len(pairs) == len(H.KNOWN) + 21 * H.PAIRS_PER_FAMILY_PAIR
    assert {(p[1], p[3]) for p in pairs[len(H.KNOWN):]} == {(a, b) for i, a in enumerate(H.FAMILIES.values()) for b in list(H.FAMILIES.values())[i:]}
    for k in H.FIXTURE_KS:
        for i, (name, ka, ra, kb, rb) in enumerate(pairs):
            num, den = (int(v) for v in z[f"hausdorff2_k{k}"][i])
            assert H.hausdorff_exact(ka, ra, kb, rb, k) == F(num, den), (name, k)
            num, den = (int(v) for v in z[f"frechet2_k{k}"][i])
            if ka == LS and kb == LS:
                assert H.frechet_exact(ra, rb, k) == F(num, den), (name, k)
            else:
                assert den == 0
    by_name = {p[0]: i for i, p in enumerate(pairs)}
    assert math.sqrt(z["hausdorff2_k1"][by_name["postgis_1"]][0]) == 14.142135623730951 and tuple(z["hausdorff2_k2"][by_name["postgis_1"]]) == (4900, 1)
    assert tuple(z["hausdorff2_k1"][by_name["identical"]]) == (0, 1) and tuple(z["frechet2_k1"][by_name["reversed"]]) == (100, 1)
