"""The mpmath reference of the geodesic measures (tests/geodesic_measure_ref.py) against closed forms and its own symmetries, and the
committed fixture against a regenerated sample — bit for bit."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

from tests import geodesic_measure_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_geodesic_golden as G  # noqa: E402

QUARTER_MERIDIAN = mp.mpf("10001965.7293127")


@pytest.fixture(autouse=True)
def thirty_digits():
    """the tests' own arithmetic on the reference's values, at the reference's precision"""
    with mp.workdps(R.DPS):
        yield


def close(a, b, tol):
    return abs(mp.mpf(a) - mp.mpf(b)) <= tol


def test_constants():
    assert close(R.C2, "40589732499314.75999814", 1e-7) and close(R.q_of_sinphi(mp.mpf(1)), R.C2, 1e-15)
    assert close(R.AREA0, "510065621724088.5093", 1e-3)
    assert close(R.inverse(0, 0, 0, 90)["s12"], QUARTER_MERIDIAN, 1e-6)


def test_closed_form_rings():
    octant, per = R.ring_measures([(0, 0), (90, 0), (0, 90), (0, 0)])
    assert close(octant, "63758202715511.0637", 1e-3) and close(octant, R.C2 * mp.pi / 2, 1e-12)
    assert close(per, R.A * mp.pi / 2 + 2 * R.inverse(0, 0, 0, 90)["s12"], 1e-15)
    for d in (10, 170, 179):  # (0, 0), (d, 0), the pole: d <= (1 - f) * 180, so the equator is the geodesic
        area, per = R.ring_measures([(0, 0), (d, 0), (0, 90), (0, 0)])
        assert close(area, R.C2 * d * R.DEG, 1e-12) and close(per, R.A * d * R.DEG + 2 * QUARTER_MERIDIAN, 1e-6)
    for l1, l2 in ((0, 30), (170, -175)):  # a lune between two meridians
        area, _ = R.ring_measures([(l1, 90), (l1, 0), (l2, -90), (l2, 0), (l1, 90)])
        assert close(area, 2 * R.C2 * ((l2 - l1) % 360) * R.DEG, 1e-12)


def test_line_integral_equals_the_i4_form():
    """the area under an arc two ways: int q d lambda, and Karney's S(sig2) - S(sig1) with I4 by quadrature"""
    for lat, azi, arc in ((30, 50, 1), (-10, 120, 2.5), (60, 10, mp.mpf("0.001"))):
        sb, cb = R._beta(lat)
        L = R.Line(sb, cb, mp.sin(azi * R.DEG), mp.cos(azi * R.DEG))
        assert abs(L.area(L.sig1 + arc) - L.i4_form(L.sig1 + arc)) <= mp.mpf("1e-15")


def test_reversal_and_midpoint_split():
    ring = [(10.0, 20.0), (40.0, 25.0), (35.0, 50.0), (5.0, 45.0), (10.0, 20.0)]
    area, per = R.ring_measures(ring)
    back, per2 = R.ring_measures(ring[::-1])
    assert area > 0 and close(back, -area, 1e-12) and close(per, per2, 1e-18)
    e = R.inverse(*ring[0], *ring[1])
    lon, lat, azi, _ = R.direct(ring[0][0], ring[0][1], e["azi1"], e["s12"] / 2)  # the midpoint of the first edge
    halves = [R.inverse(ring[0][0], ring[0][1], lon, lat), R.inverse(lon, lat, *ring[1])]
    assert close(halves[0]["S12"] + halves[1]["S12"], e["S12"], 1e-10) and close(halves[0]["s12"] + halves[1]["s12"], e["s12"], 1e-18)
    assert close(halves[0]["azi2"], halves[1]["azi1"], 1e-22) and close(halves[1]["azi2"], e["azi2"], 1e-22)
    far = R.direct(ring[0][0], ring[0][1], e["azi1"], e["s12"])
    assert close(far[0], ring[1][0], 1e-20) and close(far[1], ring[1][1], 1e-20) and close(far[2], e["azi2"], 1e-20)


def test_polar_and_antimeridian_rings():
    cap, _ = R.ring_measures([(0, 80), (120, 80), (-120, 80), (0, 80)])  # eastwards around the north pole: the cap is to the left
    assert 0 < cap < 4e12
    south, _ = R.ring_measures([(0, -80), (120, -80), (-120, -80), (0, -80)])  # eastwards around the south pole: everything but the cap
    assert close(south, -cap, 1e-12)  # ... which reduces to minus the cap
    a, _ = R.ring_measures([(179, 0), (-179, 0), (-179, 1), (179, 1), (179, 0)])
    b, _ = R.ring_measures([(-1, 0), (1, 0), (1, 1), (-1, 1), (-1, 0)])
    assert a > 0 and close(a, b, 1e-10)


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture(os.path.join(HERE, "golden", "geodesic_measures_mp.npz"))


def test_fixture_shape_and_inputs(fixture):
    fx = fixture
    exy, ereg = G.edge_cases()
    rxy, roff, rreg = G.ring_cases()
    assert np.array_equal(fx["edge_xy"], exy) and np.array_equal(fx["edge_regime"], ereg) and np.array_equal(fx["direct_in"], G.direct_cases())
    assert np.array_equal(fx["ring_xy"], rxy) and np.array_equal(fx["ring_off"], roff) and np.array_equal(fx["ring_regime"], rreg)
    assert len(exy) == 3000 and len(fx["direct_in"]) == 600 and len(roff) - 1 == 300 and set(ereg) == set(range(len(R.EDGE_REGIMES)))
    assert set(rreg) == set(range(len(R.RING_REGIMES))) and np.diff(roff).max() > 1500
    assert os.path.getsize(os.path.join(HERE, "golden", "geodesic_measures_mp.npz")) < 300 * 1024
    assert np.isnan(fx["edge_S12"]).sum() == (ereg == R.EDGE_REGIMES.index("over_pole")).sum()  # only there is S12 a convention
    assert (np.sign(fx["ring_area"]) > 0).sum() > 100 and (np.sign(fx["ring_area"]) < 0).sum() > 100  # both windings


def test_fixture_sample_regenerates_bit_for_bit(fixture):
    fx = fixture
    rng = np.random.default_rng(9)
    for i in sorted(set(rng.integers(0, len(fx["edge_xy"]), 27)) | {int(np.flatnonzero(fx["edge_regime"] == k)[0]) for k in range(len(R.EDGE_REGIMES))})[:32]:
        s12, azi1, azi2, m12, S12 = G.edge_record(fx["edge_xy"][i])
        got = np.array([s12, azi1, azi2, S12]), np.array([fx["edge_s12"][i], fx["edge_azi1"][i], fx["edge_azi2"][i], fx["edge_S12"][i]])
        assert np.array_equal(got[0], got[1], equal_nan=True) and np.float32(m12) == fx["edge_m12"][i], i
    for i in (0, 7, 301, 599):
        assert np.array_equal(G.direct_record(fx["direct_in"][i]), fx["direct_out"][i]), i
    small = [int(np.flatnonzero(fx["ring_regime"] == k)[0]) for k in (0, 2, 4, 5, 6)]  # (not the dense ones: seconds, not minutes)
    for i in small:
        a, b = fx["ring_off"][i], fx["ring_off"][i + 1]
        assert G.ring_record(fx["ring_xy"][a:b]) == (fx["ring_area"][i], fx["ring_perimeter"][i]), i
