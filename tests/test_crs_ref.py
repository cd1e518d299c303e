"""The mpmath reference of the reprojection tests (tests/crs_ref.py) is pinned by facts it does not take from the Krueger series, and the
committed fixture (tests/golden/crs_reference.npz) is what that reference computes."""
import os

import numpy as np
import pytest

from tests import crs_ref as R

import mpmath  # noqa: E402
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crs_reference.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLD)


def test_central_meridian_on_the_equator_is_the_false_origin():
    for epsg, lon0, fn in ((32633, 15.0, 0.0), (32601, -177.0, 0.0), (32760, 177.0, 10000000.0)):
        x, y = R.mp_forward(epsg, lon0, 0.0)
        assert x == 500000 and y == fn


def test_pole_northing_is_k0_times_the_quarter_meridian():
    x, y = R.mp_forward(32633, 15.0, 90.0)
    assert x == 500000
    assert abs(y - mpmath.mpf("0.9996") * mpmath.mpf("10001965.729313")) < 1e-5  # the WGS84 quarter meridian, known to the micrometre


def test_web_mercator_square_world():
    pia = mpmath.mpf("20037508.342789243")
    x, y = R.mp_forward(3857, 180.0, 85.051128779806592)
    assert abs(x - pia) < 1e-8 and abs(y - pia) < 1e-7  # the latitude is given to 17 digits: 1e-15 degrees there are 1.3e-9 m
    lon, lat = R.mp_inverse(3857, pia, pia)
    assert abs(lon - 180) < 1e-14 and abs(lat - mpmath.mpf("85.051128779806592")) < 1e-14


@pytest.mark.parametrize("lon,lat", [(16.0, 10.0), (18.0, -33.0), (12.0, 60.0), (9.0, 5.0), (21.0, -70.0), (27.0, 45.0), (3.0, -45.0), (15.5, 89.0), (14.0, -0.5), (24.0, 80.0)])
def test_cauchy_riemann_off_the_meridian(lon, lat):
    """the projection is conformal: with the isometric latitude psi, N + iE is analytic in psi + i lam, so dN/dpsi = dE/dlam and
    dN/dlam = -dE/dpsi.  Central differences in 40 digits (step 1e-12 rad: truncation 1e-24 relative)"""
    mp = mpmath
    mp.mp.dps = 40
    h = mp.mpf(10) ** -12
    hd = mp.degrees(h)
    lon, lat = mp.mpf(lon), mp.mpf(lat)
    ep, np_ = R.mp_forward(32633, lon + hd, lat)
    em, nm = R.mp_forward(32633, lon - hd, lat)
    dE_dlam, dN_dlam = (ep - em) / (2 * h), (np_ - nm) / (2 * h)
    ep, np_ = R.mp_forward(32633, lon, lat + hd)
    em, nm = R.mp_forward(32633, lon, lat - hd)
    dpsi = R.mp_psi(mp.radians(lat + hd)) - R.mp_psi(mp.radians(lat - hd))
    dE_dpsi, dN_dpsi = (ep - em) / dpsi, (np_ - nm) / dpsi
    scale = abs(dE_dlam) + abs(dN_dlam)
    assert abs(dN_dpsi - dE_dlam) < 1e-18 * scale
    assert abs(dN_dlam + dE_dpsi) < 1e-18 * scale


@pytest.mark.parametrize("lat", [0.0, 30.0, -61.5, 89.0])
def test_scale_on_the_central_meridian_is_k0(lat):
    """across the meridian (the off-meridian code path): dE / (nu cos(phi) dlam) -> k0.  The scale grows as 1 + lam^2 cos^2(phi) / 2: at a step
    of 1e-8 rad that is 5e-17, and the quadrature's absolute error (1e-18 m) against a 1e-3..6e-2 m easting offset stays below 1e-15"""
    mp = mpmath
    mp.mp.dps = 40
    h = mp.mpf(10) ** -8
    e, _ = R.mp_forward(32633, 15 + mp.degrees(h), lat)
    a, e2, _ = R._consts(mp)
    phi = mp.radians(mp.mpf(lat))
    nu = a / mp.sqrt(1 - e2 * mp.sin(phi) ** 2)
    assert abs((e - 500000) / (nu * mp.cos(phi) * h) - mp.mpf("0.9996")) < 1e-14
    # along it: dN / (rho dphi)
    rho = a * (1 - e2) / (1 - e2 * mp.sin(phi) ** 2) ** mp.mpf(1.5)
    hd = mp.degrees(mp.mpf(10) ** -12)
    n1 = R.mp_forward(32633, 15.0, mp.mpf(lat) + hd)[1]
    n0 = R.mp_forward(32633, 15.0, mp.mpf(lat) - hd)[1]
    assert abs((n1 - n0) / (2 * mp.mpf(10) ** -12 * rho) - mp.mpf("0.9996")) < 1e-20


def test_inverse_undoes_forward():
    for epsg in (32633, 32733, 32601, 3395, 3857):
        lon0 = R.describe(epsg)[1]
        for dlon, lat in ((0.0, 0.0), (2.5, 47.0), (-11.0, -72.0), (7.0, 84.0)):
            x, y = R.mp_forward(epsg, lon0 + dlon, lat)
            lon, lat2 = R.mp_inverse(epsg, x, y)
            assert abs(R.mp_wrap180(lon - (lon0 + dlon))) < 1e-30 and abs(lat2 - lat) < 1e-30  # zone 1 reaches across the antimeridian


def test_fixture_rows_are_what_the_reference_computes(fx):
    """a random 100-row sample of every group, recomputed: the stored f64 is the rounded mp value (1e-12 m)"""
    rng = np.random.default_rng(7)
    for group, codes in R.FIXTURE_GROUPS.items():
        geo = fx[f"{group}_4326"]
        rows = rng.choice(len(geo), size=100 // len(R.FIXTURE_GROUPS) + 1, replace=False)
        for epsg in codes[1:]:
            img = fx[f"{group}_{epsg}"]
            for i in rows:
                if np.isnan(img[i]).any():
                    continue
                x, y = R.mp_forward(epsg, geo[i, 0], geo[i, 1])
                assert abs(float(x) - img[i, 0]) <= 1e-12 and abs(float(y) - img[i, 1]) <= 1e-12, (group, epsg, i)


def test_fixture_holds_the_hard_spots(fx):
    tm, world, anti = fx["tm_4326"], fx["world_4326"], fx["anti_4326"]
    assert any((tm == (15.0, 0.0)).all(axis=1))  # equator and central meridian exactly
    assert np.abs(tm[:, 1]).max() == 89.9 and np.abs(world[:, 1]).max() == 85.05
    assert tm[:, 0].min() == 3.0 and tm[:, 0].max() == 27.0 and (tm[:, 0] == 18.0).any() and (tm[:, 0] == 12.0).any()
    assert (tm[:, 1] < 0).any() and (tm[:, 1] > 0).any()
    assert (anti[:, 0] == 180.0).any() and (anti[:, 0] == -180.0).any() and (anti[:, 0] > 170).any() and (anti[:, 0] < -170).any()
    assert np.isfinite(fx["anti_32601"][anti[:, 0] > 171]).all(axis=1).any()  # zone 1 reached from east longitudes, across the antimeridian
    assert np.isfinite(fx["anti_32660"][anti[:, 0] < -171]).all(axis=1).any()
    assert fx["tm_32733"][:, 1].max() > 1.9e7 and np.nanmax(np.abs(fx["world_3857"])) > 2.0e7  # georeferenced magnitudes
    assert max(len(fx[k]) for k in fx.files) * 16 < 1 << 20


def test_numpy_restatement_of_the_series_stays_within_1e8_of_the_reference(fx):
    """the basis of the 1e-7 m tolerance: f64 evaluation of the n^6 series reaches the reference to a few ulp on every fixture row
    (rows where it does not were removed by the maker); the stored worst values are what this machine measures"""
    worst = dict(zip(fx["np_worst_names"].tolist(), fx["np_worst_m"].tolist()))
    cases = R.fixture_cases(fx)
    assert len(cases) == 42 and set(worst) == {c[0] for c in cases}
    for name, s, d, a, b in cases:
        assert len(a) >= 150, name
        err = R.error_metres(d, R.np_transform(s, d, a), b).max()
        assert err <= 1e-8, (name, err)
        assert abs(err - worst[name]) <= 4e-9, (name, err, worst[name])  # another libm may differ by an ulp of 2e7 m
