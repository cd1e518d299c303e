"""Reference for the analytic reprojection (csrc/gpk_crs.h), independent of the Krueger series.

Two things live here:

* the mpmath reference (40 digits).  Transverse Mercator comes from its definition: with the isometric latitude
  psi(phi) = atanh(sin phi) - e atanh(e sin phi), the projection is the analytic function that maps zeta = psi(phi) + i (lam - lam0)
  to w = k0 M(phi_c), where phi_c is the COMPLEX latitude with psi(phi_c) = zeta and M(phi) = a (1 - e^2) int_0^phi (1 - e^2 sin^2 t)^(-3/2) dt
  is the meridian arc (on the central meridian this is the definition itself: true to scale k0, northing = k0 * arc).  psi(phi_c) = zeta is
  solved with findroot from the Gudermannian of zeta, the integral is mp.quad along the straight complex path.  Easting offset = Im w,
  northing = Re w.  The inverse runs Newton on the same two maps (their derivatives are closed forms).  Both Mercators are their closed forms.
* `np_transform`: a plain numpy restatement of the n^6 series, for the benchmark's CPU line and for measuring what f64 can reach.
"""
from __future__ import annotations

import math

import numpy as np

A = 6378137.0
INV_F = 298.257223563
K0 = 0.9996
GEOG, WEBMERC, MERC, TMERC = 0, 1, 2, 3


def describe(epsg: int):
    """(kind, lon0 degrees, false easting, false northing) of a supported EPSG code"""
    if epsg == 4326:
        return GEOG, 0.0, 0.0, 0.0
    if epsg == 3857:
        return WEBMERC, 0.0, 0.0, 0.0
    if epsg == 3395:
        return MERC, 0.0, 0.0, 0.0
    if 32601 <= epsg <= 32660:
        return TMERC, 6.0 * (epsg - 32600) - 183.0, 500000.0, 0.0
    if 32701 <= epsg <= 32760:
        return TMERC, 6.0 * (epsg - 32700) - 183.0, 500000.0, 10000000.0
    raise ValueError(f"EPSG:{epsg} is not in the analytic set")


# ---- mpmath ----------------------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath

    mpmath.mp.dps = 40
    return mpmath


def _consts(mp):
    f = 1 / mp.mpf("298.257223563")
    e2 = f * (2 - f)
    return mp.mpf(6378137), e2, mp.sqrt(e2)


def mp_psi(phi):
    """isometric latitude; real or complex phi"""
    mp = _mp()
    _, _, e = _consts(mp)
    s = mp.sin(phi)
    return mp.atanh(s) - e * mp.atanh(e * s)


def mp_meridian(phi):
    """meridian arc M(phi), the integral taken along the straight path 0 -> phi (phi may be complex)"""
    mp = _mp()
    a, e2, _ = _consts(mp)
    return a * (1 - e2) * phi * mp.quad(lambda u: (1 - e2 * mp.sin(phi * u) ** 2) ** mp.mpf(-1.5), [0, 1])


def mp_wrap180(d):
    mp = _mp()
    d = mp.mpf(d)
    while d > 180:
        d -= 360
    while d < -180:
        d += 360
    return d


def mp_tm_forward(lon, lat, lon0, fe=500000.0, fn=0.0):
    """(easting, northing) as mpf; lon, lat in degrees (floats are taken exactly)"""
    mp = _mp()
    phi = mp.radians(mp.mpf(lat))
    dl = mp.radians(mp_wrap180(mp.mpf(lon) - mp.mpf(lon0)))
    if dl == 0:
        return mp.mpf(fe), mp.mpf(fn) + K0mp(mp) * mp_meridian(phi)
    zeta = mp.mpc(mp_psi(phi), dl)
    gd = 2 * mp.atan(mp.tanh(zeta / 2))
    phic = mp.findroot(lambda p: mp_psi(p) - zeta, gd, tol=mp.mpf(10) ** -36, maxsteps=60)
    w = K0mp(mp) * mp_meridian(phic)
    return mp.mpf(fe) + w.imag, mp.mpf(fn) + w.real


def K0mp(mp):
    return mp.mpf("0.9996")


def mp_tm_inverse(x, y, lon0, fe=500000.0, fn=0.0):
    """(lon, lat) degrees as mpf: Newton on w = k0 M(phi_c), then on psi(phi) = Re psi(phi_c)"""
    mp = _mp()
    a, e2, e = _consts(mp)
    w = mp.mpc(mp.mpf(y) - mp.mpf(fn), mp.mpf(x) - mp.mpf(fe)) / K0mp(mp)
    phic = w / a
    for _ in range(60):
        d = (mp_meridian(phic) - w) / (a * (1 - e2) * (1 - e2 * mp.sin(phic) ** 2) ** mp.mpf(-1.5))
        phic -= d
        if abs(d) < mp.mpf(10) ** -37:
            break
    zeta = mp_psi(phic)
    phi = 2 * mp.atan(mp.tanh(zeta.real / 2))
    for _ in range(60):
        d = (mp_psi(phi) - zeta.real) * (1 - e2 * mp.sin(phi) ** 2) * mp.cos(phi) / (1 - e2)  # psi' = (1-e^2) / ((1 - e^2 sin^2) cos)
        phi -= d
        if abs(d) < mp.mpf(10) ** -37:
            break
    return mp_wrap180(mp.mpf(lon0) + mp.degrees(zeta.imag)), mp.degrees(phi)


def mp_forward(epsg: int, lon, lat):
    """geographic degrees -> (x, y) of `epsg`, mpf"""
    mp = _mp()
    a, _, e = _consts(mp)
    kind, lon0, fe, fn = describe(epsg)
    if kind == GEOG:
        return mp_wrap180(lon), mp.mpf(lat)
    if kind == TMERC:
        return mp_tm_forward(lon, lat, lon0, fe, fn)
    phi = mp.radians(mp.mpf(lat))
    x = a * mp.radians(mp_wrap180(lon))
    if kind == WEBMERC:
        return x, a * mp.asinh(mp.tan(phi))
    return x, a * (mp.asinh(mp.tan(phi)) - e * mp.atanh(e * mp.sin(phi)))


def mp_inverse(epsg: int, x, y):
    """(x, y) of `epsg` -> geographic degrees, mpf"""
    mp = _mp()
    a, e2, e = _consts(mp)
    kind, lon0, fe, fn = describe(epsg)
    if kind == GEOG:
        return mp_wrap180(x), mp.mpf(y)
    if kind == TMERC:
        return mp_tm_inverse(x, y, lon0, fe, fn)
    lon = mp_wrap180(mp.degrees(mp.mpf(x) / a))
    psi = mp.mpf(y) / a
    phi = 2 * mp.atan(mp.tanh(psi / 2))
    if kind == MERC:
        for _ in range(60):
            d = (mp_psi(phi) - psi) * (1 - e2 * mp.sin(phi) ** 2) * mp.cos(phi) / (1 - e2)
            phi -= d
            if abs(d) < mp.mpf(10) ** -37:
                break
    return lon, mp.degrees(phi)


# ---- numpy restatement of the n^6 series -----------------------------------------------------------------------------------------
_F = 1.0 / INV_F
_E2 = _F * (2.0 - _F)
_E = math.sqrt(_E2)
_E2M = 1.0 - _E2
_N = _F / (2.0 - _F)


def krueger(n: float = _N):
    """(alpha[6], beta[6], rectifying radius): Karney (2011) eqs. 35, 36 and 14"""
    n2, n3, n4, n5, n6 = n**2, n**3, n**4, n**5, n**6
    alp = [
        n / 2 - 2 * n2 / 3 + 5 * n3 / 16 + 41 * n4 / 180 - 127 * n5 / 288 + 7891 * n6 / 37800,
        13 * n2 / 48 - 3 * n3 / 5 + 557 * n4 / 1440 + 281 * n5 / 630 - 1983433 * n6 / 1935360,
        61 * n3 / 240 - 103 * n4 / 140 + 15061 * n5 / 26880 + 167603 * n6 / 181440,
        49561 * n4 / 161280 - 179 * n5 / 168 + 6601661 * n6 / 7257600,
        34729 * n5 / 80640 - 3418889 * n6 / 1995840,
        212378941 * n6 / 319334400,
    ]
    bet = [
        n / 2 - 2 * n2 / 3 + 37 * n3 / 96 - n4 / 360 - 81 * n5 / 512 + 96199 * n6 / 604800,
        n2 / 48 + n3 / 15 - 437 * n4 / 1440 + 46 * n5 / 105 - 1118711 * n6 / 3870720,
        17 * n3 / 480 - 37 * n4 / 840 - 209 * n5 / 4480 + 5569 * n6 / 90720,
        4397 * n4 / 161280 - 11 * n5 / 504 - 830251 * n6 / 7257600,
        4583 * n5 / 161280 - 108847 * n6 / 3991680,
        20648693 * n6 / 638668800,
    ]
    return alp, bet, A / (1 + n) * (1 + n2 / 4 + n4 / 64 + n6 / 256)


def _wrap180(d):
    return np.where(d > 180.0, d - 360.0, np.where(d < -180.0, d + 360.0, d))


def _taup(tau):
    tau1 = np.hypot(1.0, tau)
    sig = np.sinh(_E * np.arctanh(_E * tau / tau1))
    return tau * np.hypot(1.0, sig) - sig * tau1


def _tau(taup):
    tau = taup / _E2M
    for _ in range(4):
        tpa = _taup(tau)
        tau = tau + (taup - tpa) * (1.0 + _E2M * tau * tau) / (_E2M * np.hypot(1.0, tau) * np.hypot(1.0, tpa))
    return tau


def _series(c, xi, eta):
    dxi = np.zeros_like(xi)
    deta = np.zeros_like(xi)
    for j, cj in enumerate(c, start=1):
        dxi = dxi + cj * np.sin(2 * j * xi) * np.cosh(2 * j * eta)
        deta = deta + cj * np.cos(2 * j * xi) * np.sinh(2 * j * eta)
    return dxi, deta


def np_to_geographic(epsg: int, x, y):
    """(lon, lat) degrees; float64 arrays"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    kind, lon0, fe, fn = describe(epsg)
    if kind == GEOG:
        return x, y
    if kind == TMERC:
        alp, bet, ar = krueger()
        xi, eta = (y - fn) / (K0 * ar), (x - fe) / (K0 * ar)
        dxi, deta = _series(bet, xi, eta)
        xip, etap = xi - dxi, eta - deta
        sh, cx = np.sinh(etap), np.cos(xip)
        tau = _tau(np.sin(xip) / np.hypot(sh, cx))
        return lon0 + np.degrees(np.arctan2(sh, cx)), np.degrees(np.arctan(tau))
    tau = np.sinh(y / A)
    if kind == MERC:
        tau = _tau(tau)
    return np.degrees(x / A), np.degrees(np.arctan(tau))


def np_from_geographic(epsg: int, lon, lat):
    lon = np.asarray(lon, dtype=np.float64)
    lat = np.asarray(lat, dtype=np.float64)
    kind, lon0, fe, fn = describe(epsg)
    if kind == GEOG:
        return _wrap180(lon), lat
    tau = np.tan(np.radians(lat))
    if kind == TMERC:
        alp, bet, ar = krueger()
        lam = np.radians(_wrap180(lon - lon0))
        taup = _taup(tau)
        cl = np.cos(lam)
        xip, etap = np.arctan2(taup, cl), np.arcsinh(np.sin(lam) / np.hypot(taup, cl))
        dxi, deta = _series(alp, xip, etap)
        return fe + K0 * ar * (etap + deta), fn + K0 * ar * (xip + dxi)
    x = A * np.radians(_wrap180(lon))
    return x, A * np.arcsinh(tau if kind == WEBMERC else _taup(tau))


def np_transform(src_epsg: int, dst_epsg: int, xy):
    """the whole transform on an (n, 2) float64 array (no failure rules: the caller stays inside the domain)"""
    xy = np.asarray(xy, dtype=np.float64)
    lon, lat = np_to_geographic(src_epsg, xy[:, 0], xy[:, 1])
    x, y = np_from_geographic(dst_epsg, lon, lat)
    return np.stack([x, y], axis=1)


# ---- comparing ---------------------------------------------------------------------------------------------------------------------
def error_metres(dst_epsg: int, got, want):
    """per-row error in metres of `got` against `want` ((n, 2) arrays in the destination system): absolute for projected systems,
    ground distance a * hypot(dphi, cos(phi) dlam) for geographic ones (longitude is ill-conditioned near the poles)"""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    if describe(dst_epsg)[0] != GEOG:
        return np.max(np.abs(got - want), axis=1)
    dlam = np.radians(_wrap180(got[:, 0] - want[:, 0]))
    dphi = np.radians(got[:, 1] - want[:, 1])
    return A * np.hypot(dphi, np.cos(np.radians(want[:, 1])) * dlam)


# ---- the fixture (tests/golden/crs_reference.npz, written by tests/golden/make_crs_golden.py) ---------------------------------------
# group -> the systems its geographic points have images in (key f"{group}_{epsg}", (n, 2) float64; NaN rows are outside that
# system's pinned domain: more than 12 degrees from a UTM central meridian, beyond 85.05 degrees of latitude for a Mercator)
FIXTURE_GROUPS = {
    "world": (4326, 3857, 3395),
    "tm": (4326, 32633, 32733, 32634, 3857, 3395),
    "anti": (4326, 32601, 32660),
}
TOL_M = 1e-7  # metres, against the mp reference


def fixture_cases(fx):
    """every ordered pair of systems of every group: (name, src_epsg, dst_epsg, src_xy, want_xy), rows both systems pin"""
    out = []
    for group, codes in FIXTURE_GROUPS.items():
        for s in codes:
            for d in codes:
                if s == d:
                    continue
                a, b = fx[f"{group}_{s}"], fx[f"{group}_{d}"]
                ok = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)
                out.append((f"{group}:{s}->{d}", s, d, np.ascontiguousarray(a[ok]), np.ascontiguousarray(b[ok])))
    return out
