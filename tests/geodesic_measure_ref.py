"""TEST INFRASTRUCTURE: an mpmath reference for the geodesic measures of csrc/gpk_geodesic.h (inverse with azimuths, reduced length and
the area under an edge; direct; ring area and perimeter) on WGS84, at 30 digits, sharing NOTHING with the series of the header.

Bessel's reduction, as oracle/geodesic_quadrature.py states it: a geodesic is a great circle on the auxiliary sphere (reduced latitude
beta, tan beta = (1 - f) tan phi; Clairaut sin alpha cos beta = sin alpha0; k^2 = e'^2 cos^2 alpha0),

    s      = b * int sqrt(1 + k^2 sin^2 sigma) d sigma
    lambda = omega - f sin alpha0 * int (2 - f) / (1 + (1 - f) sqrt(1 + k^2 sin^2 sigma)) d sigma
    m12/b  = sqrt(1 + k^2 sin^2 sig2) cos sig1 sin sig2 - sqrt(1 + k^2 sin^2 sig1) sin sig1 cos sig2 - cos sig1 cos sig2 (J(sig2) - J(sig1)),
             J = int k^2 sin^2 sigma / sqrt(1 + k^2 sin^2 sigma) d sigma

every integral by mpmath quadrature.  DIRECT: sigma2 from s by Newton's method on the first integral.  INVERSE: in the canonical
arrangement (|phi1| >= |phi2|, phi1 <= 0, 0 <= lambda12 <= pi) lambda12(alpha1) increases on [0, pi] (Karney 2013, section 5): a bracketed
root search, which finds the SHORTEST geodesic, nearly antipodal points included.

AREA from first principles: in the equal-area cylindrical map x = lambda, y = q(phi), q(phi) = (b^2 / 2) (sin phi / (1 - e^2 sin^2 phi) +
atanh(e sin phi) / e), the area between an edge and the equator is S12 = int q d lambda along the edge, with
d lambda / d sigma = sin alpha0 / cos^2 beta - f sin alpha0 (2 - f) / (1 + (1 - f) sqrt(1 + k^2 sin^2 sigma)); at a pole the longitude
jumps, which contributes q(pole) * (the jump).  A ring's area to the left of its direction of travel is
-(sum of S12) + q(90) * (sum of the signed longitude steps) — the second term is the shift of q by -+q(90) for a ring that winds
around a pole, zero otherwise — reduced to (-A0 / 2, A0 / 2].  i4_form() is Karney's S(sig2) - S(sig1) with I4 by quadrature: the cross-check.

The named tolerances at the end are MEASURED: the worst error of the header run on the CPU (tests/geodesic_host_driver.cpp) against the
fixture tests/golden/geodesic_measures_mp.npz, per regime, as tests/test_geodesic_host.py prints them."""
from __future__ import annotations

import mpmath as mp
import numpy as np

DPS = 30  # every public function works at this precision whatever the process-wide setting is (other references change it)


def at_dps(fn):
    def wrapped(*a, **kw):
        with mp.workdps(DPS):
            return fn(*a, **kw)

    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


with mp.workdps(DPS):
    A = mp.mpf(6378137)
    F = 1 / mp.mpf("298.257223563")
    F1 = 1 - F
    B = A * F1
    E2 = F * (2 - F)
    EP2 = E2 / F1**2
    E = mp.sqrt(E2)
    C2 = (A * A + B * B * mp.atanh(E) / E) / 2  # q(90 degrees): the authalic radius squared
    AREA0 = 4 * mp.pi * C2
    DEG = mp.pi / 180
    HALF_PI = mp.pi / 2


def q_of_sinphi(sphi):
    return (B * B / 2) * (sphi / (1 - E2 * sphi * sphi) + mp.atanh(E * sphi) / E)


def _beta(lat):
    """(sin beta, cos beta) of a latitude in degrees; the poles exactly"""
    lat = mp.mpf(lat)
    if abs(lat) == 90:
        return mp.sign(lat) * mp.mpf(1), mp.mpf(0)
    t = F1 * mp.tan(lat * DEG)
    c = 1 / mp.sqrt(1 + t * t)
    return t * c, c


def _lat_of(sbet, cbet):
    return mp.atan2(sbet, F1 * cbet) / DEG


def _splits(s1, s2):
    """the interval [s1, s2] cut at the multiples of pi / 2 inside it (where the integrands peak for a geodesic that passes a pole closely)"""
    lo, hi = (s1, s2) if s1 <= s2 else (s2, s1)
    pts = [lo]
    k = mp.ceil(lo / HALF_PI)
    while k * HALF_PI < hi:
        if k * HALF_PI > lo:
            pts.append(k * HALF_PI)
        k += 1
    pts.append(hi)
    return pts if s1 <= s2 else pts[::-1]


def _quad(fn, s1, s2):
    if s1 == s2:
        return mp.mpf(0)
    return mp.quad(fn, _splits(s1, s2))


class Line:
    """the geodesic through (lat1, lon1 = 0) with azimuth alp1 (radians), as functions of the arc sigma"""

    def __init__(self, sbet1, cbet1, salp1, calp1):
        self.salp0 = salp1 * cbet1
        self.calp0 = mp.hypot(calp1, salp1 * sbet1)
        if sbet1 == 0 and calp1 < 0:
            self.sig1 = -mp.pi  # (the signed zero of the double code, said out loud)
        elif sbet1 == 0 and calp1 == 0:
            self.sig1 = mp.mpf(0)
        else:
            self.sig1 = mp.atan2(sbet1, calp1 * cbet1)
        self.k2 = EP2 * self.calp0**2

    def root(self, sig):
        return mp.sqrt(1 + self.k2 * mp.sin(sig) ** 2)

    def omega(self, sig):
        """the longitude on the auxiliary sphere, continuous in sigma: omega - sigma = atan2((s0 - 1) sin cos, cos^2 + s0 sin^2) stays in
        (-pi / 2, pi / 2) for s0 = |sin alpha0| > 0"""
        s0 = abs(self.salp0)
        ss, cs = mp.sin(sig), mp.cos(sig)
        w = sig + mp.atan2((s0 - 1) * ss * cs, cs * cs + s0 * ss * ss)
        return w if self.salp0 >= 0 else -w

    def s(self, sig2):
        return B * _quad(self.root, self.sig1, sig2)

    def lam(self, sig2):
        i3 = _quad(lambda t: (2 - F) / (1 + F1 * self.root(t)), self.sig1, sig2)
        return self.omega(sig2) - self.omega(self.sig1) - F * self.salp0 * i3

    def m12(self, sig2):
        j = _quad(lambda t: self.k2 * mp.sin(t) ** 2 / self.root(t), self.sig1, sig2)
        s1, c1, s2, c2 = mp.sin(self.sig1), mp.cos(self.sig1), mp.sin(sig2), mp.cos(sig2)
        return B * (self.root(sig2) * c1 * s2 - self.root(self.sig1) * s1 * c2 - c1 * c2 * j)

    def point(self, sig2):
        """(sin beta, cos beta, sin alpha, cos alpha) at sigma"""
        ss, cs = mp.sin(sig2), mp.cos(sig2)
        return self.calp0 * ss, mp.hypot(self.salp0, self.calp0 * cs), self.salp0, self.calp0 * cs

    def area(self, sig2):
        """int q d lambda over [sig1, sig2] — the line integral (no pole on the way: the callers see to that)"""
        if self.salp0 == 0:
            return mp.mpf(0)

        def fn(t):
            st = mp.sin(t)
            sb = self.calp0 * st
            cb2 = 1 - sb * sb
            sphi = sb / mp.sqrt(sb * sb + F1 * F1 * cb2)
            return q_of_sinphi(sphi) * (self.salp0 / cb2 - F * self.salp0 * (2 - F) / (1 + F1 * self.root(t)))

        return _quad(fn, self.sig1, sig2)

    def i4_form(self, sig2):
        """Karney's S(sig2) - S(sig1) = c^2 (alp2 - alp1) + e^2 a^2 cos alp0 sin alp0 (I4(sig2) - I4(sig1)), I4 by quadrature (2013, eqs. 58-63)"""

        def t_of(x):
            return x + mp.sqrt(1 / x + 1) * mp.asinh(mp.sqrt(x)) if x != 0 else mp.mpf(1)

        def fn(t):
            x = self.k2 * mp.sin(t) ** 2
            if EP2 == x:
                return mp.mpf(0)
            return -(t_of(EP2) - t_of(x)) / (EP2 - x) * mp.sin(t) / 2

        i4 = _quad(fn, self.sig1, sig2)
        a1 = mp.atan2(self.salp0, self.calp0 * mp.cos(self.sig1))
        a2 = mp.atan2(self.salp0, self.calp0 * mp.cos(sig2))
        return C2 * (a2 - a1) + E2 * A * A * self.calp0 * self.salp0 * i4


@at_dps
def direct(lon1, lat1, azi1, s12):
    """(lon2, lat2, azi2) in degrees (lon2 not wrapped), and sigma12"""
    sb, cb = _beta(lat1)
    alp = mp.mpf(azi1) * DEG
    L = Line(sb, cb, mp.sin(alp), mp.cos(alp))
    s12 = mp.mpf(s12)
    sig = L.sig1 + s12 / B
    for _ in range(60):
        d = (L.s(sig) - s12) / (B * L.root(sig))
        sig -= d
        if abs(d) < mp.mpf(10) ** -27:
            break
    sb2, cb2, sa2, ca2 = L.point(sig)
    return mp.mpf(lon1) + L.lam(sig) / DEG, _lat_of(sb2, cb2), mp.atan2(sa2, ca2) / DEG, sig - L.sig1


def _ang_diff(lon1, lon2):
    d = (mp.mpf(lon2) - mp.mpf(lon1)) % 360
    return d - 360 if d > 180 else d  # in (-180, 180]


def _bracketed_root(g, lo, hi):
    """the root of an increasing g on [lo, hi]: the Illinois variant of false position, bisection when it stalls"""
    glo, ghi = g(lo), g(hi)
    if glo >= 0:
        return lo
    if ghi <= 0:
        return hi
    side = 0
    for it in range(300):
        x = (lo * ghi - hi * glo) / (ghi - glo) if it % 4 != 3 else (lo + hi) / 2
        gx = g(x)
        if gx == 0 or hi - lo < mp.mpf(10) ** -27:
            return x
        if gx < 0:
            lo, glo = x, gx
            if side == -1:
                ghi /= 2
            side = -1
        else:
            hi, ghi = x, gx
            if side == 1:
                glo /= 2
            side = 1
    return (lo + hi) / 2


@at_dps
def inverse(lon1, lat1, lon2, lat2):
    """dict(s12, azi1, azi2, m12, S12) of the shortest geodesic; S12 is None where it is a matter of convention (an edge over a pole whose
    longitudes differ by exactly 180 degrees)"""
    lon12 = _ang_diff(lon1, lon2)
    lonsign = -1 if lon12 < 0 else 1
    lam12 = abs(lon12) * DEG
    p1, p2 = mp.mpf(lat1), mp.mpf(lat2)
    swapp = -1 if abs(p1) < abs(p2) else 1
    if swapp < 0:
        lonsign = -lonsign
        p1, p2 = p2, p1
    latsign = 1 if p1 < 0 else -1
    p1, p2 = p1 * latsign, p2 * latsign  # p1 <= 0, |p1| >= |p2|
    sb1, cb1 = _beta(p1)
    sb2, cb2 = _beta(p2)

    def arc_to_2(alp1):
        sa, ca = mp.sin(alp1), mp.cos(alp1)
        L = Line(sb1, cb1, sa, ca)
        cs2 = mp.sqrt(max((ca * cb1) ** 2 + (cb2 - cb1) * (cb2 + cb1), mp.mpf(0)))  # cos alpha2 cos beta2 >= 0: the first time the parallel is met
        sig2 = mp.atan2(sb2, cs2) if not (sb2 == 0 and cs2 == 0) else mp.mpf(0)
        return L, sig2

    S12 = None
    if p1 == -90:  # from the pole: a meridian; the azimuth there is measured from the meridian of lon1
        alp1 = lam12
        L, sig2 = arc_to_2(mp.mpf(0))
        alp2 = mp.mpf(0)
        S12 = -C2 * lam12 if p2 != 90 else None
    elif lam12 == 0:
        alp1 = mp.mpf(0)
        L, sig2 = arc_to_2(alp1)
        alp2 = mp.mpf(0)
        S12 = mp.mpf(0)
    elif lam12 == mp.pi:
        alp1 = mp.pi  # over the pole (south, in this arrangement)
        L, sig2 = arc_to_2(alp1)
        alp2 = mp.mpf(0)
    elif p1 == 0 and p2 == 0 and lam12 <= F1 * mp.pi:
        alp1 = alp2 = HALF_PI  # along the equator
        L, sig2 = arc_to_2(alp1)
        sig2 = lam12 / F1  # (lambda = (1 - f) sigma there)
        S12 = mp.mpf(0)
    else:
        alp1 = _bracketed_root(lambda x: (lambda Ls: Ls[0].lam(Ls[1]))(arc_to_2(x)) - lam12, mp.mpf(0), mp.pi)
        L, sig2 = arc_to_2(alp1)
        _, _, sa2, ca2 = L.point(sig2)
        alp2 = mp.atan2(sa2, ca2)
        S12 = L.area(sig2)
    s12 = L.s(sig2) if not (p1 == 0 and p2 == 0 and alp1 == HALF_PI) else A * lam12
    m12 = L.m12(sig2)
    sa1, ca1, sa2, ca2 = mp.sin(alp1), mp.cos(alp1), mp.sin(alp2), mp.cos(alp2)
    if swapp < 0:
        sa1, sa2, ca1, ca2 = sa2, sa1, ca2, ca1
    sa1, ca1, sa2, ca2 = sa1 * swapp * lonsign, ca1 * swapp * latsign, sa2 * swapp * lonsign, ca2 * swapp * latsign
    if S12 is not None:
        S12 = S12 * swapp * lonsign * latsign
    return {"s12": s12, "azi1": mp.atan2(sa1, ca1) / DEG, "azi2": mp.atan2(sa2, ca2) / DEG, "m12": m12, "S12": S12, "lon12": lon12}


@at_dps
def reduce_area(a):
    """into (-A0 / 2, A0 / 2]"""
    a = a - AREA0 * mp.floor(a / AREA0)
    return a - AREA0 if a > AREA0 / 2 else a


@at_dps
def ring_measures(xy, edges=None):
    """(signed area, perimeter) of a closed ring of (lon, lat) rows; edges: the inverse() of every edge, when the caller has them"""
    tot, per, wind = mp.mpf(0), mp.mpf(0), mp.mpf(0)
    for i in range(len(xy) - 1):
        e = edges[i] if edges is not None else inverse(xy[i][0], xy[i][1], xy[i + 1][0], xy[i + 1][1])
        assert e["S12"] is not None, "an edge over a pole with a longitude step of exactly 180 degrees has no S12 of its own"
        tot += e["S12"]
        per += e["s12"]
        wind += e["lon12"] * DEG
    return reduce_area(-tot + C2 * wind), per


def wrap180(d):
    return (np.asarray(d, dtype=np.float64) + 180.0) % 360.0 - 180.0


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
EDGE_REGIMES = ("whole", "antipodal_0.5", "antipodal_0.01", "antipodal_1e-4", "short", "meridian", "over_pole", "equator", "from_pole")
RING_REGIMES = ("small", "large", "antimeridian", "prime_meridian", "polar", "pole_vertex", "closed_form", "dense")


def load_fixture(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


# ---- tolerances: MEASURED on the CPU, not chosen -----------------------------------------------------------------------------------
GPU_FACTOR = 4  # the project's allowance for the device's sin / cos / atan2 differing from the host's by an ulp each


def karney_bound_m(s):
    """the project's existing bound for a Karney distance: 1e-9 relative + 20 nm, per edge"""
    return 1e-9 * np.abs(s) + 2e-8


def small_distance_m(lon1, lat1, lon2, lat2):
    """metres between two points a few micrometres apart at most (a result and its reference): the local metric of the ellipsoid,
    sqrt((M d phi)^2 + (N cos phi d lambda)^2)"""
    a, e2 = float(A), float(E2)
    phi = np.deg2rad(0.5 * (np.asarray(lat1) + lat2))
    w = np.sqrt(1.0 - e2 * np.sin(phi) ** 2)
    m, n = a * (1.0 - e2) / w**3, a / w
    return np.hypot(m * np.deg2rad(np.asarray(lat2) - lat1), n * np.cos(phi) * np.deg2rad(wrap180(np.asarray(lon2) - lon1)))


# Worst error of the header on the CPU against the fixture, per regime (tests/test_geodesic_host.py prints them; x86-64, glibc libm,
# 3000 edges, 600 direct cases, 300 rings).  Where nothing was measured the figure is the precision of the number format, and says so.
ULP_AZIMUTH_M = 1.6e-9  # half an ulp of 180 degrees (1.4e-14 degrees) on the longest reduced length (m12 <= a): a floor, not a measurement
# azimuths in metres: |d azi| * |m12|
AZIMUTH_ERR_M = {
    "whole": 3.3e-9,  # measured 3.159e-9
    "antipodal_0.5": 1.6e-9,  # measured 1.361e-9: the floor
    "antipodal_0.01": 1.6e-9,  # measured 1.288e-9: the floor
    "antipodal_1e-4": 1.6e-9,  # measured 3.318e-11: the floor
    "short": 1.6e-9,  # measured 1.179e-9: the floor
    "meridian": ULP_AZIMUTH_M,  # measured 0 (the azimuths are exactly 0 or 180)
    "over_pole": ULP_AZIMUTH_M,  # measured 0
    "equator": ULP_AZIMUTH_M,  # measured 8.214e-11
    "from_pole": ULP_AZIMUTH_M,  # measured 0
}
# S12 of one edge, m^2.  The bound has three terms:
#   EDGE_AREA_ERR_M2[regime]               what was measured beyond the other two
#   EDGE_AREA_REL * |S12|                  S12 reaches 1.3e14 m^2, whose ulp is 0.016 m^2
#   2 c^2 AZIMUTH_ERR_M[regime] / |m12|    only in the regimes of CONDITIONED: between nearly antipodal points S12 contains c^2 (alp2 - alp1),
#                                          and an azimuth is only known to AZIMUTH_ERR_M / m12 radians, m12 being a few kilometres there —
#                                          moving an end point by one ulp of its longitude (3e-9 m at 180 degrees) changes S12 by more
#                                          than 0.1 m^2.  That is the conditioning of the question, not an error of the series: the ring
#                                          regimes below, where the terms of neighbouring edges cancel, hold 0.003 m^2 per edge.
ULP_AREA_M2 = 0.016  # one ulp of the largest term: a floor, not a measurement
EDGE_AREA_ERR_M2 = {
    "whole": 0.043,  # measured 0.0418 (0.0547 before the relative term)
    "antipodal_0.5": ULP_AREA_M2,  # measured: nothing beyond the conditioning term (14.1 m^2 in all, m12 down to 2.3 km)
    "antipodal_0.01": ULP_AREA_M2,  # the same (3.30 m^2 in all)
    "antipodal_1e-4": ULP_AREA_M2,  # the same (0.031 m^2 in all)
    "short": 3.3e-5,  # measured 3.156e-5
    "meridian": ULP_AREA_M2,  # measured 0 (S12 is exactly 0)
    "over_pole": ULP_AREA_M2,  # not compared: the sign of +-pi c^2 is a convention there
    "equator": ULP_AREA_M2,  # measured: nothing beyond the conditioning term (0.125 m^2 in all, past (1 - f) * 180 degrees)
    "from_pole": ULP_AREA_M2,  # measured: nothing beyond the relative term (0.0156 m^2 in all)
}
CONDITIONED = ("antipodal_0.5", "antipodal_0.01", "antipodal_1e-4", "equator")
EDGE_AREA_REL = 2.0**-52
# direct: metres to the reference point, and the azimuth on arrival in degrees
DIRECT_ERR_M = 9.2e-9  # measured 8.716e-9 (8.912e-9 by the header's own inverse)
DIRECT_AZI_ERR_DEG = 1.8e-13  # measured 1.705e-13
# ring area: m^2 per edge, plus RING_AREA_REL * |area| (the final rounding, and c^2 itself is a rounded double)
RING_AREA_ERR_M2_PER_EDGE = {
    "small": 9.4e-6,  # measured 9.112e-6
    "large": 1.32e-3,  # measured 1.279e-3
    "antimeridian": 7.0e-4,  # measured 6.775e-4
    "prime_meridian": 1.08e-3,  # measured 1.048e-3
    "polar": 2.46e-3,  # measured 2.388e-3
    "pole_vertex": 1.26e-3,  # measured 1.222e-3
    "closed_form": 4.0e-3,  # measured: nothing beyond the relative term; a quarter ulp of a 1e14 m^2 term: a floor
    "dense": 4.0e-3,  # measured 0 (both 1500-vertex rings come out as the reference's doubles); the same floor
}
RING_AREA_REL = 2.0**-52
AREA_DEFECT_M2_PER_EDGE = 0.1  # GeographicLib's planimeter documentation for order 6 (recalled, not checked): above it the series is wrong
assert max(RING_AREA_ERR_M2_PER_EDGE.values()) < AREA_DEFECT_M2_PER_EDGE and max(EDGE_AREA_ERR_M2.values()) < AREA_DEFECT_M2_PER_EDGE


def edge_errors(fx, s12, azi1, azi2, S12, factor=1):
    """per regime: (worst |d s12| in units of the Karney bound, worst azimuth error in metres, worst |d S12| less the relative and the
    conditioning term)"""
    out = {}
    m12 = np.abs(fx["edge_m12"].astype(np.float64)) * (np.pi / 180.0)
    for k, name in enumerate(EDGE_REGIMES):
        i = fx["edge_regime"] == k
        ds = np.abs(s12[i] - fx["edge_s12"][i]) / karney_bound_m(fx["edge_s12"][i])
        da = np.maximum(np.abs(wrap180(azi1[i] - fx["edge_azi1"][i])), np.abs(wrap180(azi2[i] - fx["edge_azi2"][i]))) * m12[i]
        ok = ~np.isnan(fx["edge_S12"][i])
        dS = np.zeros(0)
        if S12 is not None:
            dS = np.abs(S12[i][ok] - fx["edge_S12"][i][ok]) - EDGE_AREA_REL * np.abs(fx["edge_S12"][i][ok])
            if name in CONDITIONED:
                dS = dS - factor * 2.0 * float(C2) * AZIMUTH_ERR_M[name] / np.abs(fx["edge_m12"][i][ok].astype(np.float64))
        out[name] = (ds.max(), da.max(), dS.max() if len(dS) else 0.0)
    return out


def check_edges(fx, s12, azi1, azi2, S12, factor):
    errs = edge_errors(fx, s12, azi1, azi2, S12, factor)
    print({k: tuple(f"{x:.2e}" for x in v) for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not (v[0] <= 1.0 and v[1] <= factor * AZIMUTH_ERR_M[k] and v[2] <= factor * EDGE_AREA_ERR_M2[k])}
    assert not bad, bad


def check_direct(fx, xy, azi2, factor):
    d = small_distance_m(xy[:, 0], xy[:, 1], fx["direct_out"][:, 0], fx["direct_out"][:, 1])
    print(f"direct: {d.max():.3e} m")
    assert d.max() <= factor * DIRECT_ERR_M, d.max()
    if azi2 is not None:
        da = np.abs(wrap180(azi2 - fx["direct_out"][:, 2]))
        print(f"direct azimuth: {da.max():.3e} degrees")
        assert da.max() <= factor * DIRECT_AZI_ERR_DEG, da.max()


def ring_bounds(fx, factor):
    """(area bound, perimeter bound) of every fixture ring"""
    edges = np.diff(fx["ring_off"]) - 1
    per_edge = np.array([RING_AREA_ERR_M2_PER_EDGE[RING_REGIMES[k]] for k in fx["ring_regime"]])
    return factor * (per_edge * edges + RING_AREA_REL * np.abs(fx["ring_area"])), 1e-9 * fx["ring_perimeter"] + 2e-8 * edges


def check_rings(fx, area, perimeter, factor):
    ba, bp = ring_bounds(fx, factor)
    edges = np.diff(fx["ring_off"]) - 1
    if area is not None:
        err = np.abs(area - fx["ring_area"])
        excess = (err - factor * RING_AREA_REL * np.abs(fx["ring_area"])) / edges
        print({name: f"{excess[fx['ring_regime'] == k].max():.2e}" for k, name in enumerate(RING_REGIMES)})
        assert np.all(err <= ba), np.flatnonzero(~(err <= ba))
    if perimeter is not None:
        assert np.all(np.abs(perimeter - fx["ring_perimeter"]) <= bp), np.flatnonzero(~(np.abs(perimeter - fx["ring_perimeter"]) <= bp))
