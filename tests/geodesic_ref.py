"""References for the haversine and Vincenty arms of geodesic_length (gpk_geodesic_length, csrc/gpk_lineal_ops.hip; oracle:
gpko_geodesic_length) — test infrastructure.

  haversine_mp          the great-circle distance on the sphere of radius 6 371 008.8 m at 50 digits (mpmath), from the doubles as
                        they are; HAVERSINE_ERR_M holds the error of the oracle's f64 evaluation against it, measured per regime
  vincenty_py           the oracle's Vincenty loop restated in Python floats, counting its iterations: it says which nearly
                        antipodal pairs are far from the 100-iteration limit, where an ulp of sin / atan2 cannot flip the outcome
  geodesic_group_size   the dispatch of geodesic_seq_kernel<4|16, .> restated"""
from __future__ import annotations

import math

import numpy as np

R_EARTH = 6371008.8
RAD = 0.017453292519943295


def geodesic_group_size(n_coords: int, n_seq: int) -> int:
    """lanes per sequence for haversine and vincenty: 4 up to a column mean of 24 coordinates per sequence, 16 above"""
    if n_seq <= 0:
        return 0
    return 4 if n_coords / n_seq <= 24.0 else 16


# ---- haversine -------------------------------------------------------------------------------------------------------------------
# Largest |oracle f64 haversine - 50-digit value| in metres over haversine_pairs(), measured on the CPU (glibc's sin / cos / asin),
# 1000 pairs per regime.  test_oracle_lineal_ops holds the oracle to these; the GPU gets 4 x (its sin, cos and asin may each differ
# from the host's by an ulp).  The half-angle form loses accuracy where a -> 1: towards the antipode an error u in a becomes
# u / sqrt(1 - a) in the angle.
HAVERSINE_ERR_M = {
    "short": 7.2e-14,  # measured 7.16e-14 (lines of ~150 m: 4.3e-16 relative)
    "medium": 7.0e-8,  # measured 6.93e-8 (1.4e-14 relative)
    "antipodal 0.5": 4.0e-6,  # measured 3.92e-6
    "antipodal 0.01": 3.6e-4,  # measured 3.53e-4
    "antipodal 0.0001": 0.11,  # measured 0.1016 (5e-9 relative: the pair nearest its antipode)
}
GPU_FACTOR = 4.0


def haversine_pairs(m: int = 1000):
    """{regime: (lon1, lat1, lon2, lat2)} — short lines (~100 m), pairs over the whole sphere, nearly antipodal pairs at three spreads"""
    rng = np.random.default_rng(52)
    out = {}
    p1, l1 = rng.uniform(-89, 89, m), rng.uniform(-180, 180, m)
    out["short"] = (l1, p1, l1 + rng.normal(0, 1e-3, m), p1 + rng.normal(0, 1e-3, m))
    out["medium"] = (rng.uniform(-180, 180, m), rng.uniform(-90, 90, m), rng.uniform(-180, 180, m), rng.uniform(-90, 90, m))
    for spread in (0.5, 0.01, 1e-4):
        p1, l1 = rng.uniform(-75, 75, m), rng.uniform(-180, 180, m)
        out[f"antipodal {spread:g}"] = (l1, p1, l1 + 180.0 + rng.normal(0, spread, m), -p1 + rng.normal(0, spread, m))
    return out


def haversine_mp(l1, p1, l2, p2):
    """great-circle distances in metres as mpmath numbers (50 digits)"""
    import mpmath as mp

    out = []
    with mp.workdps(50):
        rad = mp.pi / 180
        for a, b, c, d in zip(l1, p1, l2, p2):
            t1, t2 = mp.mpf(float(b)) * rad, mp.mpf(float(d)) * rad
            dl = (mp.mpf(float(c)) - mp.mpf(float(a))) * rad
            h = mp.sin((t2 - t1) / 2) ** 2 + mp.cos(t1) * mp.cos(t2) * mp.sin(dl / 2) ** 2
            out.append(2 * mp.mpf(R_EARTH) * mp.asin(mp.sqrt(h)))
    return out


def haversine_errors_m(values, exact) -> np.ndarray:
    import mpmath as mp

    with mp.workdps(50):
        return np.array([float(abs(mp.mpf(float(v)) - e)) for v, e in zip(values, exact)])


# ---- Vincenty ----------------------------------------------------------------------------------------------------------------------


def vincenty_py(lon1, lat1, lon2, lat2):
    """o_vincenty of oracle/gpk_oracle.c in Python floats -> (metres or NaN, iterations done, the last |lambda - lambda'|)"""
    a, b, f = 6378137.0, 6356752.314245, 1.0 / 298.257223563
    L = (lon2 - lon1) * RAD
    U1, U2 = math.atan((1.0 - f) * math.tan(lat1 * RAD)), math.atan((1.0 - f) * math.tan(lat2 * RAD))
    sU1, cU1, sU2, cU2 = math.sin(U1), math.cos(U1), math.sin(U2), math.cos(U2)
    lam = L
    it = 0
    while True:
        it += 1
        sl, cl = math.sin(lam), math.cos(lam)
        t0, t1 = cU2 * sl, cU1 * sU2 - sU1 * cU2 * cl
        sS = math.sqrt(t0 * t0 + t1 * t1)
        if sS == 0.0:
            return (0.0 if lon1 == lon2 and lat1 == lat2 else math.nan), it, 0.0
        cS = sU1 * sU2 + cU1 * cU2 * cl
        sig = math.atan2(sS, cS)
        sA = cU1 * cU2 * sl / sS
        c2A = 1.0 - sA * sA
        c2SM = 0.0 if c2A == 0.0 else cS - 2.0 * sU1 * sU2 / c2A
        Cc = f / 16.0 * c2A * (4.0 + f * (4.0 - 3.0 * c2A))
        lam_p = lam
        lam = L + (1.0 - Cc) * f * sA * (sig + Cc * sS * (c2SM + Cc * cS * (-1.0 + 2.0 * c2SM * c2SM)))
        step = abs(lam - lam_p)
        if step <= 1e-12:
            break
        if it == 100:
            return math.nan, it, step
    uSq = c2A * (a * a - b * b) / (b * b)
    A = 1.0 + uSq / 16384.0 * (4096.0 + uSq * (-768.0 + uSq * (320.0 - 175.0 * uSq)))
    B = uSq / 1024.0 * (256.0 + uSq * (-128.0 + uSq * (74.0 - 47.0 * uSq)))
    dS = B * sS * (c2SM + B / 4.0 * (cS * (-1.0 + 2.0 * c2SM * c2SM) - B / 6.0 * c2SM * (-3.0 + 4.0 * sS * sS) * (-3.0 + 4.0 * c2SM * c2SM)))
    return b * A * (sig - dS), it, step


def nearly_antipodal_pairs(m: int = 400):
    """nearly antipodal pairs whose outcome does not hang on an ulp: those that converge within 50 iterations and those whose lambda
    still moves by more than 1e-9 at the 100th -> (lon1, lat1, lon2, lat2, is_nan, number drawn)"""
    rng = np.random.default_rng(53)
    keep = []
    drawn = 0
    for spread in (3.0, 1.0, 0.3, 0.05):
        p1, l1 = rng.uniform(-75, 75, m), rng.uniform(-170, 170, m)
        l2, p2 = l1 + 180.0 + rng.normal(0, spread, m), -p1 + rng.normal(0, spread, m)
        for q in zip(l1, p1, l2, p2):
            drawn += 1
            v, it, step = vincenty_py(*(float(x) for x in q))
            if (not math.isnan(v) and it <= 50) or (math.isnan(v) and step > 1e-9):
                keep.append((*q, math.isnan(v)))
    k = np.array(keep)
    return k[:, 0], k[:, 1], k[:, 2], k[:, 3], k[:, 4].astype(bool), drawn
