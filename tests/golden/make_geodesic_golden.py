"""Writes tests/golden/geodesic_measures_mp.npz from the mpmath reference tests/geodesic_measure_ref.py (minutes on eight cores):

    python tests/golden/make_geodesic_golden.py [--jobs N]

  edge_xy[n, 4] (lon1, lat1, lon2, lat2), edge_regime[n] (index into EDGE_REGIMES), edge_s12, edge_azi1, edge_azi2, edge_S12 (NaN where
  it is a matter of convention), edge_m12 (f32: only ever a weight)
  direct_in[n, 4] (lon1, lat1, azi1, s12), direct_out[n, 3] (lon2 in [-180, 180], lat2, azi2)
  ring_xy[N, 2], ring_off[n + 1], ring_regime[n], ring_area[n] (signed, counter-clockwise positive), ring_perimeter[n]

Every input coordinate is a multiple of 2^-24 degrees (6e-8 degrees: it keeps the file small), so it is exact in f64 and in mpmath.
cases() is deterministic; tests/test_geodesic_ref.py recomputes a sample and compares the bits."""
from __future__ import annotations

import argparse
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import geodesic_measure_ref as R  # noqa: E402

OUT = os.path.join(HERE, "geodesic_measures_mp.npz")
Q = 2.0**24


def quant(x):
    return np.round(np.asarray(x, dtype=np.float64) * Q) / Q


def edge_cases():
    rng = np.random.default_rng(20240611)
    sets = []
    n = 1000
    sets.append((rng.uniform(-180, 180, n), rng.uniform(-90, 90, n), rng.uniform(-180, 180, n), rng.uniform(-90, 90, n)))
    for spread in (0.5, 0.01, 1e-4):
        m = 300
        p1, l1 = rng.uniform(-75, 75, m), rng.uniform(-180, 180, m)
        p1, l1 = quant(p1), quant(l1)
        sets.append((l1, p1, l1 + 180.0 + rng.normal(0, spread, m), -p1 + rng.normal(0, spread, m)))
    m = 300
    p1, l1 = quant(rng.uniform(-89, 89, m)), quant(rng.uniform(-180, 180, m))
    sets.append((l1, p1, l1 + rng.normal(0, 1e-3, m), p1 + rng.normal(0, 1e-3, m)))  # short
    m = 200
    p1, l1 = quant(rng.uniform(-89, 89, m)), quant(rng.uniform(-180, 180, m))
    sets.append((l1, p1, l1, rng.uniform(-90, 90, m)))  # meridians
    sets.append((l1, p1, l1 + 180.0, rng.uniform(-90, 90, m)))  # over a pole
    sets.append((l1, np.zeros(m), rng.uniform(-180, 180, m), np.zeros(m)))  # the equator, up to and past (1 - f) * 180 degrees
    sets.append((l1, np.where(np.arange(m) % 2 == 0, 90.0, -90.0), rng.uniform(-180, 180, m), rng.uniform(-89, 89, m)))  # from a pole
    xy, regime = [], []
    for k, (l1, p1, l2, p2) in enumerate(sets):
        a = np.stack([quant(l1), np.clip(quant(p1), -90, 90), quant(l2), np.clip(quant(p2), -90, 90)], axis=1)
        xy.append(a)
        regime.append(np.full(len(a), k, dtype=np.uint8))
    xy, regime = np.concatenate(xy), np.concatenate(regime)
    xy[:, [0, 2]] = R.wrap180(xy[:, [0, 2]])  # (exact: multiples of 2^-24 stay multiples)
    return xy, regime


def direct_cases():
    rng = np.random.default_rng(77)
    n = 600
    lon, lat = quant(rng.uniform(-180, 180, n)), quant(rng.uniform(-89.5, 89.5, n))
    azi = quant(rng.uniform(-180, 180, n))
    s = np.round(np.where(np.arange(n) % 3 == 0, rng.uniform(0, 2.0e7, n), np.where(np.arange(n) % 3 == 1, rng.uniform(0, 1.0e5, n), rng.uniform(-3.0e6, 3.9e7, n))) * 1024) / 1024
    azi[:8] = [0.0, 90.0, 180.0, -90.0, 45.0, -135.0, 0.0, 90.0]
    lat[6:8] = 0.0
    return np.stack([lon, lat, azi, s], axis=1)


def _closed(lon, lat, reverse):
    xy = np.stack([R.wrap180(quant(lon)), np.clip(quant(lat), -90, 90)], axis=1)
    xy = np.concatenate([xy, xy[:1]])
    return xy[::-1].copy() if reverse else xy


def ring_cases():
    rng = np.random.default_rng(5150)
    rings, regime = [], []

    def blob(clon, clat, rad_deg, nv, jitter, reverse):
        th = np.sort(rng.uniform(0, 2 * np.pi, nv))
        r = rad_deg * (1 + jitter * rng.uniform(-1, 1, nv))
        lat = clat + r * np.sin(th)
        lon = clon + r * np.cos(th) / max(np.cos(np.deg2rad(clat)), 0.02)
        return _closed(lon, np.clip(lat, -89.9, 89.9), reverse)

    for i in range(120):  # 10 m to 1 km
        rad_m = 10.0 * 100.0 ** rng.uniform()
        rings.append(blob(rng.uniform(-180, 180), rng.uniform(-89, 89), rad_m / 111e3, int(rng.integers(3, 12)), 0.3, i % 2 == 1))
        regime.append(0)
    for i in range(80):  # countries and continents
        rings.append(blob(rng.uniform(-170, 170), rng.uniform(-55, 55), 1.0 * 30.0 ** rng.uniform(), int(rng.integers(4, 16)), 0.25, i % 2 == 1))
        regime.append(1)
    for i in range(25):
        rings.append(blob(180.0 + rng.uniform(-2, 2), rng.uniform(-60, 60), 0.5 * 30.0 ** rng.uniform(), int(rng.integers(4, 12)), 0.25, i % 2 == 1))
        regime.append(2)
    for i in range(25):
        rings.append(blob(rng.uniform(-2, 2), rng.uniform(-60, 60), 0.5 * 30.0 ** rng.uniform(), int(rng.integers(4, 12)), 0.25, i % 2 == 1))
        regime.append(3)
    for i in range(24):  # around a pole: every longitude once
        nv = int(rng.integers(5, 24))
        lon = np.sort(rng.uniform(-180, 180, nv))
        lat = (1 if i % 4 < 2 else -1) * rng.uniform(55, 89) * (1 + 0.05 * rng.uniform(-1, 1, nv))
        rings.append(_closed(lon, np.clip(lat, -89.9, 89.9), i % 2 == 1))
        regime.append(4)
    for i, (lons, lats) in enumerate([([0, 40, 20], [60, 60, 90]), ([10, 70, 33], [-50, -65, -90]), ([100, 160, 130, 130], [20, 20, 90, 50]), ([-30, 30, 0], [0, 0, 90])]):
        for rev in (False, True):
            rings.append(_closed(np.array(lons, float), np.array(lats, float), rev))
            regime.append(5)
    closed = [([0, 90, 0], [0, 0, 90])]  # the octant
    closed += [([0, d, 0], [0, 0, 90]) for d in (10.0, 90.0, 170.0, 179.0)]  # (0, 0), (d, 0), the pole: c^2 d, a d + 2 quarter meridians
    closed += [([l1, l1, l2, l2], [90, 0, -90, 0]) for l1, l2 in ((0.0, 30.0), (-20.0, 100.0), (170.0, -175.0))]  # lunes: 2 c^2 d
    for lons, lats in closed:
        for rev in (False, True):
            rings.append(_closed(np.array(lons, float), np.array(lats, float), rev))
            regime.append(6)
    t = np.linspace(0, 2 * np.pi, 1500, endpoint=False)
    rings.append(_closed(10 + 30 * np.cos(t) * (1 + 0.1 * np.sin(7 * t)), 45 + 20 * np.sin(t) * (1 + 0.1 * np.cos(5 * t)), False))
    rings.append(_closed(175 + 25 * np.cos(t) * (1 + 0.2 * np.sin(9 * t)), -20 + 35 * np.sin(t), True))
    regime += [7, 7]
    off = np.zeros(len(rings) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rings])
    return np.concatenate(rings), off, np.array(regime, dtype=np.uint8)


def edge_record(row):
    e = R.inverse(*[float(v) for v in row])
    S = float(e["S12"]) if e["S12"] is not None else float("nan")
    return float(e["s12"]), float(e["azi1"]), float(e["azi2"]), float(e["m12"]), S


def direct_record(row):
    lon2, lat2, azi2, _ = R.direct(*[float(v) for v in row])
    lon2 = lon2 % 360
    return float(lon2 - 360 if lon2 > 180 else lon2), float(lat2), float(azi2)


def ring_record(xy):
    area, per = R.ring_measures([(float(x), float(y)) for x, y in xy])
    return float(area), float(per)


def _ring_edge(row):
    """an edge of a ring, for the pool: the mp values survive as strings"""
    e = R.inverse(*[float(v) for v in row])
    with R.mp.workdps(R.DPS):
        return {k: (None if v is None else R.mp.nstr(v, 32)) for k, v in e.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    exy, ereg = edge_cases()
    din = direct_cases()
    rxy, roff, rreg = ring_cases()
    redges = np.concatenate([np.concatenate([rxy[roff[i]:roff[i + 1] - 1], rxy[roff[i] + 1:roff[i + 1]]], axis=1) for i in range(len(roff) - 1)])
    with multiprocessing.Pool(a.jobs) as pool:
        erec = np.array(pool.map(edge_record, exy, chunksize=16))
        print("edges done", flush=True)
        drec = np.array(pool.map(direct_record, din, chunksize=16))
        print("direct done", flush=True)
        rres = pool.map(_ring_edge, redges, chunksize=16)
        print("ring edges done", flush=True)
    rarea, rper = [], []
    k = 0
    for i in range(len(roff) - 1):
        ne = int(roff[i + 1] - roff[i] - 1)
        with R.mp.workdps(R.DPS):
            edges = [{kk: (None if v is None else R.mp.mpf(v)) for kk, v in e.items()} for e in rres[k:k + ne]]
        k += ne
        ar, pe = R.ring_measures(rxy[roff[i]:roff[i + 1]], edges)
        rarea.append(float(ar))
        rper.append(float(pe))
    np.savez_compressed(OUT, edge_xy=exy, edge_regime=ereg, edge_s12=erec[:, 0], edge_azi1=erec[:, 1], edge_azi2=erec[:, 2],
                        edge_m12=erec[:, 3].astype(np.float32), edge_S12=erec[:, 4], direct_in=din, direct_out=drec, ring_xy=rxy, ring_off=roff,
                        ring_regime=rreg, ring_area=np.array(rarea), ring_perimeter=np.array(rper))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
