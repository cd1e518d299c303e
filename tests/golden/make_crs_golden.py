"""Writes tests/golden/crs_reference.npz: geographic points and their mpmath images (tests/crs_ref.py, 40 digits, rounded to f64)
in every destination system the reprojection tests use.  Stand-alone (about a minute):

    python tests/golden/make_crs_golden.py

Rows on which the numpy restatement of the n^6 series is itself further than 1e-8 m from the reference in some instance are outside
the pinned domain and are removed; the worst remaining value per instance is stored next to the points (`np_worst_*`).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import crs_ref as R  # noqa: E402

OUT = os.path.join(HERE, "crs_reference.npz")
NP_LIMIT = 1e-8


def world_points(rng):
    hard = [(0.0, 0.0), (180.0, 0.0), (-180.0, 0.0), (0.0, 85.05), (0.0, -85.05), (180.0, 85.05), (-180.0, -85.05), (179.99999999, 45.0),
            (-179.99999999, -45.0), (1e-9, 1e-9), (-1e-9, -1e-9), (90.0, 60.0), (-90.0, -60.0), (13.4, 52.5), (-74.0, 40.7), (151.2, -33.9)]
    grid = [(lo, la) for lo in np.linspace(-180, 180, 25) for la in (-85.05, -85.0, -80.0, -60.0, -30.0, -1.0, 0.0, 1.0, 30.0, 60.0, 80.0, 85.0, 85.05)]
    n = 2000 - len(hard) - len(grid)
    rnd = np.stack([rng.uniform(-180, 180, n), rng.uniform(-85.05, 85.05, n)], axis=1)
    return np.concatenate([np.array(hard), np.array(grid), rnd])


def tm_points(rng, lon0):
    offs = (-12.0, -9.0, -6.0, -3.0, -1.0, -1e-6, 0.0, 1e-6, 1.0, 3.0, 6.0, 9.0, 12.0)
    lats = (-89.9, -89.0, -85.05, -80.0, -60.0, -45.0, -10.0, -1e-6, 0.0, 1e-6, 10.0, 45.0, 60.0, 80.0, 85.05, 89.0, 89.9)
    grid = [(lon0 + o, la) for o in offs for la in lats]
    n = 2000 - len(grid)
    near = n // 2  # half inside the zone proper (+-3 degrees), half out to +-12
    rnd = np.concatenate([
        np.stack([lon0 + rng.uniform(-3, 3, near), rng.uniform(-89.9, 89.9, near)], axis=1),
        np.stack([lon0 + rng.uniform(-12, 12, n - near), rng.uniform(-89.9, 89.9, n - near)], axis=1),
    ])
    return np.concatenate([np.array(grid), rnd])


def anti_points(rng):
    hard = [(180.0, 0.0), (-180.0, 0.0), (180.0, 60.0), (-180.0, -60.0), (177.0, 0.0), (-177.0, 0.0), (179.9999999, 10.0), (-179.9999999, -10.0),
            (174.0, 30.0), (-174.0, -30.0), (177.0, 89.9), (-177.0, -89.9)]
    n = 300 - len(hard)
    lon = rng.uniform(165.0, 195.0, n)
    lon = np.where(lon > 180.0, lon - 360.0, lon)
    return np.concatenate([np.array(hard), np.stack([lon, rng.uniform(-89.9, 89.9, n)], axis=1)])


def images(geo, epsg):
    kind, lon0, _, _ = R.describe(epsg)
    out = np.full_like(geo, np.nan)
    for i, (lon, lat) in enumerate(geo):
        if kind == R.TMERC and abs(float(R.mp_wrap180(lon - lon0))) > 12.0:
            continue
        if kind in (R.WEBMERC, R.MERC) and abs(lat) > 85.05:
            continue
        x, y = R.mp_forward(epsg, lon, lat)
        out[i] = (float(x), float(y))
    return out


def main():
    rng = np.random.default_rng(20261018)
    fx = {}
    for group, geo in (("world", world_points(rng)), ("tm", tm_points(rng, 15.0)), ("anti", anti_points(rng))):
        for epsg in R.FIXTURE_GROUPS[group]:
            fx[f"{group}_{epsg}"] = geo.copy() if epsg == 4326 else images(geo, epsg)
            print(group, epsg, "done", flush=True)
    # rows the f64 series itself cannot reach to 1e-8 m leave the fixture
    for group, codes in R.FIXTURE_GROUPS.items():
        n = len(fx[f"{group}_4326"])
        keep = np.ones(n, dtype=bool)
        for s in codes:
            for d in codes:
                a, b = fx[f"{group}_{s}"], fx[f"{group}_{d}"]
                ok = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)
                if s == d or not ok.any():
                    continue
                err = np.zeros(n)
                err[ok] = R.error_metres(d, R.np_transform(s, d, a[ok]), b[ok])
                keep &= ~(err > NP_LIMIT)
        print(group, "rows removed:", int((~keep).sum()), "of", n)
        for epsg in codes:
            fx[f"{group}_{epsg}"] = fx[f"{group}_{epsg}"][keep]
    names, worst = [], []
    for name, s, d, a, b in R.fixture_cases(fx):
        names.append(name)
        worst.append(float(R.error_metres(d, R.np_transform(s, d, a), b).max()))
        print(f"{name:24s} rows {len(a):5d}  numpy worst {worst[-1]:.3e} m")
    fx["np_worst_names"] = np.array(names)
    fx["np_worst_m"] = np.array(worst)
    np.savez_compressed(OUT, **fx)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
