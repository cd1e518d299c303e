#!/usr/bin/env python3
"""minimum_rotated_rectangle / minimum_bounding_circle (gpk_minimum_rotated_rectangle, gpk_minimum_bounding_circle) timings on
device-resident data (a secondary measurement: bench.py is unchanged).

    python tools/bench_minbound.py [--steps 5] [--warmup 2] [--only c4|stars|powerlaw|rings4096] >> profiles/minbound_bench.jsonl

Workloads: benchmark config C4's clustered polygons (1M rows), 2M star polygons of 64 vertices, 200k power-law multipolygons, and 512
rings of 4096 coordinates in convex position (the work-group path).  For each column the tool first asserts, on a sample of 10 000 rows,
that every input coordinate lies within the rectangle and within the circle, to tol = 1e-9 * (row box diagonal) + 4 ulp(max |coordinate|);
then each step is one call with every output in device buffers, timed with HIP events on the stream.  There is no pass threshold: both
operators run the hull stage of gpk_convex_hull first, so the number to set each time against is gpk_convex_hull on the same column in
the same process, which every line carries, with the per-kernel times — the new work is the difference.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geopolars_amd import _abi, synth  # noqa: E402
from geopolars_amd.geoarrow import DeviceGeoArray, GeoArrowArray  # noqa: E402

STAGES = ["gpk_hull_small", "gpk_hull_small_mid", "gpk_hull_sort_big", "gpk_hull_chain_big", "gpk_minimum_rotated_rectangle", "gpk_minimum_rotated_rectangle_large",
          "gpk_minimum_bounding_circle", "gpk_minimum_bounding_circle_large"]
SAMPLE = 10_000


def _rings4096(n=512, coords=4096):
    """ellipses of 4096 coordinates (the last closes the ring), one per row: in convex position up to the rounding of the coordinates"""
    rng = np.random.default_rng(9)
    k = coords - 1
    t = 2 * np.pi * np.arange(k) / k
    xy = np.empty((n, coords, 2))
    for i in range(n):
        a, b, rot = rng.uniform(50, 150), rng.uniform(20, 150), rng.uniform(0, np.pi)
        c = rng.uniform(0, 1e5, 2)
        x, y = a * np.cos(t), b * np.sin(t)
        xy[i, :k, 0], xy[i, :k, 1] = c[0] + x * np.cos(rot) - y * np.sin(rot), c[1] + x * np.sin(rot) + y * np.cos(rot)
        xy[i, k] = xy[i, 0]
    off = np.arange(0, (n + 1) * coords, coords, dtype=np.int32)
    return GeoArrowArray(_abi.GEOM_POLYGON, xy.reshape(-1, 2), geom_offsets=np.arange(n + 1, dtype=np.int32), ring_offsets=off)


WORKLOADS = {
    "c4": ("1M clustered polygons (benchmark config C4's left side)", lambda: synth.clustered_polygons(1_000_000, seed=41, mean_neighbours=4.0)),
    "stars": ("2M star polygons of 64 vertices", lambda: synth.star_polygons(2_000_000, 64)),
    "powerlaw": ("200k power-law multipolygons, rings of at most 10^4 coordinates", lambda: synth.powerlaw_multipolygons(200_000, cap=10_000)),
    "rings4096": ("512 rings of 4096 coordinates in convex position", _rings4096),
}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return round(float(np.median(out)), 4), round(float(np.min(out)), 4)


def stages(lib, call):
    lib.gpk_profile_reset()
    lib.gpk_profile_filter(b"")
    lib.gpk_profile_enable(1)
    call()
    lib.gpk_profile_enable(0)
    torch.cuda.synchronize()
    out = {}
    for k in STAGES:
        ms, cnt = C.c_double(0), C.c_int64(0)
        lib.gpk_profile_query(k.encode(), C.byref(ms), C.byref(cnt))
        if cnt.value:
            out[k] = round(ms.value, 4)
    lib.gpk_profile_reset()
    return out


def row_ranges(host: GeoArrowArray):
    """first and one-past-last coordinate of every row"""
    g = np.asarray(host.geom_offsets, dtype=np.int64)
    if host.geom_type == _abi.GEOM_MULTIPOLYGON:
        g = np.asarray(host.part_offsets, dtype=np.int64)[g]
    if host.ring_offsets is not None:
        g = np.asarray(host.ring_offsets, dtype=np.int64)[g]
    return g[:-1], g[1:]


def check_sample(name, host, ring, centre, radius, valid):
    """every input coordinate of the sampled rows within the rectangle and within the circle, to the tests' tol; returns the rows checked"""
    lo, hi = row_ranges(host)
    rows = np.random.default_rng(3).choice(len(lo), size=min(SAMPLE, len(lo)), replace=False)
    checked = 0
    for i in rows:
        c = host.xy[lo[i]:hi[i]]
        if len(c) == 0 or not valid[i]:
            assert len(c) == 0 or not np.isfinite(c).all(), f"{name}: row {i} has no answer"
            continue
        tol = 1e-9 * float(np.hypot(*np.ptp(c, axis=0))) + 4 * float(np.spacing(np.abs(c).max()))
        r = ring[i]
        for k in range(4):
            e = r[k + 1] - r[k]
            cross = e[0] * (c[:, 1] - r[k, 1]) - e[1] * (c[:, 0] - r[k, 0])
            assert (cross >= -tol * np.hypot(*e)).all(), f"{name}: a coordinate of row {i} lies outside its rectangle"
        assert (np.hypot(c[:, 0] - centre[i, 0], c[:, 1] - centre[i, 1]) <= radius[i] + tol).all(), f"{name}: a coordinate of row {i} lies outside its circle"
        checked += 1
    return checked


def run(name, steps, warmup):
    lib = _abi.lib()
    label, make = WORKLOADS[name]
    host = make()
    stream = torch.cuda.current_stream().cuda_stream
    dev = DeviceGeoArray.upload(host, stream=stream)
    torch.cuda.synchronize()
    n = len(host)
    ring = torch.empty((n, 5, 2), dtype=torch.float64, device="cuda:0")
    centre = torch.empty((n, 2), dtype=torch.float64, device="cuda:0")
    radius = torch.empty(n, dtype=torch.float64, device="cuda:0")
    valid = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    hull_xy = torch.empty((host.n_coords + n, 2), dtype=torch.float64, device="cuda:0")
    hull_off = torch.empty(n + 1, dtype=torch.int32, device="cuda:0")
    rect = lambda: _abi.check(lib.gpk_minimum_rotated_rectangle(dev.handle, ring.data_ptr(), valid.data_ptr(), _abi.MEM_DEVICE, stream))  # noqa: E731
    circle = lambda: _abi.check(lib.gpk_minimum_bounding_circle(dev.handle, centre.data_ptr(), radius.data_ptr(), valid.data_ptr(), _abi.MEM_DEVICE, stream))  # noqa: E731
    hull = lambda: _abi.check(lib.gpk_convex_hull(dev.handle, hull_xy.data_ptr(), hull_off.data_ptr(), _abi.MEM_DEVICE, stream))  # noqa: E731
    out = {"workload": name, "what": label, "rows": n, "mean_coords": round(host.n_coords / n, 1), "steps": steps, "warmup": warmup}
    rect()
    circle()
    torch.cuda.synchronize()
    out["rows_checked"] = check_sample(name, host, ring.cpu().numpy(), centre.cpu().numpy(), radius.cpu().numpy(), valid.cpu().numpy())
    out["hull_ms_median"], out["hull_ms_min"] = timed(hull, steps, warmup)
    for key, fn in (("rectangle", rect), ("circle", circle)):
        out[f"{key}_ms_median"], out[f"{key}_ms_min"] = timed(fn, steps, warmup)
        out[f"{key}_stage_ms"] = stages(lib, fn)
        out[f"{key}_over_hull"] = round(out[f"{key}_ms_median"] / out["hull_ms_median"], 3)
        print(f"{name}: {key} {out[f'{key}_ms_median']} ms, gpk_convex_hull {out['hull_ms_median']} ms", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=sorted(WORKLOADS), action="append")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    name, cus = _abi.device_info()
    for w in a.only or list(WORKLOADS):
        r = run(w, a.steps, a.warmup)
        r["device"] = f"{name} ({cus} CUs)"
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
