#!/usr/bin/env python3
"""Polygon validity (gpk_validity) timings on device-resident data (a secondary measurement: bench.py is unchanged).

    python tools/bench_validity.py [--steps 5] [--warmup 2] [--only c4|stars|powerlaw|rings4096] >> profiles/validity_bench.jsonl

Workloads: benchmark config C4's clustered polygons (1M rows), 2M star polygons of 64 vertices, power-law multipolygons (rings of at
most 10^4 coordinates), and a column of 4096-coordinate rings (the work-group path).  Each step is one call with codes and `where` in device buffers, timed with HIP events
on the stream.  There is no pass threshold: nothing comparable exists before this call.  As context every line carries the time of
gpk_polygon_relation(a, a) on the same column, which walks the same rings, the code histogram, and the per-kernel times.
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

STAGES = ["gpk_validity", "gpk_validity_large", "gpk_polygon_relation"]


def _rings4096(n=512, coords=4096):
    """star rings of 4096 coordinates, one per row"""
    rng = np.random.default_rng(9)
    k = coords - 1
    t = 2 * np.pi * np.arange(k) / k
    xy = np.empty((n, coords, 2))
    for i in range(n):
        rad = 100.0 * (1.0 + 0.3 * np.sin(7 * t + rng.uniform(0, 6)) + 0.05 * rng.uniform(-1, 1, k))
        c = rng.uniform(0, 1e5, 2)
        xy[i, :k, 0], xy[i, :k, 1] = c[0] + rad * np.cos(t), c[1] + rad * np.sin(t)
        xy[i, k] = xy[i, 0]
    off = np.arange(0, (n + 1) * coords, coords, dtype=np.int32)
    return GeoArrowArray(_abi.GEOM_POLYGON, xy.reshape(-1, 2), geom_offsets=np.arange(n + 1, dtype=np.int32), ring_offsets=off)


WORKLOADS = {
    "c4": ("1M clustered polygons (benchmark config C4's left side)", lambda: synth.clustered_polygons(1_000_000, seed=41, mean_neighbours=4.0)),
    "stars": ("2M star polygons of 64 vertices", lambda: synth.star_polygons(2_000_000, 64)),
    # (rings capped at 10^4 coordinates: gpk_polygon_relation has no work-group path, a 10^5-coordinate row against itself takes it minutes)
    "powerlaw": ("200k power-law multipolygons, rings of at most 10^4 coordinates", lambda: synth.powerlaw_multipolygons(200_000, cap=10_000)),
    "rings4096": ("512 rings of 4096 coordinates", _rings4096),
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


def run(name, steps, warmup):
    lib = _abi.lib()
    label, make = WORKLOADS[name]
    host = make()
    stream = torch.cuda.current_stream().cuda_stream
    dev = DeviceGeoArray.upload(host, stream=stream)
    torch.cuda.synchronize()
    n = len(host)
    code = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    where = torch.empty(n, dtype=torch.int32, device="cuda:0")
    mask = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    validity = lambda: _abi.check(lib.gpk_validity(dev.handle, code.data_ptr(), where.data_ptr(), _abi.MEM_DEVICE, stream))  # noqa: E731
    relation = lambda: _abi.check(lib.gpk_polygon_relation(dev.handle, dev.handle, None, mask.data_ptr(), _abi.MEM_DEVICE, stream))  # noqa: E731
    out = {"workload": name, "what": label, "rows": n, "mean_coords": round(host.n_coords / n, 1), "steps": steps, "warmup": warmup}
    out["ms_median"], out["ms_min"] = timed(validity, steps, warmup)
    print(f"{name}: gpk_validity {out['ms_median']} ms", file=sys.stderr, flush=True)
    out["stage_ms"] = stages(lib, validity)
    out["code_histogram"] = torch.bincount(code.long(), minlength=10).tolist()
    out["self_relation_ms_median"], out["self_relation_ms_min"] = timed(relation, steps, warmup)
    out["validity_over_self_relation"] = round(out["ms_median"] / out["self_relation_ms_median"], 3)
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
