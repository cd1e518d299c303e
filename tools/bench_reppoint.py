#!/usr/bin/env python3
"""representative_point (gpk_representative_point) timings on device-resident data (a secondary measurement: bench.py is unchanged).

    python tools/bench_reppoint.py [--steps 5] [--warmup 2] [--only c4|stars|powerlaw|rings4096] >> profiles/reppoint_bench.jsonl

Workloads: benchmark config C4's clustered polygons (1M rows), 2M star polygons of 64 vertices, 200k power-law multipolygons, and a
column of 4096-coordinate rings (the work-group path).  For each column the tool first asserts, with gpk_predicate_rowwise (contains),
that the point of every row whose section is at least 1e-6 of its diagonal wide lies inside its polygon (thinner rows are counted
apart); then each step is one call with the points, the
validity bytes and the widths in device buffers, timed with HIP events on the stream.  There is no pass threshold: the number to set
the time against is gpk_centroid on the same column in the same process, which every line carries, with the per-kernel times.
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

STAGES = ["gpk_representative_point", "gpk_representative_point_large"]


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
    xy = torch.empty((n, 2), dtype=torch.float64, device="cuda:0")
    valid = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    width = torch.empty(n, dtype=torch.float64, device="cuda:0")
    cxy = torch.empty((n, 2), dtype=torch.float64, device="cuda:0")
    cvalid = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    inside = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    reppoint = lambda: _abi.check(lib.gpk_representative_point(dev.handle, xy.data_ptr(), valid.data_ptr(), width.data_ptr(), _abi.MEM_DEVICE, stream))  # noqa: E731
    centroid = lambda: _abi.check(lib.gpk_centroid(dev.handle, cxy.data_ptr(), cvalid.data_ptr(), _abi.MEM_DEVICE, stream))  # noqa: E731
    out = {"workload": name, "what": label, "rows": n, "mean_coords": round(host.n_coords / n, 1), "steps": steps, "warmup": warmup}
    # first: every non-degenerate row's point is inside its polygon, by the library's exact contains
    reppoint()
    pts = DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, xy, stream=stream)
    _abi.check(lib.gpk_predicate_rowwise(dev.handle, pts.handle, None, _abi.PRED_CONTAINS, inside.data_ptr(), _abi.MEM_DEVICE, stream))
    torch.cuda.synchronize()
    # the interior guarantee holds for rows whose widest section is at least 1e-6 of the row's diagonal: those are asserted, thinner
    # rows with a section are counted apart
    box = torch.empty((n, 4), dtype=torch.float64, device="cuda:0")
    _abi.check(lib.gpk_bounds(dev.handle, box.data_ptr(), _abi.MEM_DEVICE, stream))
    torch.cuda.synchronize()
    diag = torch.hypot(box[:, 2] - box[:, 0], box[:, 3] - box[:, 1])
    has = (valid == 1) & (width > 0)
    live = has & (width >= 1e-6 * diag)
    thin = has & ~live
    out["rows_with_a_section"], out["degenerate_rows"] = int(has.sum()), int(((valid == 1) & (width == 0)).sum())
    out["thin_rows"], out["thin_rows_outside"] = int(thin.sum()), int((thin & (inside == 0)).sum())
    outside = int((live & (inside == 0)).sum())
    assert outside == 0, f"{name}: {outside} representative points are not inside their polygons"
    out["ms_median"], out["ms_min"] = timed(reppoint, steps, warmup)
    print(f"{name}: gpk_representative_point {out['ms_median']} ms", file=sys.stderr, flush=True)
    out["stage_ms"] = stages(lib, reppoint)
    out["centroid_ms_median"], out["centroid_ms_min"] = timed(centroid, steps, warmup)
    out["reppoint_over_centroid"] = round(out["ms_median"] / out["centroid_ms_median"], 3)
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
