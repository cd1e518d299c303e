#!/usr/bin/env python3
"""Linear referencing timings on device-resident data (a secondary measurement: bench.py is unchanged).

    python tools/bench_linref.py [--steps 5] [--warmup 2] [--points 10000000] > profiles/linref_bench.jsonl

C3 data (10M synth.uniform_points x 100k synth.random_linestrings, rows = i mod L), device buffers, one process:
gpk_closest_point_rowwise, gpk_line_locate_point (plain and normalized) and, as the yardstick on the same box in the same run, the
unchanged gpk_distance_rowwise.  For this row map gpk_distance_rowwise dispatches to its grouped row-map schedule, which the new
calls do not have (a follow-up), so the three calls are ALSO timed on the first 7 L rows: below the grouped schedule's threshold
of 8 rows per target, where gpk_distance_rowwise runs the per-row kernel whose schedule the new kernels share; those ratios compare
like with like.  gpk_line_interpolate_point runs on the 100k lines and on 8M short lines (4-8 segments), with one distance for
every row and with one per row.  Locate costs at most one extra half-pass of square roots over closest point by construction (the
lengths of the segments before the winner); locate_over_closest_point says what that is in practice.
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
from geopolars_amd.geoarrow import DeviceGeoArray  # noqa: E402


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
    return {"ms_median": round(float(np.median(out)), 4), "ms_min": round(float(np.min(out)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--lines", type=int, default=100_000)
    ap.add_argument("--short-lines", type=int, default=8_000_000)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lib = _abi.lib()
    name, cus = _abi.device_info()
    dev = "cuda:0"
    stream = torch.cuda.current_stream().cuda_stream
    S = C.c_void_p(stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    pts_h, lines_h = synth.uniform_points(a.points), synth.random_linestrings(a.lines)
    n, L = a.points, a.lines
    pts = DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, torch.from_numpy(pts_h.xy).to(dev), stream=stream)
    lines = DeviceGeoArray.upload(lines_h, stream=stream)
    rows = (torch.arange(n, dtype=torch.int64, device=dev) % L).to(torch.int32)
    xy = torch.empty((n, 2), dtype=torch.float64, device=dev)
    seg = torch.empty(n, dtype=torch.int32, device=dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    res = {"device": f"{name} ({cus} CUs)", "n_points": n, "n_lines": L, "mean_vertices": round(lines_h.n_coords / L, 2), "steps": a.steps, "warmup": a.warmup}
    res["closest_point"] = timed(lambda: _abi.check(lib.gpk_closest_point_rowwise(pts.handle, lines.handle, ptr(rows), ptr(xy), ptr(seg), _abi.MEM_DEVICE, S)), a.steps, a.warmup)
    res["locate"] = timed(lambda: _abi.check(lib.gpk_line_locate_point(pts.handle, lines.handle, ptr(rows), 0, ptr(out), _abi.MEM_DEVICE, S)), a.steps, a.warmup)
    res["locate_normalized"] = timed(lambda: _abi.check(lib.gpk_line_locate_point(pts.handle, lines.handle, ptr(rows), 1, ptr(out), _abi.MEM_DEVICE, S)), a.steps, a.warmup)
    # the yardstick: the unchanged distance.  (1) as dispatched for this row map: the grouped schedule, row map built in the call
    res["distance_rowwise_as_dispatched"] = dict(timed(lambda: _abi.check(lib.gpk_distance_rowwise(pts.handle, lines.handle, ptr(rows), ptr(out), _abi.MEM_DEVICE, S)), a.steps, a.warmup),
                                                 schedule="grouped (row map built in the call)")
    # (2) its per-row kernel (distance_kernel<8, LINESTRING>), whose schedule the new kernels share: a row map below the grouped
    # schedule's threshold of 8 rows per target — the first L * 7 rows — timed for all three calls, so the ratios compare like with like
    k = min(n, 7 * L)
    sub = DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, torch.from_numpy(pts_h.xy[:k].copy()).to(dev), stream=stream)
    torch.cuda.synchronize()
    per_row = {"rows": k}
    per_row["distance_rowwise"] = timed(lambda: _abi.check(lib.gpk_distance_rowwise(sub.handle, lines.handle, ptr(rows), ptr(out), _abi.MEM_DEVICE, S)), a.steps, a.warmup)
    per_row["closest_point"] = timed(lambda: _abi.check(lib.gpk_closest_point_rowwise(sub.handle, lines.handle, ptr(rows), ptr(xy), ptr(seg), _abi.MEM_DEVICE, S)), a.steps, a.warmup)
    per_row["locate"] = timed(lambda: _abi.check(lib.gpk_line_locate_point(sub.handle, lines.handle, ptr(rows), 0, ptr(out), _abi.MEM_DEVICE, S)), a.steps, a.warmup)
    d = per_row["distance_rowwise"]["ms_median"]
    per_row["closest_point_over_distance"] = round(per_row["closest_point"]["ms_median"] / d, 3)
    per_row["locate_over_distance"] = round(per_row["locate"]["ms_median"] / d, 3)
    per_row["locate_over_closest_point"] = round(per_row["locate"]["ms_median"] / per_row["closest_point"]["ms_median"], 3)
    res["per_row_kernels_same_rows"] = per_row
    res["locate_over_closest_point"] = round(res["locate"]["ms_median"] / res["closest_point"]["ms_median"], 3)
    res["closest_point_over_distance_as_dispatched"] = round(res["closest_point"]["ms_median"] / res["distance_rowwise_as_dispatched"]["ms_median"], 3)

    # interpolate: the 100k lines, then 8M short lines; one value for every row (a kernel argument) and one value per row
    def interp(handle, m, lengths):
        oxy = torch.empty((m, 2), dtype=torch.float64, device=dev)
        valid = torch.empty(m, dtype=torch.uint8, device=dev)
        one = torch.tensor([0.37], dtype=torch.float64, device=dev)
        per = (torch.rand(m, dtype=torch.float64, device=dev) * lengths)
        r = {"rows": m}
        r["scalar_normalized"] = timed(lambda: _abi.check(lib.gpk_line_interpolate_point(handle, ptr(one), 1, 1, ptr(oxy), ptr(valid), _abi.MEM_DEVICE, S)), a.steps, a.warmup)
        r["per_row_distance"] = timed(lambda: _abi.check(lib.gpk_line_interpolate_point(handle, ptr(per), m, 0, ptr(oxy), ptr(valid), _abi.MEM_DEVICE, S)), a.steps, a.warmup)
        return r

    def lengths_of(handle, m):
        t = torch.empty(m, dtype=torch.float64, device=dev)
        _abi.check(lib.gpk_euclidean_length(handle, ptr(t), _abi.MEM_DEVICE, S))
        torch.cuda.synchronize()
        return t

    res["interpolate_100k_lines"] = interp(lines.handle, L, lengths_of(lines.handle, L))
    short_h = synth.random_linestrings(a.short_lines, seed=5, min_log2=2.0, max_log2=3.0)
    short = DeviceGeoArray.upload(short_h, stream=stream)
    torch.cuda.synchronize()
    res["interpolate_short_lines"] = dict(interp(short.handle, a.short_lines, lengths_of(short.handle, a.short_lines)), mean_vertices=round(short_h.n_coords / a.short_lines, 2))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
