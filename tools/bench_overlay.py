#!/usr/bin/env python3
"""Intersection measure join (gpk_intersection_measure_join) timings on device-resident data (a secondary measurement: bench.py is
unchanged).

    python tools/bench_overlay.py [--steps 5] [--warmup 2] [--only c4|lines] >> profiles/overlay_bench.jsonl

Workloads: benchmark config C4's sides (1M x 1M synth.clustered_polygons, seeds 41 and 42) for the area, and 100k C3 linestrings x
10k 64-vertex stars for the length.  The right side's index (GPK_INDEX_BBOX_GRID) is built once beforehand; each step is one whole
synchronous call into device buffers sized by a count-only call, timed with HIP events on the stream.  Before a time is printed the
tool asserts that the pairs at min_measure = 0 are a subset of gpk_polygon_relation_join(intersects) (gpk_line_polygon_join for the
lines) on the same columns, and that intersection_measure(a, a) equals gpk_area(a) within 1e-9 * 2 d^2 (d = a row's box diagonal).
The line next to it, for context only: gpk_polygon_relation_join(intersects) with masks on the same columns and index.
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
from geopolars_amd.spatial_index import (  # noqa: E402
    SpatialIndex,
    intersection_measure_pairs_device,
    polygon_relation_pairs_device,
    relation_pairs_device,
)

STAGES = ["gpk_bounds", "gpk_bbox_cand_count", "gpk_cand_compact", "gpk_bbox_cand_fill", "gpk_intersection_measure_refine", "gpk_pair_count", "gpk_pair_emit",
          "gpk_intersection_measure_gather", "gpk_polygon_relation_refine", "gpk_line_polygon_refine"]


def _c4():
    return synth.clustered_polygons(1_000_000, seed=41, mean_neighbours=4.0), synth.clustered_polygons(1_000_000, seed=42, mean_neighbours=4.0)


def _lines():
    return synth.random_linestrings(100_000), synth.star_polygons(10_000)  # (the columns of tools/bench_relation.py's c3_c2)


WORKLOADS = {"c4": ("1M x 1M clustered polygons (benchmark config C4): shared area", _c4),
             "lines": ("100k linestrings x 10k 64-vertex stars: length inside", _lines)}


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


def _f64(lib, fn, arr, n, width=1):
    out = torch.empty((n, width) if width > 1 else n, dtype=torch.float64, device="cuda:0")
    _abi.check(fn(arr.handle, out.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    return out


def run(name, steps, warmup):
    lib = _abi.lib()
    label, make = WORKLOADS[name]
    left_h, right_h = make()
    stream = torch.cuda.current_stream().cuda_stream
    left, right = DeviceGeoArray.upload(left_h, stream=stream), DeviceGeoArray.upload(right_h, stream=stream)
    torch.cuda.synchronize()
    idx = SpatialIndex.from_device(right, stream=stream, for_points=False)
    n = len(left_h)
    counts = torch.empty(n, dtype=torch.int32, device="cuda:0")
    out = {"workload": name, "what": label, "n_left": n, "n_right": len(right_h), "mean_left_coords": round(left_h.n_coords / n, 1),
           "mean_right_coords": round(right_h.n_coords / len(right_h), 1), "steps": steps, "warmup": warmup}
    relation = polygon_relation_pairs_device if name == "c4" else relation_pairs_device

    # check 1: the pairs at min_measure = 0 are a subset of the exact intersects join
    h = intersection_measure_pairs_device(left, right, idx, 0.0, counts, None, stream=stream)
    pairs = torch.empty((max(h, 1), 2), dtype=torch.int32, device="cuda:0")
    measures = torch.empty(max(h, 1), dtype=torch.float64, device="cuda:0")
    ours = lambda: intersection_measure_pairs_device(left, right, idx, 0.0, counts, pairs, measures, stream=stream)  # noqa: E731
    ours()
    hi = relation(left, right, idx, "intersects", counts, None, stream=stream)
    ipairs = torch.empty((max(hi, 1), 2), dtype=torch.int32, device="cuda:0")
    imasks = torch.empty(max(hi, 1), dtype=torch.uint8, device="cuda:0")
    theirs = lambda: relation(left, right, idx, "intersects", counts, ipairs, imasks, stream=stream)  # noqa: E731
    theirs()
    torch.cuda.synchronize()
    key = lambda p, k: p[:k, 0].long() * (len(right_h) + 1) + p[:k, 1].long()  # noqa: E731
    assert bool(torch.isin(key(pairs, h), key(ipairs, hi)).all()), "a pair with a positive measure does not intersect"
    m = measures[:h]
    assert bool((m > 0).all()) and bool(torch.isfinite(m).all())
    out.update(pairs=int(h), intersects_pairs=int(hi), measure_sum=float(m.sum()), measure_min=float(m.min()), measure_max=float(m.max()))

    # check 2: a polygon column against itself gives its areas
    if name == "c4":
        self_area = torch.empty(n, dtype=torch.float64, device="cuda:0")
        _abi.check(lib.gpk_intersection_measure(left.handle, left.handle, None, self_area.data_ptr(), _abi.MEM_DEVICE, None))
        area = _f64(lib, lib.gpk_area, left, n)
        box = _f64(lib, lib.gpk_bounds, left, n, 4)
        d2 = (box[:, 2] - box[:, 0]) ** 2 + (box[:, 3] - box[:, 1]) ** 2
        err = (self_area - area).abs()
        assert bool((err <= 1e-9 * 2 * d2).all()), f"intersection_measure(a, a) differs from gpk_area(a): worst {float((err / d2).max()):.3e} of d^2"
        out["self_area_worst_err_over_d2"] = float((err / d2).max())
        rowwise = lambda: lib.gpk_intersection_measure(left.handle, left.handle, None, self_area.data_ptr(), _abi.MEM_DEVICE, None)  # noqa: E731
        out["rowwise_self_ms_median"], out["rowwise_self_ms_min"] = timed(rowwise, steps, warmup)

    count_only = lambda: intersection_measure_pairs_device(left, right, idx, 0.0, counts, None, stream=stream)  # noqa: E731
    out["ms_median"], out["ms_min"] = timed(ours, steps, warmup)
    out["count_only_ms_median"], _ = timed(count_only, steps, warmup)
    out["stage_ms"] = stages(lib, ours)
    out["refine_share"] = round(out["stage_ms"].get("gpk_intersection_measure_refine", 0.0) / out["ms_median"], 3)
    out["relation_join_with_masks_ms_median"], out["relation_join_with_masks_ms_min"] = timed(theirs, steps, warmup)
    out["relation_join_stage_ms"] = stages(lib, theirs)
    out["over_relation_join_with_masks"] = round(out["ms_median"] / out["relation_join_with_masks_ms_median"], 3)
    idx.free()
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
