#!/usr/bin/env python3
"""Nearest-neighbour join (gpk_nearest_join) timings on device-resident data (a secondary measurement: bench.py is unchanged).

    python tools/bench_nearest.py [--steps 10] [--warmup 2] [--only c3|c2|c4] > profiles/<name>_nearest.jsonl

Workloads: 10M synth.uniform_points x 100k synth.random_linestrings (the C3 data, the row map replaced by the join);
10M points x 1000 synth.star_polygons (the C2 data); 1M points x 1M synth.clustered_polygons.  The right side's index
(GPK_INDEX_BBOX_GRID) is built once beforehand and timed on its own; each step is one whole call (both passes, the scan, the
pair writes; device buffers, sized by a count-only call first), timed with HIP events on the stream.  Per workload one JSON line:
ms per call (median and min), left rows/s, pairs, index build ms, and — derived on the host from a sample of queries, not from
the kernel — the mean number of right rows whose bbox lies within the returned distance (candidates the search must evaluate)
and the segments they hold.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geopolars_amd import _abi, synth  # noqa: E402
from geopolars_amd.geoarrow import DeviceGeoArray  # noqa: E402
from geopolars_amd.geoseries import GeoSeries  # noqa: E402
from geopolars_amd.spatial_index import SpatialIndex, nearest_pairs_device  # noqa: E402

WORKLOADS = {
    "c3": ("10M points x 100k linestrings", lambda: (synth.uniform_points(10_000_000), synth.random_linestrings(100_000))),
    "c2": ("10M points x 1000 star polygons", lambda: (synth.uniform_points(10_000_000), synth.star_polygons(1000, 64))),
    "c4": ("1M points x 1M clustered polygons", lambda: (synth.uniform_points(1_000_000), synth.clustered_polygons(1_000_000))),
}


def _row_coords(a) -> np.ndarray:
    off = a.geom_offsets.astype(np.int64)
    for inner in (a.part_offsets, a.ring_offsets):
        if inner is not None:
            off = inner.astype(np.int64)[off]
    return np.diff(off)


def sample_work(pts, right, bounds, best, n_sample=500, seed=0):
    """host estimate per query: right rows whose bbox is within the returned distance (the lower bound of what any bbox-pruned search
    evaluates), and their segments"""
    rng = np.random.default_rng(seed)
    rows = rng.choice(len(pts), min(n_sample, len(pts)), replace=False)
    segs = np.maximum(_row_coords(right) - 1, 0)
    cands, seg_tot = 0, 0
    for chunk in np.array_split(rows, max(1, len(rows) // 4)):
        q = pts.xy[chunk]
        qx, qy = q[:, :1], q[:, 1:]
        dx = np.maximum(np.maximum(bounds[None, :, 0] - qx, qx - bounds[None, :, 2]), 0.0)
        dy = np.maximum(np.maximum(bounds[None, :, 1] - qy, qy - bounds[None, :, 3]), 0.0)
        hit = np.hypot(dx, dy) <= best[chunk][:, None]
        cands += int(hit.sum())
        seg_tot += int((hit * segs[None, :]).sum())
    return cands / len(rows), seg_tot / len(rows)


def run(name, steps, warmup):
    label, make = WORKLOADS[name]
    pts_h, right_h = make()
    stream = torch.cuda.current_stream().cuda_stream
    pts = DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, torch.from_numpy(pts_h.xy).to("cuda:0"), stream=stream)
    right = DeviceGeoArray.upload(right_h, stream=stream)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    idx = SpatialIndex.from_device(right, stream=stream, for_points=False)
    e1.record()
    torch.cuda.synchronize()
    build_ms = e0.elapsed_time(e1)
    n = len(pts_h)
    counts = torch.empty(n, dtype=torch.int32, device="cuda:0")
    h = nearest_pairs_device(pts, right, idx, counts, None, stream=stream)
    pairs = torch.empty((max(h, 1), 2), dtype=torch.int32, device="cuda:0")
    dist = torch.empty(max(h, 1), dtype=torch.float64, device="cuda:0")
    for _ in range(warmup):
        nearest_pairs_device(pts, right, idx, counts, pairs, dist, stream=stream)
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        nearest_pairs_device(pts, right, idx, counts, pairs, dist, stream=stream)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    c = counts.cpu().numpy()
    d = dist[:h].cpu().numpy()
    first = np.concatenate([[0], np.cumsum(c)[:-1]])
    best = np.full(n, np.inf)
    best[c > 0] = d[first[c > 0]]
    t0 = time.perf_counter()
    bounds = GeoSeries(right_h, device=right).bounds()
    cand, segs = sample_work(pts_h, right_h, bounds, best)
    ms = float(np.median(times))
    return {
        "workload": name,
        "what": label,
        "n_left": n,
        "n_right": len(right_h),
        "pairs": int(h),
        "rows_with_ties": int(np.count_nonzero(c > 1)),
        "ms_per_call_median": round(ms, 4),
        "ms_per_call_min": round(float(np.min(times)), 4),
        "left_rows_per_s": round(n / (ms * 1e-3), 1),
        "index_build_ms": round(build_ms, 4),
        "mean_candidates_per_query_sampled": round(cand, 3),
        "mean_segments_per_query_sampled": round(segs, 2),
        "sample_s": round(time.perf_counter() - t0, 2),
        "steps": steps,
        "warmup": warmup,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=sorted(WORKLOADS), action="append")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    name, cus = _abi.device_info()
    for w in a.only or ["c3", "c2", "c4"]:
        r = run(w, a.steps, a.warmup)
        r["device"] = f"{name} ({cus} CUs)"
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
