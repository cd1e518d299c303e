#!/usr/bin/env python3
"""Within-distance join (gpk_dwithin_join) timings on device-resident data (a secondary measurement: bench.py is unchanged).

    python tools/bench_dwithin.py [--steps 5] [--warmup 2] [--only c3_1|c3_10|c4|lines] > profiles/<name>_dwithin_bench.jsonl

Workloads: 10M synth.uniform_points x 100k synth.random_linestrings (the C3 data) at a distance where a point has about 1 and about 10
partners; 1M x 1M synth.clustered_polygons (the C4 columns) at about one polygon diameter; 100k x 100k random linestrings.  The
distance is found by count-only calls (the pair count grows with the distance) and reported.  The right side's index
(GPK_INDEX_BBOX_GRID) is built once beforehand; each step is one whole synchronous call (device buffers sized by a count-only call),
timed with HIP events on the stream.  One untimed call with the join statistics on gives the candidates and how many of them the
box test rejected; one with the library's profiler on gives ms per stage.  For the C3 workloads gpk_nearest_join(max_distance =
distance) on the same inputs is timed as context.
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
from geopolars_amd.spatial_index import SpatialIndex, dwithin_pairs_device, nearest_pairs_device  # noqa: E402

STAGES = ["gpk_bounds", "gpk_dwithin_grow", "gpk_bbox_cand_count", "gpk_cand_compact", "gpk_bbox_cand_fill", "gpk_dwithin_refine",
          "gpk_dwithin_refine_large", "gpk_pair_count", "gpk_pair_emit", "gpk_dwithin_gather"]


def _c3():
    return synth.uniform_points(10_000_000), synth.random_linestrings(100_000)


WORKLOADS = {
    # name: (label, make, target mean partners per left row or None, fixed distance or None)
    "c3_1": ("10M points x 100k linestrings, ~1 partner per point", _c3, 1.0, None),
    "c3_10": ("10M points x 100k linestrings, ~10 partners per point", _c3, 10.0, None),
    "c4": ("1M x 1M clustered polygons, distance ~ one polygon diameter", lambda: (synth.clustered_polygons(1_000_000), synth.clustered_polygons(1_000_000, seed=1)), None, "diameter"),
    "lines": ("100k x 100k linestrings, as few partners per row as the crossing pairs allow (target 4)", lambda: (synth.random_linestrings(100_000), synth.random_linestrings(100_000, seed=1)), 4.0, None),
}


def _upload(a, stream):
    if a.geom_type == _abi.GEOM_POINT:
        return DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, torch.from_numpy(a.xy).to("cuda:0"), stream=stream)
    return DeviceGeoArray.upload(a, stream=stream)


def find_distance(left, right, idx, counts, n, target, start, stream):
    """(a distance with about target * n pairs, whether the search got there): the count grows about with the square of the distance
    once boxes overlap; it cannot go below the pairs at distance 0"""
    d = start
    for _ in range(8):
        h = dwithin_pairs_device(left, right, idx, d, counts, None, stream=stream)
        ratio = h / (target * n)
        if 0.8 <= ratio <= 1.25:
            return d, True
        d *= float(np.clip((1.0 / max(ratio, 1e-3)) ** 0.5, 0.25, 4.0))
    return d, False


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
    return out


def run(name, steps, warmup):
    lib = _abi.lib()
    label, make, target, fixed = WORKLOADS[name]
    left_h, right_h = make()
    stream = torch.cuda.current_stream().cuda_stream
    left, right = _upload(left_h, stream), _upload(right_h, stream)
    torch.cuda.synchronize()
    idx = SpatialIndex.from_device(right, stream=stream, for_points=False)
    n = len(left_h)
    counts = torch.empty(n, dtype=torch.int32, device="cuda:0")
    ext = float(np.ptp(right_h.xy[:, 0]) + np.ptp(right_h.xy[:, 1])) / 2
    converged = None
    if fixed == "diameter":
        b = right_h.xy[right_h.ring_offsets[:-1][:2000]] - right_h.xy[right_h.ring_offsets[:-1][:2000] + 1]
        d = float(8 * np.median(np.hypot(b[:, 0], b[:, 1])))  # (rings of ~24 edges: about a diameter)
    else:
        d, converged = find_distance(left, right, idx, counts, n, target, ext / np.sqrt(len(right_h)) / 4, stream)
    h = dwithin_pairs_device(left, right, idx, d, counts, None, stream=stream)
    pairs = torch.empty((max(h, 1), 2), dtype=torch.int32, device="cuda:0")
    dist = torch.empty(max(h, 1), dtype=torch.float64, device="cuda:0")
    call = lambda: dwithin_pairs_device(left, right, idx, d, counts, pairs, dist, stream=stream)  # noqa: E731
    times = timed(call, steps, warmup)
    st = (C.c_int64 * 4)()
    lib.gpk_join_stats_enable(1)
    lib.gpk_join_stats(st, 1)
    call()
    lib.gpk_join_stats(st, 1)
    lib.gpk_join_stats_enable(0)
    cand, rejected = int(st[2]), int(st[3])
    lib.gpk_profile_reset()
    lib.gpk_profile_filter(b"")
    lib.gpk_profile_enable(1)
    call()
    lib.gpk_profile_enable(0)
    torch.cuda.synchronize()
    stage_ms = {}
    for k in STAGES:
        ms, cnt = C.c_double(0), C.c_int64(0)
        lib.gpk_profile_query(k.encode(), C.byref(ms), C.byref(cnt))
        if cnt.value:
            stage_ms[k] = round(ms.value, 4)
    lib.gpk_profile_reset()
    out = {
        "workload": name, "what": label, "n_left": n, "n_right": len(right_h), "distance": d, "distance_search_converged": converged, "pairs": int(h),
        "partners_per_left_row": round(h / n, 3), "pairs_at_distance_0": int(dwithin_pairs_device(left, right, idx, 0.0, counts, None, stream=stream)), "candidates": cand,
        "box_rejected": rejected, "exact_evaluations": cand - rejected, "ms_per_call_median": round(float(np.median(times)), 4),
        "ms_per_call_min": round(float(np.min(times)), 4), "stage_ms": stage_ms, "steps": steps, "warmup": warmup,
    }
    ev = cand - rejected
    if ev and "gpk_dwithin_refine" in stage_ms:
        out["refine_ns_per_exact_evaluation"] = round(1e6 * (stage_ms["gpk_dwithin_refine"] + stage_ms.get("gpk_dwithin_refine_large", 0.0)) / ev, 3)
    # the row-wise kernel on pairs this call evaluated: one returned partner per matched left row as the row map (rows without a
    # partner map out of range: a null row, no evaluation)
    call()
    pl, pr = pairs[:h, 0].long(), pairs[:h, 1]
    rows = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    rows[pl] = pr
    matched = int((rows >= 0).sum().item())
    out_d = torch.empty(n, dtype=torch.float64, device="cuda:0")
    rw = timed(lambda: _abi.check(lib.gpk_distance_rowwise(left.handle, right.handle, C.c_void_p(rows.data_ptr()), C.c_void_p(out_d.data_ptr()), _abi.MEM_DEVICE, C.c_void_p(stream))), steps, warmup)
    grouped = left_h.geom_type == _abi.GEOM_POINT and right_h.geom_type == _abi.GEOM_LINESTRING and n >= 8 * len(right_h)
    out["rowwise_on_returned_pairs"] = {"rows_evaluated": matched, "ms_per_call_median": round(float(np.median(rw)), 4),
                                        "ns_per_evaluated_row": round(1e6 * float(np.median(rw)) / max(matched, 1), 3),
                                        "schedule": "grouped (row map built in the call)" if grouped else "per-row kernel"}
    if left_h.geom_type == _abi.GEOM_POINT:  # context: the nearest join bounded by the same distance
        hn = nearest_pairs_device(left, right, idx, counts, None, max_distance=d, stream=stream)
        np_ = torch.empty((max(hn, 1), 2), dtype=torch.int32, device="cuda:0")
        nt = timed(lambda: nearest_pairs_device(left, right, idx, counts, np_, dist[: max(hn, 1)] if hn <= h else None, max_distance=d, stream=stream), steps, warmup)
        out["nearest_join_same_distance"] = {"pairs": int(hn), "ms_per_call_median": round(float(np.median(nt)), 4)}
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
