#!/usr/bin/env python3
"""Any-family nearest join (gpk_nearest_join_any) timings on device-resident data (a secondary measurement: bench.py is unchanged).

    python tools/bench_nearest_any.py [--steps 5] [--warmup 2] [--only c2|c4] > profiles/nearest_any_bench.jsonl

Workloads: 10M synth.uniform_points x 1000 synth.star_polygons (the C2 data, a POINT left column) beside gpk_nearest_join on the same
buffers, whose bytes it must return; 1M x 1M synth.clustered_polygons (the C4 columns, polygons on both sides) beside gpk_dwithin_join
at about one polygon diameter and beside gpk_distance_rowwise(left, right, nearest_r) — the exact evaluation of the returned pairs
alone, the floor of any search.  The right side's index (GPK_INDEX_BBOX_GRID) is built once beforehand; each step is one whole
synchronous call (device buffers sized by a count-only call), timed with HIP events on the stream.  One untimed call with the join
statistics on gives the candidates listed and how many of them the box test rejected; one with the library's profiler on gives ms per
stage.  Before a time is printed the result is checked on a sample of 10 000 left rows: every returned distance is the double
gpk_distance_rowwise gives for the pair, and every row has at least one pair (the synthetic columns hold no null or empty row).
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
from geopolars_amd.spatial_index import SpatialIndex, dwithin_pairs_device, nearest_pairs_any_device, nearest_pairs_device  # noqa: E402

STAGES = ["gpk_bounds", "gpk_nearest_any_seed", "gpk_nearest_any_seed_refine", "gpk_nearest_any_seed_refine_large", "gpk_nearest_any_grow",
          "gpk_bbox_cand_count", "gpk_cand_compact", "gpk_bbox_cand_fill", "gpk_nearest_any_refine", "gpk_nearest_any_refine_large",
          "gpk_nearest_any_min", "gpk_nearest_any_hit", "gpk_pair_count", "gpk_pair_emit", "gpk_nearest_any_gather"]
SAMPLE = 10_000

WORKLOADS = {
    "c2": ("10M points x 1000 star polygons (POINT left: beside gpk_nearest_join)", lambda: (synth.uniform_points(10_000_000), synth.star_polygons(1000, 64))),
    "c4": ("1M x 1M clustered polygons (beside gpk_dwithin_join at one diameter and the row-wise floor)",
           lambda: (synth.clustered_polygons(1_000_000), synth.clustered_polygons(1_000_000, seed=1))),
}


def _upload(a, stream):
    if a.geom_type == _abi.GEOM_POINT:
        return DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, torch.from_numpy(a.xy).to("cuda:0"), stream=stream)
    return DeviceGeoArray.upload(a, stream=stream)


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


def _ms(times):
    return {"ms_per_call_median": round(float(np.median(times)), 4), "ms_per_call_min": round(float(np.min(times)), 4)}


def run(name, steps, warmup):
    lib = _abi.lib()
    label, make = WORKLOADS[name]
    left_h, right_h = make()
    stream = torch.cuda.current_stream().cuda_stream
    left, right = _upload(left_h, stream), _upload(right_h, stream)
    torch.cuda.synchronize()
    idx = SpatialIndex.from_device(right, stream=stream, for_points=False)
    n = len(left_h)
    counts = torch.empty(n, dtype=torch.int32, device="cuda:0")
    h = nearest_pairs_any_device(left, right, idx, counts, None, stream=stream)
    pairs = torch.empty((max(h, 1), 2), dtype=torch.int32, device="cuda:0")
    dist = torch.empty(max(h, 1), dtype=torch.float64, device="cuda:0")
    call = lambda: nearest_pairs_any_device(left, right, idx, counts, pairs, dist, stream=stream)  # noqa: E731
    assert call() == h

    # the check that comes before any time: the first returned partner of every row as the row map of gpk_distance_rowwise
    c = counts.long()
    first = torch.cumsum(c, 0) - c
    has = c > 0
    rows = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    rows[has] = pairs[first[has], 1]
    out_d = torch.empty(n, dtype=torch.float64, device="cuda:0")
    rowwise = lambda: _abi.check(lib.gpk_distance_rowwise(left.handle, right.handle, C.c_void_p(rows.data_ptr()), C.c_void_p(out_d.data_ptr()),  # noqa: E731
                                                          _abi.MEM_DEVICE, C.c_void_p(stream)))
    rowwise()
    torch.cuda.synchronize()
    sample = torch.from_numpy(np.random.default_rng(0).choice(n, min(SAMPLE, n), replace=False)).to("cuda:0")
    assert bool(has[sample].all()), "a sampled left row has no pair"
    got, want = dist[first[sample]].cpu().numpy(), out_d[sample].cpu().numpy()
    assert got.tobytes() == want.tobytes(), "a returned distance is not gpk_distance_rowwise's double for the pair"

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
    out = {"workload": name, "what": label, "n_left": n, "n_right": len(right_h), "pairs": int(h), "rows_with_ties": int((c > 1).sum().item()),
           **_ms(times), "candidates": cand, "box_rejected": rejected, "exact_evaluations": cand - rejected,
           "candidates_per_pair_returned": round(cand / max(h, 1), 3), "stage_ms": stage_ms, "sample_checked": int(len(sample)), "steps": steps, "warmup": warmup}
    out["rowwise_on_returned_pairs"] = _ms(timed(rowwise, steps, warmup))
    if left_h.geom_type == _abi.GEOM_POINT:  # gpk_nearest_join on the same buffers: the same bytes
        p2, d2, c2 = torch.empty_like(pairs), torch.empty_like(dist), torch.empty_like(counts)
        point_call = lambda: nearest_pairs_device(left, right, idx, c2, p2, d2, stream=stream)  # noqa: E731
        assert point_call() == h
        torch.cuda.synchronize()
        assert torch.equal(c2, counts) and torch.equal(p2[:h], pairs[:h]) and d2[:h].cpu().numpy().tobytes() == dist[:h].cpu().numpy().tobytes()
        out["nearest_join_same_buffers"] = _ms(timed(point_call, steps, warmup))
    else:  # gpk_dwithin_join at about one polygon diameter (the distance tools/bench_dwithin.py uses for these columns)
        b = right_h.xy[right_h.ring_offsets[:-1][:2000]] - right_h.xy[right_h.ring_offsets[:-1][:2000] + 1]
        d = float(8 * np.median(np.hypot(b[:, 0], b[:, 1])))
        hd = dwithin_pairs_device(left, right, idx, d, counts, None, stream=stream)
        pd_, dd = torch.empty((max(hd, 1), 2), dtype=torch.int32, device="cuda:0"), torch.empty(max(hd, 1), dtype=torch.float64, device="cuda:0")
        out["dwithin_join_one_diameter"] = {"distance": d, "pairs": int(hd),
                                            **_ms(timed(lambda: dwithin_pairs_device(left, right, idx, d, counts, pd_, dd, stream=stream), steps, warmup))}
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
