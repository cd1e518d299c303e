#!/usr/bin/env python3
"""Line x polygon predicate join (gpk_line_polygon_join) timings on device-resident data (a secondary measurement: bench.py is
unchanged).

    python tools/bench_relation.py [--steps 5] [--warmup 2] [--only c3_c2|clustered] >> profiles/relation_bench.jsonl

Workloads: 100k synth.random_linestrings (the C3 lines) x synth.star_polygons (the C2 polygons), and the same lines x 1M
synth.clustered_polygons.  The right side's index (GPK_INDEX_BBOX_GRID) is built once beforehand; each step is one whole synchronous
call into device buffers sized by a count-only call, timed with HIP events on the stream.  Per workload: the `intersects` join
with and without the per-pair masks, the other predicates' pair counts and times, and — the only other route to the same pair set —
gpk_dwithin_join at distance 0 on the same columns and index; the two pair sets are compared element by element.
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
from geopolars_amd.spatial_index import SpatialIndex, dwithin_pairs_device, relation_pairs_device  # noqa: E402

STAGES = ["gpk_bounds", "gpk_bbox_cand_count", "gpk_cand_compact", "gpk_bbox_cand_fill", "gpk_line_polygon_refine", "gpk_pair_count", "gpk_pair_emit",
          "gpk_line_polygon_gather", "gpk_dwithin_grow", "gpk_dwithin_refine", "gpk_dwithin_refine_large"]

WORKLOADS = {
    "c3_c2": ("100k linestrings x 10k star polygons of 64 vertices", lambda: (synth.random_linestrings(100_000), synth.star_polygons(10_000))),
    "clustered": ("100k linestrings x 1M clustered polygons", lambda: (synth.random_linestrings(100_000), synth.clustered_polygons(1_000_000))),
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
    left_h, right_h = make()
    stream = torch.cuda.current_stream().cuda_stream
    left, right = DeviceGeoArray.upload(left_h, stream=stream), DeviceGeoArray.upload(right_h, stream=stream)
    torch.cuda.synchronize()
    idx = SpatialIndex.from_device(right, stream=stream, for_points=False)
    n = len(left_h)
    counts = torch.empty(n, dtype=torch.int32, device="cuda:0")
    h = relation_pairs_device(left, right, idx, "intersects", counts, None, stream=stream)
    pairs = torch.empty((max(h, 1), 2), dtype=torch.int32, device="cuda:0")
    masks = torch.empty(max(h, 1), dtype=torch.uint8, device="cuda:0")
    rel = lambda: relation_pairs_device(left, right, idx, "intersects", counts, pairs, stream=stream)  # noqa: E731
    rel_masks = lambda: relation_pairs_device(left, right, idx, "intersects", counts, pairs, masks, stream=stream)  # noqa: E731
    out = {"workload": name, "what": label, "n_left": n, "n_right": len(right_h), "mean_line_coords": round(left_h.n_coords / n, 1),
           "mean_polygon_coords": round(right_h.n_coords / len(right_h), 1), "pairs": int(h), "steps": steps, "warmup": warmup}
    out["intersects_ms_median"], out["intersects_ms_min"] = timed(rel, steps, warmup)
    out["intersects_with_masks_ms_median"], _ = timed(rel_masks, steps, warmup)
    out["stage_ms"] = stages(lib, rel)
    rel_masks()
    torch.cuda.synchronize()
    out["mask_histogram"] = torch.bincount(masks[:h].long(), minlength=8).tolist()
    rel()
    torch.cuda.synchronize()
    ours = pairs[:h].clone()
    # the only other route to this pair set: the within-distance join at distance 0 (its distance machinery and all)
    hd = dwithin_pairs_device(left, right, idx, 0.0, counts, None, stream=stream)
    dpairs = torch.empty((max(hd, 1), 2), dtype=torch.int32, device="cuda:0")
    dw = lambda: dwithin_pairs_device(left, right, idx, 0.0, counts, dpairs, stream=stream)  # noqa: E731
    out["dwithin0_pairs"] = int(hd)
    out["dwithin0_ms_median"], out["dwithin0_ms_min"] = timed(dw, steps, warmup)
    out["dwithin0_stage_ms"] = stages(lib, dw)
    dw()
    torch.cuda.synchronize()
    out["pair_sets_equal"] = bool(hd == h and torch.equal(ours, dpairs[:hd]))
    out["speedup_over_dwithin0"] = round(out["dwithin0_ms_median"] / out["intersects_ms_median"], 3)
    for pred in ("within", "covered_by", "crosses", "touches"):
        hp = relation_pairs_device(left, right, idx, pred, counts, None, stream=stream)
        pp = torch.empty((max(hp, 1), 2), dtype=torch.int32, device="cuda:0")
        ms, _ = timed(lambda: relation_pairs_device(left, right, idx, pred, counts, pp, stream=stream), steps, warmup)
        out[pred] = {"pairs": int(hp), "ms_median": ms}
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
