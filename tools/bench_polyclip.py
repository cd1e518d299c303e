#!/usr/bin/env python3
"""Polygon clip (gpk_polygon_clip) timings on device-resident data (a secondary measurement: bench.py is unchanged).

    python tools/bench_polyclip.py [--steps 5] [--warmup 2] [--only c4|stars] >> profiles/polyclip_bench.jsonl

Workloads: benchmark config C4's 1M x 1M synth.clustered_polygons, and 100k x 10k 64-vertex synth.star_polygons.  The pairs are those
of gpk_polygon_relation_join(intersects) with masks on the right side's prebuilt GPK_INDEX_BBOX_GRID index; each step of the clip is one
whole call over the pair lists into a fresh result column (freed after the step), timed with HIP events on the stream.  Before a time
is printed the tool asserts, on EVERY returned pair (in slices: the left column is gathered per pair), that area(intersection) is
gpk_intersection_measure of the pair and that area(intersection) + area(difference) is area(a): the measure's 1e-9 * (d_a^2 + d_b^2)
<= 2e-9 * d^2 plus, per clip, 1e-9 * d * (perimeter(a) + perimeter(b)) <= 1e-9 * d^2 * (edges(a) + edges(b)), d the diagonal of the
pair's joint box; and that no row is unresolved.  Beside the clip: gpk_intersection_measure and gpk_polygon_relation on the same
first --sample pairs (the same edges x edges work without output geometry — the numbers to set the clip against) and the join itself.
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
from geopolars_amd.spatial_index import SpatialIndex, polygon_clip_pairs_device, polygon_relation_pairs_device  # noqa: E402

STAGES = ["gpk_polygon_clip_count", "gpk_polygon_clip_fill", "gpk_polygon_clip_stitch", "gpk_polygon_clip_offsets", "gpk_polygon_clip_emit",
          "gpk_polygon_clip_totals", "gpk_scan_partial", "gpk_scan_totals", "gpk_scan_final", "gpk_intersection_measure", "gpk_polygon_relation"]

WORKLOADS = {
    "c4": ("1M x 1M clustered polygons (benchmark config C4)",
           lambda: (synth.clustered_polygons(1_000_000, seed=41, mean_neighbours=4.0), synth.clustered_polygons(1_000_000, seed=42, mean_neighbours=4.0))),
    "stars": ("100k x 10k star polygons of 64 vertices", lambda: (synth.star_polygons(100_000, 64, seed=7), synth.star_polygons(10_000))),
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


def _f64(lib, fn, arr, n, width=1):
    out = torch.empty((n, width) if width > 1 else n, dtype=torch.float64, device="cuda:0")
    if n:
        _abi.check(fn(arr.handle, out.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    return out


def run(name, steps, warmup, sample, piece):
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

    h = polygon_relation_pairs_device(left, right, idx, "intersects", counts, None, stream=stream)
    pairs = torch.empty((max(h, 1), 2), dtype=torch.int32, device="cuda:0")
    masks = torch.empty(max(h, 1), dtype=torch.uint8, device="cuda:0")
    join = lambda: polygon_relation_pairs_device(left, right, idx, "intersects", counts, pairs, masks, stream=stream)  # noqa: E731
    join()
    torch.cuda.synchronize()
    li, ri = pairs[:h, 0].contiguous(), pairs[:h, 1].contiguous()
    out["pairs"] = int(h)

    # ---- the cross-checks, on every returned pair
    st_i, st_d = torch.empty(h, dtype=torch.uint8, device="cuda:0"), torch.empty(h, dtype=torch.uint8, device="cuda:0")
    inter = polygon_clip_pairs_device(left, right, li, ri, "intersection", out_status=st_i, stream=stream)
    diff = polygon_clip_pairs_device(left, right, li, ri, "difference", out_status=st_d, stream=stream)
    torch.cuda.synchronize()
    out["status_intersection"], out["status_difference"] = torch.bincount(st_i.long(), minlength=5).tolist(), torch.bincount(st_d.long(), minlength=5).tolist()
    assert out["status_intersection"][4] == 0 and out["status_difference"][4] == 0, "unresolved rows"
    area_i, area_d = _f64(lib, lib.gpk_area, inter.device(), h), _f64(lib, lib.gpk_area, diff.device(), h)
    area_a = _f64(lib, lib.gpk_area, left, n)[li.long()]
    box_a, box_b = _f64(lib, lib.gpk_bounds, left, n, 4)[li.long()], _f64(lib, lib.gpk_bounds, right, len(right_h), 4)[ri.long()]
    d2 = (torch.maximum(box_a[:, 2], box_b[:, 2]) - torch.minimum(box_a[:, 0], box_b[:, 0])) ** 2 + \
         (torch.maximum(box_a[:, 3], box_b[:, 3]) - torch.minimum(box_a[:, 1], box_b[:, 1])) ** 2
    measure = torch.empty(h, dtype=torch.float64, device="cuda:0")
    li_h = li.cpu().numpy().astype(np.int64)
    for k0 in range(0, h, piece):
        k1 = min(h, k0 + piece)
        sub = DeviceGeoArray.upload(left_h.take(li_h[k0:k1]), stream=stream)
        _abi.check(lib.gpk_intersection_measure(sub.handle, right.handle, ri[k0:k1].contiguous().data_ptr(), measure[k0:k1].data_ptr(), _abi.MEM_DEVICE, None))
        torch.cuda.synchronize()
        sub.free()

    def coords_per_row(col):  # POLYGON columns
        return torch.from_numpy(np.diff(col.ring_offsets[col.geom_offsets]).astype(np.float64)).cuda()

    edges = coords_per_row(left_h)[li.long()] + coords_per_row(right_h)[ri.long()]
    bound_clip = 1e-9 * d2 * edges
    err_i, err_sum = (area_i - measure).abs(), (area_i + area_d - area_a).abs()
    assert bool((err_i <= 2e-9 * d2 + bound_clip).all()), f"area(intersection) differs from intersection_area: worst {float((err_i / d2).max()):.3e} of d^2"
    assert bool((err_sum <= 2 * bound_clip + 1e-15 * area_a).all()), f"intersection + difference differs from area(a): worst {float((err_sum / d2).max()):.3e} of d^2"
    err_i, err_sum = (err_i / d2).max(), (err_sum / d2).max()
    out.update(worst_area_vs_measure_over_d2=float(err_i), worst_sum_vs_area_over_d2=float(err_sum), out_coords=int(inter.device().n_coords),
               out_bytes=int(inter.device().nbytes()))
    inter.device().free()
    diff.device().free()

    # ---- timings
    def clip_all(rows_l=li, rows_r=ri, how="intersection", drop=False):
        r = polygon_clip_pairs_device(left, right, rows_l, rows_r, how, drop_empty=drop, stream=stream)
        r.device().free()

    out["clip_ms_median"], out["clip_ms_min"] = timed(clip_all, steps, warmup)
    out["clip_difference_ms_median"], _ = timed(lambda: clip_all(how="difference"), steps, warmup)
    out["clip_drop_empty_ms_median"], _ = timed(lambda: clip_all(drop=True), steps, warmup)
    out["clip_stage_ms"] = stages(lib, clip_all)
    k = min(h, sample)
    sub = DeviceGeoArray.upload(left_h.take(li_h[:k]), stream=stream)
    sub_l, sub_r = li[:k].contiguous(), ri[:k].contiguous()
    mbuf, rbuf = torch.empty(k, dtype=torch.float64, device="cuda:0"), torch.empty(k, dtype=torch.uint8, device="cuda:0")
    measure_call = lambda: _abi.check(lib.gpk_intersection_measure(sub.handle, right.handle, sub_r.data_ptr(), mbuf.data_ptr(), _abi.MEM_DEVICE, None))  # noqa: E731
    relation_call = lambda: _abi.check(lib.gpk_polygon_relation(sub.handle, right.handle, sub_r.data_ptr(), rbuf.data_ptr(), _abi.MEM_DEVICE, None))  # noqa: E731
    out["sample_pairs"] = int(k)
    out["sample_measure_ms_median"], out["sample_measure_ms_min"] = timed(measure_call, steps, warmup)
    out["sample_relation_ms_median"], out["sample_relation_ms_min"] = timed(relation_call, steps, warmup)
    out["sample_clip_ms_median"], out["sample_clip_ms_min"] = timed(lambda: clip_all(sub_l, sub_r), steps, warmup)
    out["sample_clip_over_measure"] = round(out["sample_clip_ms_median"] / out["sample_measure_ms_median"], 3)
    out["sample_clip_over_relation"] = round(out["sample_clip_ms_median"] / out["sample_relation_ms_median"], 3)
    out["join_intersects_with_masks_ms_median"], out["join_intersects_with_masks_ms_min"] = timed(join, steps, warmup)
    sub.free()
    idx.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=200_000, help="pairs the measure, the relation and the clip are timed on side by side")
    ap.add_argument("--piece", type=int, default=500_000, help="pairs per call of the measure in the cross-check (its left column is gathered per pair)")
    ap.add_argument("--only", choices=sorted(WORKLOADS), action="append")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    name, cus = _abi.device_info()
    for w in a.only or list(WORKLOADS):
        r = run(w, a.steps, a.warmup, a.sample, a.piece)
        r["device"] = f"{name} ({cus} CUs)"
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
