#!/usr/bin/env python3
"""Polygon union (gpk_polygon_union) and grouped union (GeoSeries.union_all) timings on device-resident data (a secondary
measurement: bench.py is unchanged).

    python tools/bench_polyunion.py [--steps 5] [--warmup 2] [--only c4|stars] [--no-union-all] >> profiles/polyunion_bench.jsonl

The workloads and the pairs are those of tools/bench_polyclip.py: benchmark config C4's 1M x 1M synth.clustered_polygons and 100k x 10k
64-vertex synth.star_polygons, over the pairs of gpk_polygon_relation_join(intersects).  Each step is one whole call over the pair lists
into a fresh result column (freed after the step), timed with HIP events on the stream; gpk_polygon_clip(intersection) is timed on the
same pairs in the same process, and the ratio is reported.  Before a time is printed the tool asserts on EVERY pair that
area(union) = area(a) + area(b) - intersection_area, with the bound bench_polyclip.py uses for its identities: the measure's
2e-9 * d^2 plus the union's 1e-9 * d^2 * (edges(a) + edges(b)), d the diagonal of the pair's joint box; and that no row is unresolved.
For C4 it also runs union_all of the left side grouped by the 64 x 64 grid cell of the centroid (one line of its own: rounds are not
timed apart; the status histogram of the groups is reported, not asserted)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geopolars_amd import _abi  # noqa: E402
from geopolars_amd.geoarrow import DeviceGeoArray  # noqa: E402
from geopolars_amd.geoseries import GeoSeries  # noqa: E402
from geopolars_amd.spatial_index import SpatialIndex, polygon_clip_pairs_device, polygon_relation_pairs_device, polygon_union_pairs_device  # noqa: E402
from tools.bench_polyclip import WORKLOADS, _f64, timed  # noqa: E402

STAGES = ["gpk_polygon_union_count", "gpk_polygon_union_fill", "gpk_polygon_union_stitch", "gpk_polygon_union_offsets", "gpk_polygon_union_emit",
          "gpk_polygon_union_totals", "gpk_scan_partial", "gpk_scan_totals", "gpk_scan_final"]


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


def run(name, steps, warmup, piece):
    lib = _abi.lib()
    label, make = WORKLOADS[name]
    left_h, right_h = make()
    stream = torch.cuda.current_stream().cuda_stream
    left, right = DeviceGeoArray.upload(left_h, stream=stream), DeviceGeoArray.upload(right_h, stream=stream)
    torch.cuda.synchronize()
    idx = SpatialIndex.from_device(right, stream=stream, for_points=False)
    n = len(left_h)
    counts = torch.empty(n, dtype=torch.int32, device="cuda:0")
    out = {"workload": name, "what": label, "n_left": n, "n_right": len(right_h), "steps": steps, "warmup": warmup}
    h = polygon_relation_pairs_device(left, right, idx, "intersects", counts, None, stream=stream)
    pairs = torch.empty((max(h, 1), 2), dtype=torch.int32, device="cuda:0")
    masks = torch.empty(max(h, 1), dtype=torch.uint8, device="cuda:0")
    polygon_relation_pairs_device(left, right, idx, "intersects", counts, pairs, masks, stream=stream)
    torch.cuda.synchronize()
    li, ri = pairs[:h, 0].contiguous(), pairs[:h, 1].contiguous()
    out["pairs"] = int(h)

    # ---- the identity, on every returned pair
    st = torch.empty(h, dtype=torch.uint8, device="cuda:0")
    uni = polygon_union_pairs_device(left, right, li, ri, "union", out_status=st, stream=stream)
    torch.cuda.synchronize()
    out["status_union"] = torch.bincount(st.long(), minlength=5).tolist()
    assert out["status_union"][4] == 0, "unresolved rows"
    area_u = _f64(lib, lib.gpk_area, uni.device(), h)
    area_a, area_b = _f64(lib, lib.gpk_area, left, n)[li.long()], _f64(lib, lib.gpk_area, right, len(right_h))[ri.long()]
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
    err = (area_u - (area_a + area_b - measure)).abs()
    assert bool((err <= 2e-9 * d2 + 1e-9 * d2 * edges + 1e-15 * (area_a + area_b)).all()), \
        f"area(union) differs from area(a) + area(b) - intersection_area: worst {float((err / d2).max()):.3e} of d^2"
    out.update(worst_identity_over_d2=float((err / d2).max()), out_coords=int(uni.device().n_coords), out_bytes=int(uni.device().nbytes()))
    uni.device().free()

    # ---- timings: the union and the intersection on the same pairs
    def union_all_pairs(drop=False):
        r = polygon_union_pairs_device(left, right, li, ri, "union", drop_empty=drop, stream=stream)
        r.device().free()

    def clip_all_pairs():
        r = polygon_clip_pairs_device(left, right, li, ri, "intersection", stream=stream)
        r.device().free()

    out["union_ms_median"], out["union_ms_min"] = timed(union_all_pairs, steps, warmup)
    out["intersection_ms_median"], out["intersection_ms_min"] = timed(clip_all_pairs, steps, warmup)
    out["union_over_intersection"] = round(out["union_ms_median"] / out["intersection_ms_median"], 3)
    out["union_stage_ms"] = stages(lib, union_all_pairs)
    idx.free()
    return out, left_h


def run_union_all(left_h, cells=64):
    """union_all of the column grouped by the cells x cells grid cell of the centroid: one wall-clock time (upload and the final
    download included), the rounds and the status histogram of the groups"""
    s = GeoSeries(left_h)
    xy = s.centroid().array.xy
    lo, hi = np.nanmin(xy, axis=0), np.nanmax(xy, axis=0)
    cell = np.clip(((xy - lo) / (hi - lo) * cells).astype(np.int64), 0, cells - 1)
    by = np.nan_to_num(cell[:, 0] * cells + cell[:, 1]).astype(np.int64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, status = s.union_all(by=by, return_status=True)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    sizes = np.bincount(np.unique(by, return_inverse=True)[1])
    return {"workload": "c4_union_all", "what": f"union_all of C4's left side by a {cells} x {cells} grid cell of the centroid", "n_rows": len(left_h),
            "groups": int(len(out)), "largest_group": int(sizes.max()), "rounds": int(np.ceil(np.log2(max(int(sizes.max()), 1)))),
            "wall_ms": round(ms, 1), "status_groups": np.bincount(status, minlength=5).tolist(), "out_parts": int(out.array.n_parts),
            "out_coords": int(out.array.n_coords)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--piece", type=int, default=500_000, help="pairs per call of the measure in the cross-check (its left column is gathered per pair)")
    ap.add_argument("--only", choices=sorted(WORKLOADS), action="append")
    ap.add_argument("--no-union-all", action="store_true", help="leave out union_all of C4's left side")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    name, cus = _abi.device_info()
    for w in a.only or list(WORKLOADS):
        r, left_h = run(w, a.steps, a.warmup, a.piece)
        r["device"] = f"{name} ({cus} CUs)"
        print(json.dumps(r), flush=True)
        if w == "c4" and not a.no_union_all:
            u = run_union_all(left_h)
            u["device"] = r["device"]
            print(json.dumps(u), flush=True)


if __name__ == "__main__":
    main()
