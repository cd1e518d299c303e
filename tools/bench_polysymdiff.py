#!/usr/bin/env python3
"""Polygon symmetric difference (gpk_polygon_symdiff) timings on device-resident data (a secondary measurement: bench.py is
unchanged).

    python tools/bench_polysymdiff.py [--steps 5] [--warmup 2] [--only c4|stars] [--out profiles/polysymdiff_bench.jsonl]

The workloads and the pairs are those of tools/bench_polyclip.py and tools/bench_polyunion.py: benchmark config C4's 1M x 1M
synth.clustered_polygons and 100k x 10k 64-vertex synth.star_polygons, over the pairs of gpk_polygon_relation_join(intersects).  Each
step is one whole call over the pair lists into a fresh result column (freed after the step), timed with HIP events on the stream.
Before a time is printed the tool asserts on EVERY pair that area(result) = area(a) + area(b) - 2 intersection_area, with the bound
bench_polyclip.py uses for its identities — the measure's 2e-9 * d^2, twice, plus the clip's 1e-9 * d^2 * (edges(a) + edges(b)), d
the diagonal of the pair's joint box — and that no row has status 4.  Then it times gpk_polygon_symdiff and, on the same pairs in
the same process, gpk_polygon_union and the three-call route a caller had to chain before: difference(a, b), difference(b, a) and the
union of the two columns row by row (that union makes a null row where either difference is empty: the route is timed as it is).
One JSON line per workload, printed and appended to --out."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geopolars_amd import _abi  # noqa: E402
from geopolars_amd.geoarrow import DeviceGeoArray  # noqa: E402
from geopolars_amd.spatial_index import (  # noqa: E402
    SpatialIndex,
    polygon_clip_pairs_device,
    polygon_relation_pairs_device,
    polygon_symdiff_pairs_device,
    polygon_union_pairs_device,
)
from tools.bench_polyclip import WORKLOADS, _f64, timed  # noqa: E402

STAGES = ["gpk_polygon_symdiff_count", "gpk_polygon_symdiff_fill", "gpk_polygon_symdiff_stitch", "gpk_polygon_symdiff_offsets", "gpk_polygon_symdiff_emit",
          "gpk_polygon_symdiff_totals", "gpk_scan_partial", "gpk_scan_totals", "gpk_scan_final"]


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
    sym = polygon_symdiff_pairs_device(left, right, li, ri, out_status=st, stream=stream)
    torch.cuda.synchronize()
    out["status_symdiff"] = torch.bincount(st.long(), minlength=5).tolist()
    assert out["status_symdiff"][4] == 0, "unresolved rows"
    area_s = _f64(lib, lib.gpk_area, sym.device(), h)
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
    err = (area_s - (area_a + area_b - 2.0 * measure)).abs()
    assert bool((err <= 2 * 2e-9 * d2 + 1e-9 * d2 * edges + 1e-15 * (area_a + area_b)).all()), \
        f"area(result) differs from area(a) + area(b) - 2 intersection_area: worst {float((err / d2).max()):.3e} of d^2"
    out.update(worst_identity_over_d2=float((err / d2).max()), out_coords=int(sym.device().n_coords), out_bytes=int(sym.device().nbytes()))
    sym.device().free()

    # ---- timings: the call, the union, and the three-call route on the same pairs
    def symdiff_all_pairs():
        r = polygon_symdiff_pairs_device(left, right, li, ri, stream=stream)
        r.device().free()

    def union_all_pairs():
        r = polygon_union_pairs_device(left, right, li, ri, "union", stream=stream)
        r.device().free()

    def three_calls():
        d_ab = polygon_clip_pairs_device(left, right, li, ri, "difference", stream=stream)
        d_ba = polygon_clip_pairs_device(right, left, ri, li, "difference", stream=stream)
        r = polygon_union_pairs_device(d_ab.device(), d_ba.device(), None, None, "union", stream=stream)
        r.device().free()
        d_ab.device().free()
        d_ba.device().free()

    out["symdiff_ms_median"], out["symdiff_ms_min"] = timed(symdiff_all_pairs, steps, warmup)
    out["union_ms_median"], out["union_ms_min"] = timed(union_all_pairs, steps, warmup)
    out["three_call_ms_median"], out["three_call_ms_min"] = timed(three_calls, steps, warmup)
    out["symdiff_over_union"] = round(out["symdiff_ms_median"] / out["union_ms_median"], 3)
    out["three_call_over_symdiff"] = round(out["three_call_ms_median"] / out["symdiff_ms_median"], 3)
    out["symdiff_stage_ms"] = stages(lib, symdiff_all_pairs)
    idx.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--piece", type=int, default=500_000, help="pairs per call of the measure in the cross-check (its left column is gathered per pair)")
    ap.add_argument("--only", choices=sorted(WORKLOADS), action="append")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polysymdiff_bench.jsonl"), help="the file the result lines are appended to")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    name, cus = _abi.device_info()
    for w in a.only or list(WORKLOADS):
        r = run(w, a.steps, a.warmup, a.piece)
        r["device"] = f"{name} ({cus} CUs)"
        line = json.dumps(r)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
