#!/usr/bin/env python3
"""Line clip (gpk_line_clip) timings on device-resident data (a secondary measurement: bench.py is unchanged).

    python tools/bench_lineclip.py [--steps 5] [--warmup 2] [--only c3_c2|clustered] >> profiles/lineclip_bench.jsonl

Workloads (those of tools/bench_relation.py): 100k synth.random_linestrings x 10k 64-vertex synth.star_polygons, and the same lines x
1M synth.clustered_polygons.  The pairs are those of gpk_line_polygon_join(intersects) with masks on the right side's prebuilt
GPK_INDEX_BBOX_GRID index; each step of the clip is one whole call over the pair lists into a fresh result column (freed after the
step), timed with HIP events on the stream.  Before a time is printed the tool asserts, on the returned pairs: length(intersection)
is gpk_intersection_measure of the pair and length(intersection) + length(difference) is length(L), each within 2e-9 * length(L); a
non-empty intersection has an intersecting mask; the difference is empty exactly where the mask says covered_by.  Beside the clip:
gpk_intersection_measure on the same pairs (the same segments x edges work without output geometry — the number to set the clip
against; its line column is gathered per pair on the device, so both are timed on the first --sample pairs) and
gpk_line_polygon_join(intersects) on the same columns and index.
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
from geopolars_amd.spatial_index import SpatialIndex, line_clip_pairs_device, relation_pairs_device  # noqa: E402

STAGES = ["gpk_line_clip_count", "gpk_scan_partial", "gpk_scan_totals", "gpk_scan_final", "gpk_line_clip_totals", "gpk_line_clip_offsets",
          "gpk_line_clip_fill", "gpk_intersection_measure", "gpk_line_polygon_refine"]

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


def lengths(lib, arr: DeviceGeoArray) -> torch.Tensor:
    out = torch.empty(arr.n_geoms, dtype=torch.float64, device="cuda:0")
    if arr.n_geoms:
        _abi.check(lib.gpk_euclidean_length(arr.handle, out.data_ptr(), _abi.MEM_DEVICE, None))
    torch.cuda.synchronize()
    return out


def gathered_lines(xy: torch.Tensor, off: torch.Tensor, rows: torch.Tensor) -> DeviceGeoArray:
    """the LINESTRING column whose row k is row rows[k] of (xy, off), built on the device"""
    start, size = off[rows.long()].long(), (off[1:] - off[:-1])[rows.long()].long()
    new_off = torch.zeros(len(rows) + 1, dtype=torch.int64, device=xy.device)
    new_off[1:] = torch.cumsum(size, 0)
    src = torch.arange(int(new_off[-1]), device=xy.device) + torch.repeat_interleave(start - new_off[:-1], size)
    out_xy = xy[src].contiguous()
    some = size > 0  # (the gather is this tool's own: its first and last coordinate of every row are checked before it is used)
    assert bool((out_xy[new_off[:-1][some]] == xy[start[some]]).all()) and bool((out_xy[new_off[1:][some] - 1] == xy[(start + size)[some] - 1]).all())
    return DeviceGeoArray.from_device_buffers(_abi.GEOM_LINESTRING, out_xy, geom_offsets=new_off.to(torch.int32))


def run(name, steps, warmup, sample, piece):
    lib = _abi.lib()
    label, make = WORKLOADS[name]
    lines_h, polys_h = make()
    stream = torch.cuda.current_stream().cuda_stream
    lines, polys = DeviceGeoArray.upload(lines_h, stream=stream), DeviceGeoArray.upload(polys_h, stream=stream)
    torch.cuda.synchronize()
    idx = SpatialIndex.from_device(polys, stream=stream, for_points=False)
    n = len(lines_h)
    counts = torch.empty(n, dtype=torch.int32, device="cuda:0")
    out = {"workload": name, "what": label, "n_lines": n, "n_polys": len(polys_h), "mean_line_coords": round(lines_h.n_coords / n, 1),
           "mean_poly_coords": round(polys_h.n_coords / len(polys_h), 1), "steps": steps, "warmup": warmup}

    h = relation_pairs_device(lines, polys, idx, "intersects", counts, None, stream=stream)
    pairs = torch.empty((max(h, 1), 2), dtype=torch.int32, device="cuda:0")
    masks = torch.empty(max(h, 1), dtype=torch.uint8, device="cuda:0")
    join = lambda: relation_pairs_device(lines, polys, idx, "intersects", counts, pairs, masks, stream=stream)  # noqa: E731
    join()
    torch.cuda.synchronize()
    li, pi = pairs[:h, 0].contiguous(), pairs[:h, 1].contiguous()
    out["pairs"] = int(h)

    # ---- the cross-checks, on every returned pair (the measure in slices: its line column is gathered per pair)
    inside = line_clip_pairs_device(lines, polys, li, pi, "intersection", stream=stream)
    outside = line_clip_pairs_device(lines, polys, li, pi, "difference", stream=stream)
    len_l = lengths(lib, lines)[li.long()]
    len_in, len_out = lengths(lib, inside.device()), lengths(lib, outside.device())
    xy_l = torch.from_numpy(lines_h.xy).cuda()
    off_l = torch.from_numpy(lines_h.geom_offsets).cuda()
    measure = torch.empty(h, dtype=torch.float64, device="cuda:0")
    for k0 in range(0, h, piece):
        k1 = min(h, k0 + piece)
        sub = gathered_lines(xy_l, off_l, li[k0:k1])
        _abi.check(lib.gpk_intersection_measure(sub.handle, polys.handle, pi[k0:k1].contiguous().data_ptr(), measure[k0:k1].data_ptr(), _abi.MEM_DEVICE, None))
        torch.cuda.synchronize()
        sub.free()
    err_in, err_sum = ((len_in - measure).abs() / len_l).max(), ((len_in + len_out - len_l).abs() / len_l).max()
    assert float(err_in) <= 2e-9, f"length(intersection) differs from intersection_length: worst {float(err_in):.3e} of length(L)"
    assert float(err_sum) <= 2e-9, f"inside + outside differs from the line: worst {float(err_sum):.3e} of length(L)"
    m = masks[:h]

    def non_empty(how):  # which pairs have a part: the map of DROP_EMPTY, on the device
        src = torch.empty(max(h, 1), dtype=torch.int32, device="cuda:0")
        kept = line_clip_pairs_device(lines, polys, li, pi, how, drop_empty=True, out_src=src, stream=stream)
        torch.cuda.synchronize()
        has = torch.zeros(h, dtype=torch.bool, device="cuda:0")
        has[src[: len(kept)].long()] = True
        kept.device().free()
        return has

    has_in, has_out = non_empty("intersection"), non_empty("difference")
    assert bool(((m & 3) != 0)[has_in].all()), "a non-empty intersection whose mask does not intersect"
    assert bool((~has_out == ((m != 0) & ((m & 4) == 0))).all()), "the difference is empty exactly for covered_by rows"
    out.update(worst_inside_vs_measure=float(err_in), worst_inside_plus_outside=float(err_sum), pairs_with_a_piece=int(has_in.sum()),
               out_coords=int(inside.device().n_coords), out_bytes=int(inside.device().nbytes()))
    inside.device().free()
    outside.device().free()

    # ---- timings
    def clip_all(rows_l=li, rows_p=pi, how="intersection", drop=False):
        r = line_clip_pairs_device(lines, polys, rows_l, rows_p, how, drop_empty=drop, stream=stream)
        r.device().free()

    out["clip_ms_median"], out["clip_ms_min"] = timed(clip_all, steps, warmup)
    out["clip_drop_empty_ms_median"], _ = timed(lambda: clip_all(drop=True), steps, warmup)
    out["clip_difference_ms_median"], _ = timed(lambda: clip_all(how="difference"), steps, warmup)
    out["clip_stage_ms"] = stages(lib, clip_all)
    k = min(h, sample)
    sub = gathered_lines(xy_l, off_l, li[:k])
    sub_p = pi[:k].contiguous()
    sub_l = li[:k].contiguous()
    mbuf = torch.empty(k, dtype=torch.float64, device="cuda:0")
    measure_call = lambda: _abi.check(lib.gpk_intersection_measure(sub.handle, polys.handle, sub_p.data_ptr(), mbuf.data_ptr(), _abi.MEM_DEVICE, None))  # noqa: E731
    out["sample_pairs"] = int(k)
    out["sample_measure_ms_median"], out["sample_measure_ms_min"] = timed(measure_call, steps, warmup)
    out["sample_clip_ms_median"], out["sample_clip_ms_min"] = timed(lambda: clip_all(sub_l, sub_p), steps, warmup)
    out["sample_clip_over_measure"] = round(out["sample_clip_ms_median"] / out["sample_measure_ms_median"], 3)
    out["join_intersects_with_masks_ms_median"], out["join_intersects_with_masks_ms_min"] = timed(join, steps, warmup)
    sub.free()
    idx.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=200_000, help="pairs the measure and the clip are timed on side by side")
    ap.add_argument("--piece", type=int, default=50_000, help="pairs per call of the measure in the cross-check (its line column is gathered per pair)")
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
