#!/usr/bin/env python3
"""Point predicate join (gpk_point_relation_join) timings on device-resident data (a secondary measurement: bench.py is unchanged).

    python tools/bench_pointrel.py [--steps 5] [--warmup 2] [--only c2|c3|dups|mpt] >> profiles/pointrel_bench.jsonl

Workloads:
    c2    C2's data: 10M uniform points x 1000 star polygons of 64 vertices (intersects, within, touches)
    c3    1M points x C3's 100k random linestrings; one point in ten sits on a vertex of a line, one in a hundred on a line's end
          (intersects, within, touches: which lines END at the point, which pass through it)
    dups  1M x 1M points, half of the right ones copies of left ones (equals, intersects)
    mpt   100k multipoints of 64 points x C4's 100k clustered polygons (intersects, within, crosses)
The right side's index (GPK_INDEX_BBOX_GRID; for c2 also the point-in-polygon tables gpk_spatial_join reads) is built once beforehand;
each step is one whole synchronous call into device buffers sized by a count-only call, timed with HIP events on the stream.  The
lines to measure against are gpk_dwithin_join at distance 0 on the same columns and index (same candidates, more arithmetic) and, for
c2, gpk_spatial_join(intersects) (the tuned single-cell path).  Before a time is printed the `intersects` pair set is compared element
by element with both, and the tool stops when they differ.  No time is a pass / fail gate.
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
from geopolars_amd.geoarrow import DeviceGeoArray, GeoArrowArray  # noqa: E402
from geopolars_amd.spatial_index import SpatialIndex, dwithin_pairs_device, join_pairs_device, point_relation_pairs_device  # noqa: E402

STAGES = ["gpk_bounds", "gpk_bbox_cand_count", "gpk_cand_compact", "gpk_bbox_cand_fill", "gpk_point_relation_refine", "gpk_point_relation_refine_large",
          "gpk_pair_count", "gpk_pair_emit", "gpk_point_relation_gather", "gpk_dwithin_grow", "gpk_dwithin_refine", "gpk_dwithin_refine_large"]


def _c2():
    return synth.uniform_points(10_000_000), synth.star_polygons(1000, 64), ("intersects", "within", "touches"), True


def _c3():
    lines = synth.random_linestrings(100_000)
    rng = np.random.default_rng(7)
    xy = rng.uniform(0.0, synth.DOMAIN, (1_000_000, 2))
    on = rng.integers(0, lines.n_coords, 100_000)
    xy[::10] = lines.xy[on]
    xy[::100] = lines.xy[lines.geom_offsets[rng.integers(0, len(lines), 10_000)]]
    return GeoArrowArray.from_points(xy), lines, ("intersects", "within", "touches"), False


def _dups():
    rng = np.random.default_rng(8)
    left = rng.uniform(0.0, synth.DOMAIN, (1_000_000, 2))
    right = rng.uniform(0.0, synth.DOMAIN, (1_000_000, 2))
    right[::2] = left[rng.integers(0, len(left), len(right) // 2)]
    return GeoArrowArray.from_points(left), GeoArrowArray.from_points(right), ("equals", "intersects"), False


def _mpt():
    polys = synth.clustered_polygons(100_000, seed=41, mean_neighbours=4.0)
    rng = np.random.default_rng(9)
    n, k = 100_000, 64
    centre = rng.uniform(0.0, synth.DOMAIN, (n, 1, 2))
    xy = (centre + rng.normal(0.0, synth.DOMAIN / np.sqrt(n), (n, k, 2))).reshape(-1, 2)
    return GeoArrowArray(_abi.GEOM_MULTIPOINT, xy, geom_offsets=np.arange(0, n * k + 1, k, dtype=np.int32)), polys, ("intersects", "within", "crosses"), False


WORKLOADS = {"c2": ("10M uniform points x 1000 star polygons of 64 vertices (C2's data)", _c2),
             "c3": ("1M points (10 % on line vertices) x 100k random linestrings (C3's right side)", _c3),
             "dups": ("1M x 1M points, half of the right ones copies of left ones", _dups),
             "mpt": ("100k multipoints of 64 points x 100k clustered polygons (C4's side)", _mpt)}


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
    left_h, right_h, predicates, with_spatial_join = make()
    stream = torch.cuda.current_stream().cuda_stream
    left, right = DeviceGeoArray.upload(left_h, stream=stream), DeviceGeoArray.upload(right_h, stream=stream)
    torch.cuda.synchronize()
    idx = SpatialIndex.from_device(right, stream=stream, for_points=with_spatial_join)
    n = len(left_h)
    counts = torch.empty(n, dtype=torch.int32, device="cuda:0")
    out = {"workload": name, "what": label, "n_left": n, "n_right": len(right_h), "mean_left_coords": round(left_h.n_coords / n, 1),
           "mean_right_coords": round(right_h.n_coords / len(right_h), 1), "steps": steps, "warmup": warmup}
    ours = None
    for pred in predicates:
        h = point_relation_pairs_device(left, right, idx, pred, counts, None, stream=stream)
        pairs = torch.empty((max(h, 1), 2), dtype=torch.int32, device="cuda:0")
        masks = torch.empty(max(h, 1), dtype=torch.uint8, device="cuda:0")
        plain = lambda: point_relation_pairs_device(left, right, idx, pred, counts, pairs, stream=stream)  # noqa: E731
        with_masks = lambda: point_relation_pairs_device(left, right, idx, pred, counts, pairs, masks, stream=stream)  # noqa: E731
        r = {"pairs": int(h)}
        r["ms_median"], r["ms_min"] = timed(plain, steps, warmup)
        r["with_masks_ms_median"], _ = timed(with_masks, steps, warmup)
        r["stage_ms"] = stages(lib, plain)
        r["refine_share"] = round(r["stage_ms"].get("gpk_point_relation_refine", 0.0) / r["ms_median"], 3)
        with_masks()
        torch.cuda.synchronize()
        r["mask_histogram"] = torch.bincount(masks[:h].long(), minlength=16).tolist()
        if pred == "intersects":
            plain()
            torch.cuda.synchronize()
            ours = pairs[:h].clone()
        out[pred] = r
    h = out["intersects"]["pairs"]
    # the within-distance join at distance 0: same candidates, more arithmetic
    hd = dwithin_pairs_device(left, right, idx, 0.0, counts, None, stream=stream)
    dpairs = torch.empty((max(hd, 1), 2), dtype=torch.int32, device="cuda:0")
    dw = lambda: dwithin_pairs_device(left, right, idx, 0.0, counts, dpairs, stream=stream)  # noqa: E731
    dw()
    torch.cuda.synchronize()
    out["dwithin0_pairs"] = int(hd)
    out["dwithin0_pairs_equal"] = bool(hd == h and torch.equal(ours, dpairs[:hd]))
    assert out["dwithin0_pairs_equal"], f"{name}: the intersects pair set ({h}) differs from dwithin at 0 ({hd})"
    out["dwithin0_ms_median"], out["dwithin0_ms_min"] = timed(dw, steps, warmup)
    out["dwithin0_stage_ms"] = stages(lib, dw)
    out["intersects_over_dwithin0"] = round(out["intersects"]["ms_median"] / out["dwithin0_ms_median"], 3)
    if with_spatial_join:  # the tuned point x polygon join
        hs = join_pairs_device(left, right, idx, "intersects", counts, None, stream=stream)
        spairs = torch.empty((max(hs, 1), 2), dtype=torch.int32, device="cuda:0")
        sj = lambda: join_pairs_device(left, right, idx, "intersects", counts, spairs, stream=stream)  # noqa: E731
        sj()
        torch.cuda.synchronize()
        out["spatial_join_pairs"] = int(hs)
        out["spatial_join_pairs_equal"] = bool(hs == h and torch.equal(ours, spairs[:hs]))
        assert out["spatial_join_pairs_equal"], f"{name}: the intersects pair set ({h}) differs from gpk_spatial_join's ({hs})"
        out["spatial_join_ms_median"], out["spatial_join_ms_min"] = timed(sj, steps, warmup)
        out["intersects_over_spatial_join"] = round(out["intersects"]["ms_median"] / out["spatial_join_ms_median"], 3)
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
