#!/usr/bin/env python3
"""Line x line predicate join (gpk_line_relation_join) timings on device-resident data (a secondary measurement: bench.py is
unchanged).

    python tools/bench_linerel.py [--steps 5] [--warmup 2] [--only lines|self] >> profiles/linerel_bench.jsonl

Workloads: the `lines` workload of tools/bench_dwithin.py (100k x 100k synth.random_linestrings, seeds 0 and 1) and a self-join of the
100k left lines.  The right side's index (GPK_INDEX_BBOX_GRID) is built once beforehand; each step is one whole synchronous call into
device buffers sized by a count-only call, timed with HIP events on the stream.  Per workload and predicate (intersects, crosses,
touches, overlaps): the join without and with the per-pair masks and the refine kernel's share of it.  The line to measure against is
gpk_dwithin_join at distance 0 on the same columns and index, the only route to "which lines meet" before.  The two `intersects` pair
sets are compared element by element, and the tool stops before it prints a time when they differ.
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
from geopolars_amd.spatial_index import SpatialIndex, dwithin_pairs_device, line_relation_pairs_device  # noqa: E402

STAGES = ["gpk_bounds", "gpk_bbox_cand_count", "gpk_cand_compact", "gpk_bbox_cand_fill", "gpk_line_relation_refine", "gpk_pair_refine", "gpk_pair_count",
          "gpk_pair_emit", "gpk_line_relation_gather", "gpk_dwithin_grow", "gpk_dwithin_refine", "gpk_dwithin_refine_large"]
PREDICATES = ("intersects", "crosses", "touches", "overlaps")


def _lines():
    return synth.random_linestrings(100_000), synth.random_linestrings(100_000, seed=1)


def _self():
    return synth.random_linestrings(100_000), None


WORKLOADS = {"lines": ("100k x 100k random linestrings (the lines workload of bench_dwithin.py)", _lines), "self": ("100k random linestrings against themselves", _self)}


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
    left = DeviceGeoArray.upload(left_h, stream=stream)
    right = left if right_h is None else DeviceGeoArray.upload(right_h, stream=stream)
    right_h = left_h if right_h is None else right_h
    torch.cuda.synchronize()
    idx = SpatialIndex.from_device(right, stream=stream, for_points=False)
    n = len(left_h)
    counts = torch.empty(n, dtype=torch.int32, device="cuda:0")
    out = {"workload": name, "what": label, "n_left": n, "n_right": len(right_h), "mean_left_coords": round(left_h.n_coords / n, 1),
           "mean_right_coords": round(right_h.n_coords / len(right_h), 1), "steps": steps, "warmup": warmup}
    ours = None
    for pred in PREDICATES:
        h = line_relation_pairs_device(left, right, idx, pred, counts, None, stream=stream)
        pairs = torch.empty((max(h, 1), 2), dtype=torch.int32, device="cuda:0")
        masks = torch.empty(max(h, 1), dtype=torch.uint8, device="cuda:0")
        plain = lambda: line_relation_pairs_device(left, right, idx, pred, counts, pairs, stream=stream)  # noqa: E731
        with_masks = lambda: line_relation_pairs_device(left, right, idx, pred, counts, pairs, masks, stream=stream)  # noqa: E731
        r = {"pairs": int(h)}
        r["ms_median"], r["ms_min"] = timed(plain, steps, warmup)
        r["with_masks_ms_median"], _ = timed(with_masks, steps, warmup)
        r["stage_ms"] = stages(lib, plain)
        r["with_masks_stage_ms"] = stages(lib, with_masks)
        r["refine_share"] = round(r["stage_ms"].get("gpk_line_relation_refine", 0.0) / r["ms_median"], 3)
        with_masks()
        torch.cuda.synchronize()
        r["mask_histogram"] = torch.bincount(masks[:h].long(), minlength=128).tolist()
        if pred == "intersects":
            plain()
            torch.cuda.synchronize()
            ours = pairs[:h].clone()
        out[pred] = r
    h = out["intersects"]["pairs"]
    # the within-distance join at distance 0: the only route to per-pair information before
    hd = dwithin_pairs_device(left, right, idx, 0.0, counts, None, stream=stream)
    dpairs = torch.empty((max(hd, 1), 2), dtype=torch.int32, device="cuda:0")
    dw = lambda: dwithin_pairs_device(left, right, idx, 0.0, counts, dpairs, stream=stream)  # noqa: E731
    out["dwithin0_pairs"] = int(hd)
    out["dwithin0_ms_median"], out["dwithin0_ms_min"] = timed(dw, steps, warmup)
    out["dwithin0_stage_ms"] = stages(lib, dw)
    dw()
    torch.cuda.synchronize()
    out["dwithin0_pairs_equal"] = bool(hd == h and torch.equal(ours, dpairs[:hd]))
    assert out["dwithin0_pairs_equal"], f"{name}: the intersects pair set ({h}) differs from dwithin at 0 ({hd})"
    out["intersects_over_dwithin0"] = round(out["intersects"]["ms_median"] / out["dwithin0_ms_median"], 3)
    out["intersects_with_masks_over_dwithin0"] = round(out["intersects"]["with_masks_ms_median"] / out["dwithin0_ms_median"], 3)
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
