#!/usr/bin/env python3
"""Take and filter of geometry rows (gpk_geoarray_take / gpk_geoarray_filter) on device-resident columns (a secondary measurement:
bench.py is unchanged).

    python tools/bench_take.py [--steps 5] [--warmup 2] [--only points|poly8|poly64|c4|powerlaw] >> profiles/take_bench.jsonl

Columns: 10M points, 8M x 8-vertex polygons, 2M x 64-vertex polygons, benchmark config C4's 1M clustered polygons, 1M power-law
multipolygons.  Index lists (device-resident): identity, sorted with repeats, a random permutation; plus filter at 0.5 (a device bool
mask).  Before anything is timed the result is asserted against GeoArrowArray.take: in full for the smallest column, and for the
others the totals of every level plus 10 000 sampled rows of the result.  Two yardsticks on the same column: gpk_geoarray_concat of the
single column — a plain device copy of the same bytes: the floor — and the route a caller had before: gpk_geoarray_to_wkb, then
gpk_take_binary, then gpk_geoarray_from_wkb (skipped, and said so, where the WKB column exceeds i32 offsets).  Times: HIP events, per
call around the whole call (its one wait and the result's allocation and release included) and per kernel through gpk_profile_query;
medians of --steps after --warmup.  Bytes moved: the result's buffers read once and written once, plus the index list."""
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

STAGES = ["gpk_geotake_count", "gpk_geotake_totals", "gpk_geotake_rows", "gpk_geotake_bitmap", "gpk_geotake_strips", "gpk_geotake_offsets", "gpk_geotake_coords",
          "gpk_scan_partial", "gpk_scan_totals", "gpk_scan_final"]

WORKLOADS = {
    "points": ("10M points", lambda: synth.uniform_points(10_000_000, seed=3)),
    "poly8": ("8M polygons of 8 vertices", lambda: synth.star_polygons(8_000_000, 8, seed=5)),
    "poly64": ("2M polygons of 64 vertices", lambda: synth.star_polygons(2_000_000, 64, seed=7)),
    "c4": ("1M clustered polygons (benchmark config C4)", lambda: synth.clustered_polygons(1_000_000, seed=41, mean_neighbours=4.0)),
    "powerlaw": ("1M power-law multipolygons", lambda: synth.powerlaw_multipolygons(1_000_000, seed=9)),
}
SMALLEST = "points"  # by bytes: checked in full


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
    return round(float(np.median(out)), 4)


def stage_medians(lib, call, steps):
    """per-kernel HIP-event times of `steps` profiled calls: the median over the calls of each stage's sum"""
    runs = {k: [] for k in STAGES}
    for _ in range(steps):
        lib.gpk_profile_reset()
        lib.gpk_profile_filter(b"")
        lib.gpk_profile_enable(1)
        call()
        lib.gpk_profile_enable(0)
        torch.cuda.synchronize()
        for k in STAGES:
            ms, cnt = C.c_double(0), C.c_int64(0)
            lib.gpk_profile_query(k.encode(), C.byref(ms), C.byref(cnt))
            if cnt.value:
                runs[k].append(ms.value)
    lib.gpk_profile_reset()
    return {k: round(float(np.median(v)), 4) for k, v in runs.items() if v}


def _levels(a: GeoArrowArray):
    return [o for o in (a.geom_offsets, a.part_offsets, a.ring_offsets) if o is not None]


def assert_same(got: GeoArrowArray, want: GeoArrowArray, what):
    assert got.geom_type == want.geom_type and len(got) == len(want), what
    for g, w in zip(_levels(got), _levels(want)):
        assert np.array_equal(g, w), what
    assert got.xy.shape == want.xy.shape and bool((got.xy.view(np.uint64) == want.xy.view(np.uint64)).all()), what
    assert np.array_equal(got.is_valid(), want.is_valid()), what


def check(name, host: GeoArrowArray, dev: DeviceGeoArray, idx: np.ndarray, got: DeviceGeoArray, rng):
    """`got` = take(dev, idx) against the host: in full for the smallest column, else its totals and 10 000 sampled rows"""
    if name == SMALLEST:
        assert_same(got.download(), host.take(idx), name)
        return "full"
    lo, hi = idx.astype(np.int64), idx.astype(np.int64) + 1
    for off in _levels(host):  # the coordinates of every row: down the first and last child of each level
        lo, hi = off[lo].astype(np.int64), off[hi].astype(np.int64)
    n_coords = int((hi - lo).sum()) if _levels(host) else len(idx)
    assert (got.n_geoms, got.n_coords) == (len(idx), n_coords), (name, got.n_geoms, got.n_coords, len(idx), n_coords)
    sample = np.sort(rng.choice(len(idx), size=min(10_000, len(idx)), replace=False)).astype(np.int64)
    assert_same(got.take(sample).download(), host.take(idx[sample]), name)
    return "totals + 10000 sampled rows"


def wkb_route(lib, dev: DeviceGeoArray, idx_dev, stream):
    """to_wkb -> take_binary -> from_wkb, all buffers on the device; returns the callable, or the refusal's text"""
    n, n_idx = dev.n_geoms, int(idx_dev.numel())
    off = torch.empty(n + 1, dtype=torch.int32, device="cuda:0")
    nb = C.c_int64(0)
    rc = lib.gpk_geoarray_to_wkb(dev.handle, off.data_ptr(), None, 0, C.byref(nb), _abi.MEM_DEVICE, stream)
    if rc != _abi.GPK_OK:
        return None, _abi.last_error()
    values = torch.empty(max(int(nb.value), 1), dtype=torch.uint8, device="cuda:0")
    out_off = torch.empty(n_idx + 1, dtype=torch.int32, device="cuda:0")
    ob = C.c_int64(0)
    _abi.check(lib.gpk_geoarray_to_wkb(dev.handle, off.data_ptr(), values.data_ptr(), values.numel(), C.byref(nb), _abi.MEM_DEVICE, stream))
    rc = lib.gpk_take_binary(values.data_ptr(), off.data_ptr(), None, n, idx_dev.data_ptr(), n_idx, out_off.data_ptr(), None, 0, C.byref(ob), None, _abi.MEM_DEVICE, stream)
    if rc != _abi.GPK_OK:
        return None, _abi.last_error()
    out_values = torch.empty(max(int(ob.value), 1), dtype=torch.uint8, device="cuda:0")

    def call():
        _abi.check(lib.gpk_geoarray_to_wkb(dev.handle, off.data_ptr(), values.data_ptr(), values.numel(), C.byref(nb), _abi.MEM_DEVICE, stream))
        _abi.check(lib.gpk_take_binary(values.data_ptr(), off.data_ptr(), None, n, idx_dev.data_ptr(), n_idx, out_off.data_ptr(), out_values.data_ptr(),
                                       out_values.numel(), C.byref(ob), None, _abi.MEM_DEVICE, stream))
        h, gt = C.c_void_p(), C.c_int32(-1)
        _abi.check(lib.gpk_geoarray_from_wkb(out_values.data_ptr(), out_off.data_ptr(), n_idx, None, _abi.MEM_DEVICE, stream, C.byref(h), C.byref(gt)))
        lib.gpk_geoarray_free(h)

    return call, None


def run(name, steps, warmup):
    lib = _abi.lib()
    label, make = WORKLOADS[name]
    host = make()
    stream = torch.cuda.current_stream().cuda_stream
    dev = DeviceGeoArray.upload(host, stream=stream)
    torch.cuda.synchronize()
    n = len(host)
    rng = np.random.default_rng(1)
    lists = {"identity": np.arange(n, dtype=np.int64), "sorted_repeats": np.sort(rng.integers(0, n, n)).astype(np.int64), "permutation": rng.permutation(n).astype(np.int64)}
    out = {"workload": name, "what": label, "n_rows": n, "n_coords": host.n_coords, "column_bytes": host.nbytes(), "steps": steps, "warmup": warmup, "lists": {}}

    def free_after(make_result):
        def call():
            make_result().free()
        return call

    for what, idx in lists.items():
        idx_dev = torch.from_numpy(idx).cuda()
        got = dev.take(idx_dev, stream=stream)
        checked = check(name, host, dev, idx, got, rng)
        moved = 2 * got.nbytes() + idx.nbytes
        got.free()
        take = free_after(lambda: dev.take(idx_dev, stream=stream))
        r = {"checked": checked, "bytes_moved": moved, "call_ms": timed(take, steps, warmup), "stage_ms": stage_medians(lib, take, steps)}
        kernels = sum(r["stage_ms"].values())
        r["kernels_ms"] = round(kernels, 4)
        r["tb_s_call"], r["tb_s_kernels"] = round(moved / r["call_ms"] / 1e9, 3), round(moved / kernels / 1e9, 3)
        route, refusal = wkb_route(lib, dev, idx_dev, stream)
        if route is None:
            r["wkb_route"] = "refused: " + refusal
        else:
            r["wkb_route_ms"] = timed(route, steps, warmup)
        out["lists"][what] = r

    concat = free_after(lambda: DeviceGeoArray.concat([dev], stream=stream)[0])
    out["concat_ms"] = timed(concat, steps, warmup)
    out["concat_tb_s"] = round(2 * host.nbytes() / out["concat_ms"] / 1e9, 3)
    out["identity_over_concat"] = round(out["lists"]["identity"]["call_ms"] / out["concat_ms"], 3)

    mask = rng.uniform(size=n) < 0.5
    mask_dev = torch.from_numpy(mask).cuda()
    got = dev.filter(mask_dev, stream=stream)
    kept = np.nonzero(mask)[0].astype(np.int64)
    checked = check(name, host, dev, kept, got, rng)
    moved = 2 * got.nbytes() + mask.nbytes
    got.free()
    flt = free_after(lambda: dev.filter(mask_dev, stream=stream))
    r = {"checked": checked, "kept": int(mask.sum()), "bytes_moved": moved, "call_ms": timed(flt, steps, warmup), "stage_ms": stage_medians(lib, flt, steps)}
    r["kernels_ms"] = round(sum(r["stage_ms"].values()), 4)
    r["tb_s_call"], r["tb_s_kernels"] = round(moved / r["call_ms"] / 1e9, 3), round(moved / r["kernels_ms"] / 1e9, 3)
    out["filter_0.5"] = r
    dev.free()
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
