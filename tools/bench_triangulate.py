#!/usr/bin/env python3
"""Polygon triangulation (gpk_triangulate) timings on device-resident data (a secondary measurement: bench.py is unchanged).

    python tools/bench_triangulate.py [--steps 5] [--warmup 2] [--only c4|stars|powerlaw|rings4096] >> profiles/triangulate_bench.jsonl

Workloads: benchmark config C4's clustered polygons (1M rows), 2M star polygons of 64 vertices, power-law multipolygons (rings of at
most 10^4 coordinates: the rows above 5000 node slots keep their list in global scratch), and 512 rings of 4096 coordinates (the
work-group path).  A step is one call with indices, offsets and status in device buffers (capacity n_coords + 3 n_rings: no size query),
timed with HIP events on the stream.  Before a time is printed the answer is checked: every row gpk_validity calls valid has status 0
and at most its share of triangles, and on 10 000 sampled rows the float sum of the triangle areas equals gpk_area within 1e-9
relative.  There is no pass threshold: nothing comparable exists before this call.  As context every line carries gpk_validity and
gpk_convex_hull on the same column — the two existing exact O(n^2) / constructive neighbours — and the per-kernel times.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_validity import WORKLOADS, timed  # noqa: E402
from geopolars_amd import _abi  # noqa: E402
from geopolars_amd.geoarrow import DeviceGeoArray  # noqa: E402

STAGES = ["gpk_triangulate", "gpk_triangulate_large", "gpk_triangulate_huge", "gpk_triangulate_gather"]


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


def verify(host, xy, index, offsets, status, code, area):
    """the checks that come before a time; returns (valid rows, failed valid rows, worst relative area error on the sample)"""
    n = len(host)
    valid = code == 0
    counts = (offsets[1:] - offsets[:-1]).long()
    ro = torch.from_numpy(host.ring_offsets.astype(np.int64)).cuda()
    if host.geom_type == _abi.GEOM_MULTIPOLYGON:
        first_ring = torch.from_numpy(host.part_offsets.astype(np.int64)).cuda()[torch.from_numpy(host.geom_offsets.astype(np.int64)).cuda()]
    else:
        first_ring = torch.from_numpy(host.geom_offsets.astype(np.int64)).cuda()
    share = (ro[first_ring[1:]] - ro[first_ring[:-1]]) + 3 * (first_ring[1:] - first_ring[:-1])
    has = area > 0  # (a valid row without a non-empty member is GPK_TRI_EMPTY)
    bad = valid & has & (status != 0)
    assert not bool((valid & (counts > share)).any()), "a valid row above its share"
    assert int(bad.sum()) == 0, f"{int(bad.sum())} valid rows without status 0, the first: row {int(torch.nonzero(bad)[0])}"
    rows = torch.nonzero(valid & has).flatten()
    pick = rows[torch.from_numpy(np.random.default_rng(3).choice(len(rows), min(10_000, len(rows)), replace=False)).cuda()]
    # the triangles of the sampled rows only (a gather through all 10^8 index triples at once is more than the sample needs)
    c = counts[pick]
    slot = torch.repeat_interleave(torch.arange(len(pick), device="cuda"), c)
    first = torch.repeat_interleave(offsets[:-1].long()[pick] - (torch.cumsum(c, 0) - c), c)
    p = xy[index[first + torch.arange(len(slot), device="cuda")].long()]  # (t, 3, 2)
    a2 = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])
    total = torch.zeros(n, dtype=torch.float64, device="cuda").index_add_(0, pick[slot], 0.5 * a2)
    err = ((total[pick] - area[pick]).abs() / area[pick]).max().item()
    assert err <= 1e-9, f"sum of triangle areas against gpk_area: {err:.3g} relative"
    return int(valid.sum()), int(bad.sum()), err


def run(name, steps, warmup):
    lib = _abi.lib()
    label, make = WORKLOADS[name]
    host = make()
    stream = torch.cuda.current_stream().cuda_stream
    dev = DeviceGeoArray.upload(host, stream=stream)
    torch.cuda.synchronize()
    n, cap = len(host), host.n_coords + 3 * host.n_rings
    index = torch.empty((cap, 3), dtype=torch.int32, device="cuda:0")
    offsets = torch.empty(n + 1, dtype=torch.int32, device="cuda:0")
    status = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    code = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    area = torch.empty(n, dtype=torch.float64, device="cuda:0")
    hull_xy = torch.empty((host.n_coords + n, 2), dtype=torch.float64, device="cuda:0")
    hull_off = torch.empty(n + 1, dtype=torch.int32, device="cuda:0")
    total = C.c_int64(0)
    tri = lambda: _abi.check(lib.gpk_triangulate(dev.handle, index.data_ptr(), cap, offsets.data_ptr(), status.data_ptr(), C.byref(total), _abi.MEM_DEVICE, stream))  # noqa: E731
    validity = lambda: _abi.check(lib.gpk_validity(dev.handle, code.data_ptr(), None, _abi.MEM_DEVICE, stream))  # noqa: E731
    hull = lambda: _abi.check(lib.gpk_convex_hull(dev.handle, hull_xy.data_ptr(), hull_off.data_ptr(), _abi.MEM_DEVICE, stream))  # noqa: E731
    out = {"workload": name, "what": label, "rows": n, "mean_coords": round(host.n_coords / n, 1), "steps": steps, "warmup": warmup}
    tri()
    validity()
    _abi.check(lib.gpk_area(dev.handle, area.data_ptr(), _abi.MEM_DEVICE, stream))
    torch.cuda.synchronize()
    out["triangles"] = int(total.value)
    out["valid_rows"], _, out["worst_area_error"] = verify(host, torch.from_numpy(host.xy).cuda(), index[: total.value], offsets, status, code, area)
    out["status_histogram"] = torch.bincount(status.long(), minlength=3).tolist()
    out["ms_median"], out["ms_min"] = timed(tri, steps, warmup)
    print(f"{name}: gpk_triangulate {out['ms_median']} ms", file=sys.stderr, flush=True)
    out["stage_ms"] = stages(lib, tri)
    out["validity_ms_median"], _ = timed(validity, steps, warmup)
    out["convex_hull_ms_median"], _ = timed(hull, steps, warmup)
    out["triangulate_over_validity"] = round(out["ms_median"] / out["validity_ms_median"], 2)
    out["triangulate_over_convex_hull"] = round(out["ms_median"] / out["convex_hull_ms_median"], 2)
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
