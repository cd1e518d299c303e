#!/usr/bin/env python3
"""Row-wise distance between two non-point columns (gpk_distance_rowwise -> gpk_pairdist.hip) on device-resident data (a secondary
measurement: bench.py is unchanged).

    python tools/bench_distance_pairs.py [--steps 10] [--warmup 2] [--only clustered|stars|lines|powerlaw] > profiles/<name>_pairdist_bench.jsonl

Workloads: 1M synth.clustered_polygons, row i against row i + 1 (touching and near neighbours); 1M 64-vertex star polygons, row i
against a random row (mostly far apart: full sweeps); 100k x 100k synth.random_linestrings (4 - 256 segments), permuted;
100k synth.powerlaw_multipolygons (capped at 4096 vertices) x 100k star polygons.  Both columns and the row map live on the device;
each step is one call with a device output, timed with HIP events on the stream.  Per workload one JSON line: ms per call (median,
min), rows/s, the segment pairs a full sweep evaluates (sum of n_A * n_B, counted on the host from the offsets), the share of rows
that came out 0, and the rows sent to the work-group schedule (n_A * n_B > PD_LARGE_COST, restated here).
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

LARGE_COST = 1 << 16  # gpk_pairdist.hip PD_LARGE_COST


def _row_coords(a) -> np.ndarray:
    off = a.geom_offsets.astype(np.int64)
    for inner in (a.part_offsets, a.ring_offsets):
        if inner is not None:
            off = inner.astype(np.int64)[off]
    return np.diff(off)


def _stars(n, seed):
    return synth.star_polygons(n, 64, seed=seed)


WORKLOADS = {
    "clustered": ("1M clustered polygons, row i x row i+1",
                  lambda: (lambda a: (a, a, (np.arange(len(a)) + 1) % len(a)))(synth.clustered_polygons(1_000_000))),
    "stars": ("1M 64-vertex star polygons x a random row",
              lambda: (lambda a: (a, a, np.random.default_rng(1).integers(0, len(a), len(a))))(_stars(1_000_000, 7))),
    "lines": ("100k x 100k random linestrings, permuted",
              lambda: (lambda a: (a, a, np.random.default_rng(2).permutation(len(a))))(synth.random_linestrings(100_000))),
    "powerlaw": ("100k power-law multipolygons (cap 4096) x 100k star polygons",
                 lambda: (synth.powerlaw_multipolygons(100_000, cap=4096), _stars(100_000, 8), None)),
}


def run(name, steps, warmup):
    label, make = WORKLOADS[name]
    a_h, b_h, rows_h = make()
    stream = torch.cuda.current_stream().cuda_stream
    a = DeviceGeoArray.upload(a_h, stream=stream)
    b = a if b_h is a_h else DeviceGeoArray.upload(b_h, stream=stream)
    n = len(a_h)
    rows = None if rows_h is None else torch.from_numpy(np.ascontiguousarray(rows_h, dtype=np.int64).astype(np.uint32).view(np.int32)).to("cuda:0")
    out = torch.empty(n, dtype=torch.float64, device="cuda:0")
    lib = _abi.lib()

    def call():
        _abi.check(lib.gpk_distance_rowwise(a.handle, b.handle, None if rows is None else C.c_void_p(rows.data_ptr()), C.c_void_p(out.data_ptr()),
                                            _abi.MEM_DEVICE, C.c_void_p(stream)))

    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    d = out.cpu().numpy()
    na = _row_coords(a_h)
    nb = _row_coords(b_h)
    nb = nb if rows_h is None else nb[np.asarray(rows_h, dtype=np.int64)]
    cost = na.astype(np.int64) * nb.astype(np.int64)
    ms = float(np.median(times))
    return {
        "workload": name,
        "what": label,
        "rows": n,
        "ms_per_call_median": round(ms, 4),
        "ms_per_call_min": round(float(np.min(times)), 4),
        "rows_per_s": round(n / (ms * 1e-3), 1),
        "segment_pairs_full_sweep": int(cost.sum()),
        "zero_share": round(float(np.mean(d == 0.0)), 4),
        "nan_rows": int(np.isnan(d).sum()),
        "large_rows": int(np.count_nonzero(cost > LARGE_COST)),
        "steps": steps,
        "warmup": warmup,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=sorted(WORKLOADS), action="append")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    name, cus = _abi.device_info()
    for w in a.only or ["clustered", "stars", "lines", "powerlaw"]:
        r = run(w, a.steps, a.warmup)
        r["device"] = f"{name} ({cus} CUs)"
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
