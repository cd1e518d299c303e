#!/usr/bin/env python3
"""Row-wise discrete Hausdorff and Frechet distance (gpk_hausdorff_distance -> gpk_hausdorff.hip, gpk_frechet_distance ->
gpk_frechet.hip) on device-resident data (a secondary measurement: bench.py is unchanged).

    python tools/bench_hausdorff.py [--steps 10] [--warmup 2] [--only lines_k1|lines_k4|clustered] [--rows N] > profiles/hausdorff_bench.jsonl

Workloads: 100k x 100k synth.random_linestrings (4 - 256 segments) with a permuted row map — the column of
tools/bench_distance_pairs.py — at subdivisions k = 1 and k = 4, both measures; 1M synth.clustered_polygons, row i against row i + 1,
Hausdorff only.  Both columns and the row map live on the device; each step is one call with a device output, timed with HIP events on
the stream.  Before a time is printed the device outputs are checked row by row: hausdorff >= gpk_distance_rowwise and frechet >=
hausdorff for every non-NaN row (the distance is a min of mins over terms of which the Hausdorff distance is a max of mins; every
Frechet coupling visits every sample of both sides).  Per workload one JSON line: ms per call (median, min) of each measure, and beside
them the time of gpk_distance_rowwise on the same columns — the number to set them against: it evaluates the same n_A * n_B
point-segment terms — with the ratios, the point-segment terms of a Hausdorff call and the cells of a Frechet call (counted on the
host from the offsets), and the rows each call sent to its list kernel (thresholds restated here).
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

HD_LARGE_COST = 1 << 16  # gpk_hausdorff.h
FR_LARGE_COST = 1 << 14  # gpk_frechet.h
FRECHET_MAX_SHORT = 16384  # GPK_FRECHET_MAX_SHORT


def _row_counts(a):
    """per row: coordinates and non-empty sequences"""
    off = a.geom_offsets.astype(np.int64)
    seq = off
    for inner in (a.part_offsets, a.ring_offsets):
        if inner is not None:
            seq = off
            off = inner.astype(np.int64)[off]
    coords = np.diff(off)
    if a.ring_offsets is None:  # LINESTRING: one sequence a row
        return coords, (coords > 0).astype(np.int64)
    lens = np.diff(a.ring_offsets.astype(np.int64))
    nonempty = np.concatenate([[0], np.cumsum(lens > 0)])
    return coords, nonempty[seq[1:]] - nonempty[seq[:-1]]


WORKLOADS = {
    "lines_k1": ("100k x 100k random linestrings, permuted, k = 1", 1, True,
                 lambda n: (lambda a: (a, np.random.default_rng(2).permutation(len(a))))(synth.random_linestrings(n or 100_000))),
    "lines_k4": ("100k x 100k random linestrings, permuted, k = 4", 4, True,
                 lambda n: (lambda a: (a, np.random.default_rng(2).permutation(len(a))))(synth.random_linestrings(n or 100_000))),
    "clustered": ("1M clustered polygons, row i x row i+1, k = 1", 1, False,
                  lambda n: (lambda a: (a, (np.arange(len(a)) + 1) % len(a)))(synth.clustered_polygons(n or 1_000_000))),
}


def timed(call, steps, warmup):
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
    return {"ms_median": float(np.median(times)), "ms_min": float(np.min(times))}


def run(name, steps, warmup, n_rows):
    label, k, with_frechet, make = WORKLOADS[name]
    a_h, rows_h = make(n_rows)
    stream = torch.cuda.current_stream().cuda_stream
    a = DeviceGeoArray.upload(a_h, stream=stream)
    n = len(a_h)
    rows = torch.from_numpy(np.ascontiguousarray(rows_h, dtype=np.int64).astype(np.uint32).view(np.int32)).to("cuda:0")
    d, h, f = (torch.full((n,), -1.0, dtype=torch.float64, device="cuda:0") for _ in range(3))
    lib = _abi.lib()
    r, s = C.c_void_p(rows.data_ptr()), C.c_void_p(stream)

    def distance():
        _abi.check(lib.gpk_distance_rowwise(a.handle, a.handle, r, C.c_void_p(d.data_ptr()), _abi.MEM_DEVICE, s))

    def hausdorff():
        _abi.check(lib.gpk_hausdorff_distance(a.handle, a.handle, r, k, C.c_void_p(h.data_ptr()), _abi.MEM_DEVICE, s))

    def frechet():
        _abi.check(lib.gpk_frechet_distance(a.handle, a.handle, r, k, C.c_void_p(f.data_ptr()), None, _abi.MEM_DEVICE, s))

    # the checks come first: no time is printed for an output that breaks them
    distance()
    hausdorff()
    if with_frechet:
        frechet()
    torch.cuda.synchronize()
    ok = ~torch.isnan(h)
    assert bool((torch.isnan(d) == torch.isnan(h)).all()), "hausdorff and distance disagree on the NaN rows"
    assert bool((h[ok] >= d[ok]).all()), f"hausdorff < distance on {int((h[ok] < d[ok]).sum())} rows"
    res = {"workload": label, "rows": n, "subdivisions": k, "hausdorff_ge_distance": True, "nan_rows": int((~ok).sum())}
    if with_frechet:
        both = ok & ~torch.isnan(f)
        assert bool((torch.isnan(f) == torch.isnan(h)).all()), "frechet and hausdorff disagree on the NaN rows (no row of this column is above the cap)"
        assert bool((f[both] >= h[both]).all()), f"frechet < hausdorff on {int((f[both] < h[both]).sum())} rows"
        res["frechet_ge_hausdorff"] = True

    coords, seqs = _row_counts(a_h)
    samples = (coords - seqs) * k + seqs
    terms = samples * coords[rows_h] + samples[rows_h] * coords
    res["point_segment_terms"] = int(terms.sum())
    res["hausdorff_listed_rows"] = int((terms > HD_LARGE_COST).sum())
    res["distance_rowwise"] = timed(distance, steps, warmup)
    res["hausdorff"] = timed(hausdorff, steps, warmup)
    res["hausdorff_over_distance"] = res["hausdorff"]["ms_median"] / res["distance_rowwise"]["ms_median"]
    if with_frechet:
        fs = np.where(coords > 0, (coords - 1) * k + 1, 0)
        cells = fs * fs[rows_h]
        assert int(np.minimum(fs, fs[rows_h]).max()) <= FRECHET_MAX_SHORT
        res["frechet_cells"] = int(cells.sum())
        res["frechet_listed_rows"] = int((cells > FR_LARGE_COST).sum())
        res["frechet"] = timed(frechet, steps, warmup)
        res["frechet_over_distance"] = res["frechet"]["ms_median"] / res["distance_rowwise"]["ms_median"]
    name_dev, cus = _abi.device_info()
    res["device"] = name_dev
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--rows", type=int, default=0, help="rows per column (default: the workload's own size)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    for name in ([args.only] if args.only else list(WORKLOADS)):
        run(name, args.steps, args.warmup, args.rows)


if __name__ == "__main__":
    main()
