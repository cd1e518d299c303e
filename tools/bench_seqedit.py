#!/usr/bin/env python3
"""segmentize / remove_repeated_points / reverse / orient_polygons on device-resident columns (a secondary measurement: bench.py is
unchanged).

    python tools/bench_seqedit.py [--steps 5] [--warmup 2] [--only points|poly8|poly64|c4|powerlaw] >> profiles/seqedit_bench.jsonl

The five columns of tools/bench_take.py.  The floor of every operation is gpk_geoarray_take with the identity index (device-resident)
on the same column in the same process: the calls are timed alternately, one round of all of them per step, medians of --steps after
--warmup.  Before anything is timed every operation's result is asserted against tests/seqedit_ref.py on sampled rows (the operations
work sequence by sequence, so the rows of the result are the results of the rows): bit for bit, every level.  segmentize runs twice:
with a bound nothing exceeds (the passes alone) and with a bound that splits the median segment in four (the figure there is output
bytes per second, beside take's).  Times: HIP events around the whole call, its one wait and the result's allocation and release
included; per kernel through gpk_profile_query."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geopolars_amd import _abi  # noqa: E402
from geopolars_amd.geoarrow import DeviceGeoArray  # noqa: E402
from tests import seqedit_ref as R  # noqa: E402
from tools.bench_take import WORKLOADS, assert_same  # noqa: E402

STAGES = ["gpk_seqedit_heads", "gpk_seqedit_rowstart", "gpk_seqedit_count", "gpk_scan_totals", "gpk_seqedit_place", "gpk_seqedit_offsets",
          "gpk_seqedit_strips", "gpk_seqedit_segfill", "gpk_seqedit_shells", "gpk_seqedit_argmin", "gpk_seqedit_argmin_long", "gpk_seqedit_revfill",
          "gpk_geotake_count", "gpk_geotake_totals", "gpk_geotake_rows", "gpk_geotake_strips", "gpk_geotake_offsets", "gpk_geotake_coords",
          "gpk_scan_partial", "gpk_scan_final"]
SAMPLE = 300


def stage_ms(lib, call):
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
    host = make()
    stream = torch.cuda.current_stream().cuda_stream
    dev = DeviceGeoArray.upload(host, stream=stream)
    torch.cuda.synchronize()
    n = len(host)
    rng = np.random.default_rng(1)
    identity = torch.arange(n, dtype=torch.int64, device="cuda:0")
    seglen = np.hypot(*np.diff(host.xy[: 1 << 20], axis=0).T)
    m_split = float(np.median(seglen[seglen > 0])) / 4 if host.geom_type in R.EDITED else 1.0
    m_none = 1e300
    ops = {
        "take_identity": (lambda: dev.take(identity, stream=stream), lambda a: a),
        "reverse": (lambda: dev.reverse(stream=stream), R.reverse),
        "orient_polygons": (lambda: dev.orient_polygons(stream=stream), R.orient_polygons),
        "remove_repeated_points": (lambda: dev.remove_repeated_points(stream=stream), R.remove_repeated_points),
        "segmentize_none": (lambda: dev.segmentize(m_none, stream=stream), lambda a: R.segmentize(a, m_none)),
        "segmentize_split": (lambda: dev.segmentize(m_split, stream=stream), lambda a: R.segmentize(a, m_split)),
    }
    sample = np.sort(rng.choice(n, size=min(SAMPLE, n), replace=False)).astype(np.int64)
    want_rows = host.take(sample)
    out = {"workload": name, "what": label, "n_rows": n, "n_coords": host.n_coords, "column_bytes": host.nbytes(), "steps": steps, "warmup": warmup,
           "m_split": m_split, "checked": f"{len(sample)} sampled rows of every operation, bit for bit", "ops": {}}
    for op, (call, ref) in ops.items():
        got = call()
        assert_same(got.take(sample).download(), ref(want_rows), (name, op))
        out["ops"][op] = {"n_coords_out": got.n_coords, "bytes_out": got.nbytes()}
        got.free()
    times = {op: [] for op in ops}
    for step in range(warmup + steps):
        for op, (call, _) in ops.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call().free()
            b.record()
            torch.cuda.synchronize()
            if step >= warmup:
                times[op].append(a.elapsed_time(b))
    floor = float(np.median(times["take_identity"]))
    for op, (call, _) in ops.items():
        r = out["ops"][op]
        r["call_ms"] = round(float(np.median(times[op])), 4)
        r["over_take"] = round(r["call_ms"] / floor, 3)
        r["out_gb_s"] = round(r["bytes_out"] / r["call_ms"] / 1e6, 1)
        r["stage_ms"] = stage_ms(lib, lambda: call().free())
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
