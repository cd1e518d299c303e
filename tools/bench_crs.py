"""Analytic reprojection (gpk_reproject) at 10M device-resident points, beside the HBM-bound floor of the same traffic.

    python tools/bench_crs.py [--n 10000000] [--reps 30] [--out profiles/crs_bench.jsonl]

Per instance (4326->3857, 4326->3395, 4326->UTM, UTM->4326, UTM->neighbouring UTM): device time per call (HIP events around `reps`
calls, n_failed = NULL so nothing is read back), coordinates/s, and the ratio to gpk_affine_transform on the same column in the same
process — 16 B in and 16 B out per coordinate, the floor for this traffic.  Also the numpy restatement of the series (tests/crs_ref.py)
on the host, and the worst error of the GPU against the mp fixture per fixture case.  One JSON object per line.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geopolars_amd import _abi  # noqa: E402
from geopolars_amd.geoarrow import DeviceGeoArray  # noqa: E402
from tests import crs_ref as R  # noqa: E402

INSTANCES = [(4326, 3857), (4326, 3395), (4326, 32633), (32633, 4326), (32633, 32634)]


def gpu_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cpu-n", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crs_bench.jsonl"))
    a = ap.parse_args()
    lib = _abi.lib()
    name, cus = _abi.device_info()
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(5)
    # lon/lat inside zone 33's pinned domain (15 +- 12 degrees) and the Mercators' latitudes
    geo = np.stack([rng.uniform(3.0, 27.0, a.n), rng.uniform(-80.0, 84.0, a.n)], axis=1)
    lines = []

    def emit(**kw):
        kw.update(device=name, cus=cus)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    sources = {4326: torch.from_numpy(geo).cuda()}
    out = torch.empty_like(sources[4326])
    dev = {4326: DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, sources[4326])}
    # the UTM source column is made on the device
    utm = torch.empty_like(out)
    _abi.check(lib.gpk_reproject(dev[4326].handle, 4326, 32633, utm.data_ptr(), None, _abi.MEM_DEVICE, stream))
    torch.cuda.synchronize()
    sources[32633] = utm
    dev[32633] = DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, utm)
    m6 = (C.c_double * 6)(1.0, 0.0, 10.0, 0.0, 1.0, 10.0)
    for s, d in INSTANCES:
        h = dev[s].handle
        nf = C.c_int64(-1)
        _abi.check(lib.gpk_reproject(h, s, d, out.data_ptr(), C.byref(nf), _abi.MEM_DEVICE, stream))
        # alternate floor / instance / floor so that both see the same clocks
        floor1 = gpu_ms(lambda: _abi.check(lib.gpk_affine_transform(h, m6, out.data_ptr(), _abi.MEM_DEVICE, stream)), a.reps)
        ms = gpu_ms(lambda: _abi.check(lib.gpk_reproject(h, s, d, out.data_ptr(), None, _abi.MEM_DEVICE, stream)), a.reps)
        floor2 = gpu_ms(lambda: _abi.check(lib.gpk_affine_transform(h, m6, out.data_ptr(), _abi.MEM_DEVICE, stream)), a.reps)
        floor = 0.5 * (floor1 + floor2)
        k = min(a.cpu_n, a.n)
        src_host = sources[s][:k].cpu().numpy()
        t0 = time.perf_counter()
        R.np_transform(s, d, src_host)
        cpu_s = time.perf_counter() - t0
        emit(bench="reproject", instance=f"{s}->{d}", n=a.n, n_failed=int(nf.value), ms_per_call=ms, coords_per_s=a.n / (ms * 1e-3), GBps=32 * a.n / (ms * 1e-3) / 1e9,
             affine_ms_per_call=floor, affine_ms_before_after=[floor1, floor2], affine_GBps=32 * a.n / (floor * 1e-3) / 1e9, ratio_to_affine_floor=ms / floor,
             numpy_coords_per_s=k / cpu_s, numpy_n=k, timing="HIP events around reps calls, device-resident in and out, n_failed=NULL", reps=a.reps)
    # accuracy of the device against the mp fixture
    fx = np.load(os.path.join(ROOT, "tests", "golden", "crs_reference.npz"))
    np_worst = dict(zip(fx["np_worst_names"].tolist(), fx["np_worst_m"].tolist()))
    for cname, s, d, src, want in R.fixture_cases(fx):
        x = torch.from_numpy(src).cuda()
        o = torch.empty_like(x)
        col = DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, x)  # lives until the launch has finished
        _abi.check(lib.gpk_reproject(col.handle, s, d, o.data_ptr(), None, _abi.MEM_DEVICE, stream))
        torch.cuda.synchronize()
        emit(bench="reproject_accuracy", case=cname, rows=len(src), gpu_worst_m=float(R.error_metres(d, o.cpu().numpy(), want).max()), numpy_worst_m=np_worst[cname], tolerance_m=R.TOL_M)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
