"""Geodesic area / perimeter / inverse / direct (gpk_geodesic.hip) on (lon, lat) columns, beside gpk_geodesic_length(GPK_GEODESIC_KARNEY) on
the same column in the same process: the same inverse per exterior edge, on the per-row lane-group schedule.

    python tools/bench_geodesic.py [--scale 1.0] [--steps 5] [--warmup 2] [--out profiles/geodesic_bench.jsonl]

Columns: 1M clustered polygons (domain 60), 2M 64-vertex stars, 1M power-law multipolygons (domain 80), 10M point pairs.  Before it
times, the tool asserts per polygon column that the perimeter is the geodesic length where a row has no hole (and at least it elsewhere),
and 300 sampled rows (and 300 sampled pairs) against csrc/gpk_geodesic.h run on the host by tests/geodesic_host_driver.cpp, within the
GPU rules of tests/geodesic_measure_ref.py.  Then 5 steps after 2, device-resident in and out, HIP events around every step: medians.
One JSON object per line."""
import argparse
import json
import os
import pathlib
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geopolars_amd import _abi, synth  # noqa: E402
from geopolars_amd.geoarrow import DeviceGeoArray  # noqa: E402
from tests import geodesic_measure_ref as R  # noqa: E402
from tests.test_geodesic_host import _compilers, run_driver  # noqa: E402


def median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms


def host_driver(workdir):
    exe = str(workdir / "geodesic_driver")
    for cxx in _compilers():
        r = subprocess.run([cxx, "-std=c++17", "-ffp-contract=off", "-O2", f"-I{ROOT}/geopolars_amd/csrc", f"{ROOT}/tests/geodesic_host_driver.cpp", "-o", exe],
                           capture_output=True, text=True)
        if r.returncode == 0:
            return exe
    raise RuntimeError("no host compiler built tests/geodesic_host_driver.cpp")


def empty_job():
    z = np.zeros
    return {"edge_xy": z((0, 4)), "edge_s12": z(0), "edge_azi1": z(0), "edge_azi2": z(0), "edge_m12": z(0, dtype=np.float32), "edge_S12": z(0),
            "edge_regime": z(0, dtype=np.int32), "direct_in": z((0, 4)), "direct_out": z((0, 3)), "ring_off": z(1, dtype=np.int32),
            "ring_regime": z(0, dtype=np.int32), "ring_xy": z((0, 2)), "ring_area": z(0), "ring_perimeter": z(0)}


def row_rings(col, g):
    if col.part_offsets is None:
        return [list(range(col.geom_offsets[g], col.geom_offsets[g + 1]))]
    return [list(range(col.part_offsets[p], col.part_offsets[p + 1])) for p in range(col.geom_offsets[g], col.geom_offsets[g + 1])]


def host_rows(exe, workdir, col, sample):
    """(signed, unsigned, perimeter, edges) of the sampled rows by the header on the host"""
    job, xy, off, owner = empty_job(), [], [0], []
    for k, g in enumerate(sample):
        for part in row_rings(col, g):
            for j, r in enumerate(part):
                c = col.xy[col.ring_offsets[r]:col.ring_offsets[r + 1]]
                xy.append(c)
                off.append(off[-1] + len(c))
                owner.append((k, j == 0))
    n = len(owner)
    job.update(ring_xy=np.concatenate(xy), ring_off=np.array(off, dtype=np.int32), ring_regime=np.zeros(n, dtype=np.int32), ring_area=np.zeros(n),
               ring_perimeter=np.zeros(n))
    _, _, rings, _ = run_driver(exe, workdir, job)
    out = np.zeros((4, len(sample)))
    for (k, shell), (area, per), ne in zip(owner, rings, np.diff(off) - 1):
        out[0, k] += area
        out[1, k] += abs(area) if shell else -abs(area)
        out[2, k] += per
        out[3, k] += max(ne, 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geodesic_bench.jsonl"))
    a = ap.parse_args()
    lib = _abi.lib()
    name, cus = _abi.device_info()
    stream = torch.cuda.current_stream().cuda_stream
    workdir = pathlib.Path(tempfile.mkdtemp(prefix="geodesic_bench_"))
    exe = host_driver(workdir)
    lines = []
    per_edge = max(R.RING_AREA_ERR_M2_PER_EDGE.values())

    def emit(**kw):
        kw.update(device=name, cus=cus, steps=a.steps, warmup=a.warmup, timing="HIP events around every step, device-resident in and out: medians")
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    n = lambda k: max(1000, int(k * a.scale))  # noqa: E731
    columns = [("clustered_polygons_1M", lambda: synth.clustered_polygons(n(1_000_000), domain=60.0)),
               ("stars_2M_x64", lambda: synth.star_polygons(n(2_000_000), 64, domain=60.0)),
               ("powerlaw_multipolygons_1M", lambda: synth.powerlaw_multipolygons(n(1_000_000), domain=80.0))]
    for cname, make in columns:
        col = make()
        dev = DeviceGeoArray.upload(col, stream=stream)
        rows = len(col)
        area, per, length = (torch.empty(rows, dtype=torch.float64, device="cuda") for _ in range(3))
        call_area = lambda flags, pa, pp: _abi.check(lib.gpk_geodesic_area(dev.handle, flags, pa, pp, _abi.MEM_DEVICE, stream))  # noqa: E731
        call_len = lambda: _abi.check(lib.gpk_geodesic_length(dev.handle, 0, length.data_ptr(), _abi.MEM_DEVICE, stream))  # noqa: E731
        signed = torch.empty_like(area)
        call_area(_abi.GEODESIC_AREA_SIGNED, signed.data_ptr(), per.data_ptr())
        call_area(0, area.data_ptr(), None)
        call_len()
        torch.cuda.synchronize()
        h_signed, h_area, h_per, h_len = (t.cpu().numpy() for t in (signed, area, per, length))
        # the identity: a row's perimeter is its geodesic length when it has no hole, and at least that otherwise
        rings_per_row = np.diff(col.geom_offsets) if col.part_offsets is None else np.add.reduceat(np.diff(col.part_offsets), col.geom_offsets[:-1])
        parts_per_row = np.ones(rows, dtype=np.int64) if col.part_offsets is None else np.diff(col.geom_offsets)
        hole_free = rings_per_row == parts_per_row
        edges = np.add.reduceat(np.diff(col.ring_offsets) - 1, (col.geom_offsets if col.part_offsets is None else col.part_offsets[col.geom_offsets])[:-1])
        tol = 1e-9 * h_len + 2e-8 * edges
        assert np.all(np.abs(h_per - h_len)[hole_free] <= tol[hole_free]) and np.all(h_per >= h_len - tol), cname
        sample = np.sort(np.random.default_rng(1).choice(rows, min(300, rows), replace=False))
        want = host_rows(exe, workdir, col, sample)
        bound = R.GPU_FACTOR * (per_edge * want[3] + R.RING_AREA_REL * np.abs(want[0]))
        assert np.all(np.abs(h_signed[sample] - want[0]) <= bound) and np.all(np.abs(h_area[sample] - want[1]) <= bound), cname
        assert np.all(np.abs(h_per[sample] - want[2]) <= 1e-9 * want[2] + 2e-8 * want[3]), cname
        ms_both, _ = median_ms(lambda: call_area(0, area.data_ptr(), per.data_ptr()), a.steps, a.warmup)
        ms_len1, _ = median_ms(call_len, a.steps, a.warmup)
        ms_per, _ = median_ms(lambda: call_area(0, None, per.data_ptr()), a.steps, a.warmup)
        ms_area, _ = median_ms(lambda: call_area(0, area.data_ptr(), None), a.steps, a.warmup)
        ms_len2, _ = median_ms(call_len, a.steps, a.warmup)
        ms_len = 0.5 * (ms_len1 + ms_len2)
        all_edges, ext_edges = int((np.diff(col.ring_offsets) - 1).sum()), int(round(float(edges.sum() if hole_free.all() else 0)))
        emit(bench="geodesic_area", column=cname, rows=rows, coords=int(col.n_coords), edges=all_edges, hole_free_rows=int(hole_free.sum()),
             area_and_perimeter_ms=ms_both, area_ms=ms_area, perimeter_ms=ms_per, geodesic_length_karney_ms=ms_len, geodesic_length_before_after_ms=[ms_len1, ms_len2],
             edges_per_s_area_and_perimeter=all_edges / (ms_both * 1e-3), perimeter_over_length=ms_per / ms_len, area_and_perimeter_over_length=ms_both / ms_len,
             exterior_edges_if_hole_free=ext_edges, sampled_rows_checked=len(sample))
        del dev, area, per, length, signed
    # ---- point pairs
    m = n(10_000_000)
    rng = np.random.default_rng(8)
    pa = np.stack([rng.uniform(-180, 180, m), rng.uniform(-89, 89, m)], axis=1)
    pb = np.stack([rng.uniform(-180, 180, m), rng.uniform(-89, 89, m)], axis=1)
    ta, tb = torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda()
    da, db = DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, ta), DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, tb)
    s12, z1, z2 = (torch.empty(m, dtype=torch.float64, device="cuda") for _ in range(3))
    dest = torch.empty((m, 2), dtype=torch.float64, device="cuda")
    inv = lambda p1, p2, p3: _abi.check(lib.gpk_geodesic_inverse(da.handle, db.handle, None, p1, p2, p3, _abi.MEM_DEVICE, stream))  # noqa: E731
    direct = lambda: _abi.check(lib.gpk_geodesic_direct(da.handle, z1.data_ptr(), m, s12.data_ptr(), m, dest.data_ptr(), None, _abi.MEM_DEVICE, stream))  # noqa: E731
    inv(s12.data_ptr(), z1.data_ptr(), z2.data_ptr())
    direct()
    torch.cuda.synchronize()
    sample = np.sort(np.random.default_rng(2).choice(m, 300, replace=False))
    job = empty_job()
    k = len(sample)
    job.update(edge_xy=np.concatenate([pa[sample], pb[sample]], axis=1), edge_s12=np.zeros(k), edge_azi1=np.zeros(k), edge_azi2=np.zeros(k),
               edge_m12=np.zeros(k, dtype=np.float32), edge_S12=np.zeros(k), edge_regime=np.zeros(k, dtype=np.int32))
    want, _, _, _ = run_driver(exe, workdir, job)
    got = np.stack([t[torch.from_numpy(sample).cuda()].cpu().numpy() for t in (s12, z1, z2)], axis=1)
    assert np.all(np.abs(got[:, 0] - want[:, 0]) <= R.karney_bound_m(want[:, 0]))
    azi_m = np.abs(R.wrap180(got[:, 1:] - want[:, 1:3])) * (np.pi / 180) * np.abs(want[:, 3:4])
    assert azi_m.max() <= R.GPU_FACTOR * R.AZIMUTH_ERR_M["whole"], azi_m.max()
    back = dest[torch.from_numpy(sample).cuda()].cpu().numpy()  # direct(a, azi1, s12) lands on b
    miss = R.small_distance_m(back[:, 0], back[:, 1], pb[sample, 0], pb[sample, 1])
    assert np.all(miss <= R.GPU_FACTOR * (R.DIRECT_ERR_M + R.AZIMUTH_ERR_M["whole"]) + R.karney_bound_m(want[:, 0])), miss.max()
    ms_s, _ = median_ms(lambda: inv(s12.data_ptr(), None, None), a.steps, a.warmup)
    ms_all, _ = median_ms(lambda: inv(s12.data_ptr(), z1.data_ptr(), z2.data_ptr()), a.steps, a.warmup)
    ms_dir, _ = median_ms(direct, a.steps, a.warmup)
    # the yardstick on the same pairs: two-point linestrings through gpk_geodesic_length
    lxy = torch.stack([ta, tb], dim=1).reshape(-1, 2).contiguous()
    loff = torch.arange(0, 2 * m + 1, 2, dtype=torch.int32, device="cuda")
    dl = DeviceGeoArray.from_device_buffers(_abi.GEOM_LINESTRING, lxy, geom_offsets=loff)
    length = torch.empty(m, dtype=torch.float64, device="cuda")
    call_len = lambda: _abi.check(lib.gpk_geodesic_length(dl.handle, 0, length.data_ptr(), _abi.MEM_DEVICE, stream))  # noqa: E731
    call_len()
    torch.cuda.synchronize()
    assert torch.equal(length, s12)  # the same inverse: the same bits
    ms_len, _ = median_ms(call_len, a.steps, a.warmup)
    emit(bench="geodesic_points", pairs=m, distance_ms=ms_s, distance_and_bearings_ms=ms_all, destination_ms=ms_dir, geodesic_length_karney_ms=ms_len,
         pairs_per_s_distance=m / (ms_s * 1e-3), pairs_per_s_destination=m / (ms_dir * 1e-3), distance_over_length=ms_s / ms_len, sampled_pairs_checked=k,
         distance_bits_equal_geodesic_length=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
