#!/usr/bin/env python3
"""k-nearest-neighbours join (gpk_knn_join) timings on device-resident data (a secondary measurement: bench.py is unchanged).

    python tools/bench_knn.py [--steps 5] [--warmup 2] [--only c2|self] [--k 1 --k 8 ...] > profiles/knn_bench.jsonl

Workloads, each at k = 1, 8 and 32: 10M synth.uniform_points x 1000 synth.star_polygons (the C2 data), and 1M uniform points against
themselves with GPK_KNN_EXCLUDE_SELF.  The right side's index (GPK_INDEX_BBOX_GRID) is built once beforehand; each step is one whole
synchronous call into device buffers of n_left * k pairs, timed with HIP events on the stream.  One untimed call with the join
statistics on gives the candidates listed; one with the library's profiler on gives ms per stage.  Beside every time stands
gpk_nearest_join_any on the same buffers in the same process: the call the parent commit has, and the number to hold k = 1 against.

Before a time is printed the result is checked:
  * at k = 1 (without the self exclusion) the pairs are, per left row, the lowest-r pair of gpk_nearest_join_any with the same distance
    bits;
  * on 1000 sampled left rows, at every k, the result equals a stable sort of gpk_distance_rowwise against every right row.
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
from geopolars_amd.spatial_index import SpatialIndex, knn_pairs_device, nearest_pairs_any_device  # noqa: E402

STAGES = ["gpk_bounds", "gpk_knn_walk", "gpk_bbox_cand_count", "gpk_cand_compact", "gpk_bbox_cand_fill", "gpk_knn_refine", "gpk_knn_refine_large",
          "gpk_knn_span", "gpk_knn_select_wave", "gpk_knn_select_list", "gpk_pair_count", "gpk_pair_emit", "gpk_knn_emit"]
SAMPLE = 1000
KS = (1, 8, 32)


def _c2():
    return synth.uniform_points(10_000_000), synth.star_polygons(1000, 64), False


def _self():
    pts = synth.uniform_points(1_000_000)
    return pts, pts, True


WORKLOADS = {
    "c2": ("10M points x 1000 star polygons (C2 data)", _c2),
    "self": ("1M x 1M uniform points against themselves, GPK_KNN_EXCLUDE_SELF", _self),
}


def _upload(a, stream):
    if a.geom_type == _abi.GEOM_POINT:
        return DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, torch.from_numpy(a.xy).to("cuda:0"), stream=stream)
    return DeviceGeoArray.upload(a, stream=stream)


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
    return out


def _ms(times):
    return {"ms_per_call_median": round(float(np.median(times)), 4), "ms_per_call_min": round(float(np.min(times)), 4)}


def _bits(t):
    return t.contiguous().view(torch.int64)


def sample_reference(lib, left_h, right, n_right, sample, top, exclude_self, stream):
    """per sampled left row the first `top` of a stable sort of (gpk_distance_rowwise, r) over every right row: (right rows, distances)"""
    per = max(1, min(len(sample), (1 << 25) // n_right))  # left rows per row-wise call
    rows = torch.arange(n_right, dtype=torch.int32, device="cuda:0").repeat(per)
    r_top, d_top = [], []
    for at in range(0, len(sample), per):
        chunk = sample[at:at + per]
        m = len(chunk)
        xy = torch.from_numpy(np.repeat(left_h.xy[chunk], n_right, axis=0)).to("cuda:0")
        rep = DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, xy, stream=stream)
        out = torch.empty(m * n_right, dtype=torch.float64, device="cuda:0")
        _abi.check(lib.gpk_distance_rowwise(rep.handle, right.handle, C.c_void_p(rows.data_ptr()), C.c_void_p(out.data_ptr()), _abi.MEM_DEVICE,
                                            C.c_void_p(stream)))
        torch.cuda.synchronize()
        D = out.view(m, n_right) + 0.0
        assert not bool(torch.isnan(D).any()), "the synthetic columns hold no unusable row"
        if exclude_self:
            D[torch.arange(m, device="cuda:0"), torch.from_numpy(chunk).to("cuda:0")] = float("inf")
        d_sorted, r_sorted = torch.sort(D, dim=1, stable=True)  # (stable: ties go to the lower right row)
        r_top.append(r_sorted[:, :top].clone())
        d_top.append(d_sorted[:, :top].clone())
        del rep, xy, out, D, d_sorted, r_sorted
    return torch.cat(r_top), torch.cat(d_top)


def check_sample(sample, reference, usable_right, k, counts, pairs, dist):
    """the sampled rows' pairs and distances == the first k of their reference"""
    r_top, d_top = reference
    c = counts.long()
    first = torch.cumsum(c, 0) - c
    for j, l in enumerate(sample.tolist()):
        o, cnt = int(first[l]), int(c[l])
        assert cnt == min(k, usable_right), (l, cnt)
        assert torch.equal(pairs[o:o + cnt, 1].long(), r_top[j, :cnt]), f"row {l}: the right rows differ from the sorted matrix row"
        assert bool((pairs[o:o + cnt, 0] == l).all())
        assert torch.equal(_bits(dist[o:o + cnt]), _bits(d_top[j, :cnt])), f"row {l}: a distance is not gpk_distance_rowwise's double"


def run(name, ks, steps, warmup):
    lib = _abi.lib()
    label, make = WORKLOADS[name]
    left_h, right_h, exclude_self = make()
    stream = torch.cuda.current_stream().cuda_stream
    left = _upload(left_h, stream)
    right = left if right_h is left_h else _upload(right_h, stream)
    torch.cuda.synchronize()
    idx = SpatialIndex.from_device(right, stream=stream, for_points=False)
    n, n_right = len(left_h), len(right_h)
    sample = np.sort(np.random.default_rng(0).choice(n, min(SAMPLE, n), replace=False))

    # gpk_nearest_join_any on the same buffers: the k = 1 check, and the time that stands beside every k
    nc = torch.empty(n, dtype=torch.int32, device="cuda:0")
    hn = nearest_pairs_any_device(left, right, idx, nc, None, stream=stream)
    npairs, nd = torch.empty((max(hn, 1), 2), dtype=torch.int32, device="cuda:0"), torch.empty(max(hn, 1), dtype=torch.float64, device="cuda:0")
    nearest_call = lambda: nearest_pairs_any_device(left, right, idx, nc, npairs, nd, stream=stream)  # noqa: E731
    assert nearest_call() == hn
    torch.cuda.synchronize()
    c1 = torch.empty(n, dtype=torch.int32, device="cuda:0")
    p1, d1 = torch.empty((n, 2), dtype=torch.int32, device="cuda:0"), torch.empty(n, dtype=torch.float64, device="cuda:0")
    h1 = knn_pairs_device(left, right, idx, 1, c1, p1, d1, stream=stream)
    torch.cuda.synchronize()
    ncl = nc.long()
    firsts = (torch.cumsum(ncl, 0) - ncl)[ncl > 0]
    assert h1 == len(firsts) and torch.equal(c1, torch.clamp(nc, max=1)), "k = 1: not one pair per row that has a nearest row"
    assert torch.equal(p1[:h1], npairs[firsts]) and torch.equal(_bits(d1[:h1]), _bits(nd[firsts])), "k = 1: not the nearest join's lowest-r pair"
    nearest_ms = _ms(timed(nearest_call, steps, warmup))
    del p1, d1, c1

    reference = sample_reference(lib, left_h, right, n_right, sample, min(max(ks), n_right), exclude_self, stream)
    results = []
    for k in ks:
        counts = torch.empty(n, dtype=torch.int32, device="cuda:0")
        pairs = torch.empty((n * k, 2), dtype=torch.int32, device="cuda:0")
        dist = torch.empty(n * k, dtype=torch.float64, device="cuda:0")
        call = lambda: knn_pairs_device(left, right, idx, k, counts, pairs, dist, exclude_self=exclude_self, stream=stream)  # noqa: E731
        h = call()
        torch.cuda.synchronize()
        check_sample(sample, reference, n_right - (1 if exclude_self else 0), k, counts, pairs, dist)
        times = timed(call, steps, warmup)
        st = (C.c_int64 * 4)()
        lib.gpk_join_stats_enable(1)
        lib.gpk_join_stats(st, 1)
        call()
        lib.gpk_join_stats(st, 1)
        lib.gpk_join_stats_enable(0)
        cand, rejected = int(st[2]), int(st[3])
        lib.gpk_profile_reset()
        lib.gpk_profile_filter(b"")
        lib.gpk_profile_enable(1)
        call()
        lib.gpk_profile_enable(0)
        torch.cuda.synchronize()
        stage_ms = {}
        for s in STAGES:
            ms, cnt = C.c_double(0), C.c_int64(0)
            lib.gpk_profile_query(s.encode(), C.byref(ms), C.byref(cnt))
            if cnt.value:
                stage_ms[s] = round(ms.value, 4)
        lib.gpk_profile_reset()
        results.append({"workload": name, "what": label, "k": k, "exclude_self": exclude_self, "n_left": n, "n_right": n_right, "pairs": int(h),
                        **_ms(times), "nearest_join_any_same_buffers": nearest_ms, "candidates": cand, "box_rejected": rejected,
                        "candidates_per_pair_returned": round(cand / max(h, 1), 3), "stage_ms": stage_ms, "sample_checked": int(len(sample)),
                        "steps": steps, "warmup": warmup})
        del counts, pairs, dist
    idx.free()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=sorted(WORKLOADS), action="append")
    ap.add_argument("--k", type=int, action="append")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    name, cus = _abi.device_info()
    for w in a.only or list(WORKLOADS):
        for r in run(w, tuple(a.k or KS), a.steps, a.warmup):
            r["device"] = f"{name} ({cus} CUs)"
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
