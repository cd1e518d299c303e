#!/usr/bin/env python3
"""bench.py — the BASELINE.json configurations of the hot path, one process per GPU.

    python bench.py [--config c2|c3|c4|c5] [--gpus N] [--steps K] [--warmup W]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Default = the headline, `configs[1]` ("C2"): predicate evals/s of the 10M-point x 1k-polygon (64-vertex)
point-in-polygon join.  The other configurations print one line each in the same format:

  c2  10M random points contains() against 1k 64-vertex polygons            gpk_spatial_join_async   STRONG scaling (the 10M-point
                                                                                                     problem is fixed: BASELINE's "1/2/4/8 GPU";
                                                                                                     the weak form rides along in config)
  c3  10M points euclidean distance to 100k linestrings (4-256 segments)    gpk_distance_rowwise     weak scaling
  c4  1M x 1M polygon intersects() spatial join, left side row-sharded      gpk_spatial_join         strong scaling
  c5  6.25M points (one rank's share of 50M) within() 5M power-law          gpk_spatial_join_async   weak scaling
      multipolygons + area() of the rank's share of them                    + gpk_area

A step = one full pass of the operator over one batch that is ALREADY RESIDENT IN HBM (C2 rotates through
`--rotate` distinct input / output sets, > 256 MiB in total, so that no step finds its inputs in the Infinity
Cache).  Rank 0 prints ONE JSON line with `roofline` (dominant kernel, HIP-event timed on the launching
stream).

A plain run does only what the headline figure needs: set up, warm up, time exactly `--steps` steps, write the
last step's outputs when `--dump-outputs DIR` is given, print the line.  `--full` adds everything else, as
extra legs of the same run: at N=1 `cpu_baseline` (the CPU oracle on the host cores over a bounded sample of
the same workload), the secondary measurements each configuration reports in `config` (C2: the PCIe leg, the
weak-scaled form, the default call shape, the exact phase's counters; C3: the shuffled row map and the one-shot
call; C4 / C5: repeated index builds, C5's index variant, full-column area and right-partitioned one-shot), and
parity: the GPU result is compared with the oracle on a RANDOM sample of rows (>= 200k, `--parity-rows`);
a full run that fails parity prints no number.

--dump-outputs DIR writes what the timed path returned in its last timed step (rank 0's share) as DIR/<name>.npy,
float32 where every value is exact in it, float64 otherwise: per-row outputs at a fixed, seeded sample of at
most DUMP_ROWS rows (`sample_rows.npy` names them), the pairs whose left row is in that sample, and the total.
The inputs depend on the arguments only, so two builds can be compared output for output.
"""
from __future__ import annotations

# (Thread placement of the cpu_baseline leg: OMP_PROC_BIND=close / OMP_PLACES=cores was tried to make it repeatable across driver boxes
# and made it five times SLOWER on the GPU box (1.0e11 against 5.8e11 evals/s: the container's CPU set and the places do not line up),
# so the OpenMP runtime is left to place its threads; the line reports the minimum and the median of the runs, the CPU model, the
# logical CPUs and how many of them this process may run on.)
import argparse
import ctypes as C
import glob
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

RANDOM_LINE_PEAK_GBS = 50e9 * 64 / 1e9  # tools/micro/random_lines.hip: independent scattered 64-byte lines at a 3 GB footprint
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (about 6.3 achievable)
F64_VALU_PEAK = 39.3e12  # f64 vector instructions / s: 78.6 TFLOP/s FMA = 39.3 T instructions
C5_CHUNKS = 8  # the C5 right side is the concatenation of 8 fixed chunks of 625k multipolygons (one per rank at 8 GPUs)
DUMP_ROWS = 1 << 19  # --dump-outputs: per-row outputs are written at a fixed sample of this many rows (all of them when there are fewer)
DUMP_SEED = 4245
DUMP_MAX_BYTES = 64 << 20


# ------------------------------------------------------------------------------------------------------
def source_hash() -> str:
    """Content hash of the kernel sources: profiles/*_pmc_traffic.json names the hash it was measured at, and a
    measurement of other sources is not reported as this build's traffic."""
    h = hashlib.sha256()
    for fn in sorted(glob.glob(os.path.join(ROOT, "geopolars_amd", "csrc", "*"))):
        if fn.endswith((".hip", ".h", ".cpp")):
            with open(fn, "rb") as f:
                h.update(os.path.basename(fn).encode())
                h.update(f.read())
    return h.hexdigest()[:16]


def pmc_record(kernel: str):
    """Latest committed PMC traffic record for `kernel` whose source hash matches this tree (else None + reason)."""
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic*.json")), key=os.path.getmtime)
    cur = source_hash()
    stale = None
    for fn in reversed(cands):  # any record measured at THIS tree's hash counts; otherwise name the newest one
        try:
            with open(fn) as f:
                t = json.load(f)
        except Exception:
            continue
        if t.get("kernel") != kernel:
            continue
        if t.get("source_hash") == cur:
            return t, None
        if stale is None:
            stale = f"stale: {os.path.basename(fn)} was measured at source hash {t.get('source_hash')}, this tree is {cur} (re-run tools/profile_headline.sh)"
    return None, stale or "no PMC record for this kernel under profiles/"


def pmc_config_record(config: str):
    """Raw / factor-corrected PMC traffic of a configuration's dominant kernel from the latest committed
    profiles/r*_pmc_traffic_configs.json whose source hash matches this tree (else None + reason)."""
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic_configs.json")), key=os.path.getmtime)
    cur = source_hash()
    stale = None
    for fn in reversed(cands):
        try:
            with open(fn) as f:
                t = json.load(f)
        except Exception:
            continue
        if t.get("source_hash") != cur:
            if stale is None:
                stale = f"stale: {os.path.basename(fn)} was measured at source hash {t.get('source_hash')}, this tree is {cur} (re-run tools/profile_configs.sh)"
            continue
        r = t.get("configs", {}).get(config)
        if r is None:
            return None, f"{os.path.basename(fn)} holds no record for {config}"
        return r, f"raw FETCH_SIZE + WRITE_SIZE of {r['kernel']} per launch; with the 16-byte-stream read factor {t.get('read_factor_of_the_16_byte_stream')}: {r['traffic_bytes_with_read_factor']} B (gathers are tallied at 64 B per request: the truth lies between)"
    return None, stale or "no PMC record for this configuration under profiles/"


def roofline_traffic(roofline: dict, config: str) -> dict:
    r, note = pmc_config_record(config)
    roofline["traffic"] = r["traffic_bytes_raw"] if r else None
    roofline["traffic_note"] = note
    if r and r.get("valu_wave_instructions_per_launch") and roofline.get("launch_ms"):
        # a second roofline for kernels that are not bandwidth-bound: vector instructions issued (SQ_INSTS_VALU, one per wave of 64
        # lanes) against the f64 issue rate — an upper bound on what arithmetic could explain
        lane_rate = r["valu_wave_instructions_per_launch"] * 64.0 / (roofline["launch_ms"] * 1e-3)
        issued = {"wave_instructions_per_launch": r["valu_wave_instructions_per_launch"], "achieved_lane_instr_per_s": lane_rate, "peak": F64_VALU_PEAK,
                  "frac": lane_rate / F64_VALU_PEAK, "salu_wave_instructions_per_launch": r.get("salu_wave_instructions_per_launch")}
        if "valu" not in roofline:
            roofline["valu"] = issued
        else:  # the configuration states its own arithmetic roofline (useful instructions): the issued ones go next to it
            roofline["valu"]["issued"] = issued
    return roofline


class Ctx:
    """torch / torch.distributed plumbing shared by every configuration."""

    def __init__(self, args):
        import torch
        import torch.distributed as dist

        from geopolars_amd import _abi

        self.torch, self.dist, self.args = torch, dist, args
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if self.world != args.gpus:  # (main() launches the ranks itself when there is no launcher: this is a launcher that disagrees)
            if self.rank == 0:
                print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={self.world}: the line reports n_gpus = {self.world}", file=sys.stderr)
        if not torch.cuda.is_available():
            print("bench.py: no GPU visible — libgeopolars_hip has no CPU fallback", file=sys.stderr, flush=True)
            if self.world > 1:
                # (the launcher ends the other ranks when the first one exits: every rank says why before that — each leaves a marker and
                # waits, up to 30 s, until all have)
                d = _marker_dir()
                os.makedirs(d, exist_ok=True)
                open(os.path.join(d, f"nogpu.{self.rank}"), "w").close()
                t0 = time.time()
                while time.time() - t0 < 30.0 and sum(1 for f in os.listdir(d) if f.startswith("nogpu.")) < self.world:
                    time.sleep(0.05)
            sys.exit(3)
        torch.cuda.set_device(self.local_rank)
        self.dev = torch.device("cuda", self.local_rank)
        self.use_dist = self.world > 1 or args.force_dist or (args.spawn and "WORLD_SIZE" in os.environ)
        if self.use_dist:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29511")
            if os.environ.get("NCCL_DEBUG", "").upper() in ("", "VERSION"):
                os.environ["NCCL_DEBUG"] = "WARN"  # no RCCL version banner on stdout: rank 0 prints ONE JSON line
            os.environ.setdefault("NCCL_DEBUG_FILE", "/dev/stderr")  # RCCL's warnings do not belong on stdout either
            dist.init_process_group("nccl", rank=self.rank, world_size=self.world, device_id=self.dev)
        self.lib = _abi.lib()
        self.dev_name, self.cus = _abi.device_info()
        self.stream = torch.cuda.current_stream().cuda_stream

    def barrier(self):
        if self.use_dist:
            self.dist.barrier()
        self.torch.cuda.synchronize()

    def max_over_ranks(self, seconds: float) -> float:
        if not self.use_dist:
            return seconds
        t = self.torch.tensor([seconds], dtype=self.torch.float64, device=self.dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def all_ranks(self, v: float) -> list:
        if not self.use_dist:
            return [v]
        t = self.torch.zeros(self.world, dtype=self.torch.float64, device=self.dev)
        t[self.rank] = v
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return [float(x) for x in t.tolist()]

    def sum_over_ranks(self, v: float) -> float:
        if not self.use_dist:
            return v
        t = self.torch.tensor([v], dtype=self.torch.float64, device=self.dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return float(t.item())

    def kernel_ms(self, name: str):
        ms, cnt = C.c_double(0), C.c_int64(0)
        self.lib.gpk_profile_query(name.encode(), C.byref(ms), C.byref(cnt))
        return (ms.value / max(cnt.value, 1), int(cnt.value))

    def timed(self, step, dominant: str, steps: int, warmup: int, profile: bool = True, one_launch_steps=None):
        """W untimed steps (every kernel bracketed by events after the first: per-kernel durations without taxing the
        timed region), then exactly K steps between barrier + synchronize, only the dominant kernel carrying events.
        -> (seconds max over ranks, dominant-kernel ms per launch, launches, {kernel: ms} from the warm-up)"""
        lib = self.lib
        lib.gpk_profile_reset()
        lib.gpk_profile_filter(b"")
        for w in range(warmup):
            lib.gpk_profile_enable(1 if (profile and w > 0) else 0)
            step(w)
        lib.gpk_profile_enable(0)
        self.torch.cuda.synchronize()
        warm = self._all_kernels(max(warmup - 1, 1))
        lib.gpk_profile_reset()
        # one_launch_steps(warm) -> True: a step is ONE launch of the dominant kernel (the fused point join).  Its duration then comes
        # from one pair of HIP events on the launching stream AROUND the K back-to-back launches, divided by K (launch gaps included:
        # an upper bound of the kernel's own time) — an event pair per launch costs the timed region 5 - 7 us per step, which is
        # nothing next to three kernels and 6 % of one.
        span = bool(profile and one_launch_steps is not None and one_launch_steps(warm))
        lib.gpk_profile_filter(dominant.encode())
        lib.gpk_profile_enable(1 if (profile and not span) else 0)
        ev = (self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)) if span else None
        self.barrier()
        t0 = time.perf_counter()
        if span:
            ev[0].record(self.torch.cuda.current_stream())
        for i in range(steps):
            step(warmup + i)
        if span:
            ev[1].record(self.torch.cuda.current_stream())
        self.barrier()
        t1 = time.perf_counter()
        lib.gpk_profile_enable(0)
        lib.gpk_profile_filter(b"")
        if span:
            k_ms, k_n = ev[0].elapsed_time(ev[1]) / steps, steps
        else:
            k_ms, k_n = self.kernel_ms(dominant)
        self.span_events = span
        lib.gpk_profile_reset()
        self.rank_seconds = self.all_ranks(t1 - t0)  # every rank's own clock around the same K steps (the line carries them)
        return self.max_over_ranks(t1 - t0), k_ms, k_n, warm

    # substring queries: no name here is a substring of another one that can run in the same step
    KERNELS = ("gpk_pip_tile", "gpk_pip_write", "gpk_join_prep", "gpk_distance_grouped", "gpk_dist_hist", "gpk_dist_scatter", "gpk_dist_probe", "gpk_dist_batches", "gpk_dist_iota",
               "gpk_dist_offsets", "gpk_rowmap", "gpk_bbox_cand_count", "gpk_bbox_cand_fill", "gpk_cand_compact", "gpk_pair_refine", "gpk_pair_count", "gpk_pair_emit", "gpk_counts_copy",
               "gpk_ring_area", "gpk_area_combine", "gpk_seq_long", "gpk_scan", "gpk_seq_bbox", "gpk_bounds_combine", "gpk_stats_to_bbox")

    def _all_kernels(self, calls: int) -> dict:
        out = {}
        for name in self.KERNELS:
            ms, cnt = C.c_double(0), C.c_int64(0)
            self.lib.gpk_profile_query(name.encode(), C.byref(ms), C.byref(cnt))
            if cnt.value:
                out[name] = ms.value / calls  # ms per step (a name may cover several launches)
        return out

    def finish(self):
        if self.use_dist:
            self.dist.destroy_process_group()


def open_comm_guarded(ctx: "Ctx", seconds: float):
    """The library's own communicator (gpk_comm_init + one tiny gpk_allgatherv_rows_f64: the first collective is where a broken
    fabric shows) opened with a BOUNDED wait, and an agreement of all ranks over the torch group on whether everybody got it.
    -> (Comm or None, note): None = every rank falls back to geopolars_amd.dist's torch.distributed exchange (the one the gloo
    world-2 tests cover); a rank still stuck inside RCCL's initialisation is left behind on its own thread."""
    import threading

    from geopolars_amd.dist import Comm

    torch = ctx.torch
    box = {}

    def work():
        try:
            c = Comm.from_torch(ctx.dev)
            probe = torch.full((1, 1), float(ctx.rank), dtype=torch.float64, device=ctx.dev)
            got = c.all_gather_rows(probe)
            torch.cuda.synchronize()
            if got.shape[0] != ctx.world or [float(v) for v in got.flatten().tolist()] != [float(r) for r in range(ctx.world)]:
                raise RuntimeError(f"gpk_allgatherv_rows_f64 probe returned {got.flatten().tolist()}")
            box["comm"] = c
        except BaseException as e:  # noqa: BLE001 (reported, and the run goes on without the communicator)
            box["err"] = f"{type(e).__name__}: {e}"

    if os.environ.get("GPK_BENCH_FAIL_COMM"):  # test hook: behave as if the library's communicator never came up
        box["err"] = "GPK_BENCH_FAIL_COMM set"
    else:
        th = threading.Thread(target=work, daemon=True)
        th.start()
        th.join(seconds)
        if th.is_alive():
            box["err"] = f"gpk_comm_init / the first collective did not return within {seconds:.0f} s"
    ok = torch.tensor([1 if "comm" in box else 0], dtype=torch.int32, device=ctx.dev)
    ctx.dist.all_reduce(ok, op=ctx.dist.ReduceOp.MIN)
    if int(ok.item()) == 1:
        return box["comm"], ""
    note = box.get("err", "another rank could not open the library's communicator")
    print(f"bench.py rank {ctx.rank}: C-ABI exchange unavailable ({note}): falling back to torch.distributed", file=sys.stderr)
    return None, note


def _marker_dir() -> str:
    return os.path.join(os.environ.get("TMPDIR", "/tmp"), f"gpk_bench_{os.environ.get('MASTER_PORT', 'single')}_{os.environ.get('TORCHELASTIC_RUN_ID', os.getppid())}")


def error_line(args, message: str) -> dict:
    """what rank 0 prints when the run did not finish: the contract's keys with no value, and why"""
    return {"metric": {"c2": "predicate evals/sec (10M pts x 1k polys point-in-polygon)", "c3": "point-to-linestring distance evaluations/sec",
                       "c4": "polygon x polygon intersects() join pairs/sec", "c5": "within()+area() rows/sec"}.get(args.config, args.config),
            "value": None, "unit": None, "n_gpus": int(os.environ.get("WORLD_SIZE", "1")), "steps": args.steps, "warmup": args.warmup, "ms_per_step": None,
            "higher_is_better": True, "scaling": None, "vs_baseline": None, "dtype": "f64", "data": "synthetic", "config": {"workload": args.config}, "error": message}


def start_watchdog(args, rank: int, seconds: float) -> None:
    """A daemon thread per rank: when the run outlives `seconds`, or ANOTHER rank leaves an error marker (it died: the survivors would wait
    in a collective for ever), rank 0 prints the JSON line with `error` and every rank exits — the caller always gets a line."""
    import threading

    d = _marker_dir()
    os.makedirs(d, exist_ok=True)
    t_end = time.monotonic() + seconds

    def watch():
        while True:
            time.sleep(1.0)
            why = None
            if time.monotonic() > t_end:
                why = f"watchdog: the run did not finish within {seconds:.0f} s"
            else:
                try:
                    for fn in os.listdir(d):
                        if fn.endswith(".err") and fn != f"rank{rank}.err":
                            why = f"{fn[:-4]} failed: " + open(os.path.join(d, fn)).read()[:400]
                            break
                except OSError:
                    pass
            if why:
                if rank == 0:
                    emit_line(error_line(args, why))
                os._exit(4)

    threading.Thread(target=watch, daemon=True).start()


def emit_line(line: dict) -> None:
    """Rank 0's ONE JSON line, on a line of its own: RCCL writes its warnings to the C stdout buffer, which is flushed in
    4 KiB pieces that end mid-line — so the C buffer is flushed first and the JSON starts after a newline."""
    try:
        C.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.write("\n" + json.dumps(line) + "\n")
    sys.stdout.flush()


def dev_array(torch, a, dev, stream):
    """Host GeoArrowArray -> device-resident handle over torch tensors (uploaded once, outside every timed region)."""
    from geopolars_amd.dist import GeoBuffers

    return GeoBuffers.from_host(a, dev).to_device_geoarray(stream)


def sample_rows(n: int, k: int, seed: int) -> np.ndarray:
    k = min(n, k)
    return np.sort(np.random.default_rng(seed).choice(n, size=k, replace=False)).astype(np.int64)


def pairs_of_rows(pairs: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """Rows of a sorted (l, r) pair list whose l is in `rows` (sorted), with l renumbered to the position in `rows`."""
    if len(pairs) == 0:
        return pairs.reshape(0, 2)
    lo = np.searchsorted(pairs[:, 0], rows, side="left")
    hi = np.searchsorted(pairs[:, 0], rows, side="right")
    cnt = hi - lo
    idx = np.repeat(lo - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(int(cnt.sum()))
    out = pairs[idx].copy()
    out[:, 0] = np.repeat(np.arange(len(rows), dtype=pairs.dtype), cnt)
    return out


def dump_arrays(out_dir: str, arrays: dict) -> None:
    """--dump-outputs: each array as out_dir/<name>.npy, float32 when every value survives the cast exactly, float64 otherwise"""
    os.makedirs(out_dir, exist_ok=True)
    conv = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        f32 = a.astype(np.float32)
        exact = np.array_equal(f32.astype(a.dtype), a, equal_nan=a.dtype.kind == "f")
        conv[name] = f32 if exact else a.astype(np.float64)
    total = sum(a.nbytes for a in conv.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit(f"bench.py --dump-outputs: {total} bytes exceed the {DUMP_MAX_BYTES}-byte budget")
    for name, a in conv.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


def dump_join(out_dir: str, counts, pairs, total: int, base: int = 0, per_row: dict | None = None) -> None:
    """--dump-outputs of a join: hit counts (+ other per-row outputs) at the fixed row sample, the (l, r) pairs whose left row
    (global numbering: `base` is the join's left_row_base) is in the sample, and the total number of pairs"""
    idx = sample_rows(int(counts.shape[0]), DUMP_ROWS, seed=DUMP_SEED)
    gc = counts.cpu().numpy()
    h = min(int(total), int(pairs.shape[0]))
    gp = pairs[:h].cpu().numpy().astype(np.int64)
    got = pairs_of_rows(gp - np.array([base, 0]), idx)
    got[:, 0] = idx[got[:, 0]] + base
    arrays = {"sample_rows": idx + base, "counts": gc[idx], "pairs": got, "n_pairs": np.array([total], dtype=np.int64)}
    for name, t in (per_row or {}).items():  # (a per-row output of another column: its own sample, named <name>_rows)
        rows = sample_rows(int(t.shape[0]), DUMP_ROWS, seed=DUMP_SEED)
        arrays[name], arrays[f"{name}_rows"] = t.cpu().numpy()[rows], rows
    dump_arrays(out_dir, arrays)


def base_line(ctx: Ctx, metric: str, value: float, unit: str, ms_per_step: float, scaling: str, config: dict, roofline: dict) -> dict:
    a = ctx.args
    return {
        "metric": metric,
        "value": value,
        "unit": unit,
        "n_gpus": ctx.world,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": scaling,
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": dict(config, device=ctx.dev_name, cus=ctx.cus),
        "roofline": roofline,
        "ranks": {
            "world": ctx.world,
            "backend": ("nccl (RCCL)" if ctx.use_dist else None),
            "ms_per_step_per_rank": [t / a.steps * 1e3 for t in getattr(ctx, "rank_seconds", [])],
        },
    }


# ======================================================================================================
# C2 — the headline
# ======================================================================================================
def run_c2(ctx: Ctx) -> None:
    torch, args, lib = ctx.torch, ctx.args, ctx.lib
    from geopolars_amd import _abi, synth
    from geopolars_amd.dist import broadcast_geoarray
    from geopolars_amd.geoarrow import DeviceGeoArray
    from geopolars_amd.spatial_index import SpatialIndex, join_pairs_device, join_pairs_enqueue

    n, m, dev, stream = args.points, args.polys, ctx.dev, ctx.stream
    polys_host = synth.star_polygons(m, args.verts) if ctx.rank == 0 else None
    if ctx.use_dist:
        polys_host = broadcast_geoarray(polys_host, 0, device=dev)  # RCCL, once, outside the timed region
    polys = DeviceGeoArray.upload(polys_host, stream=stream)
    index = SpatialIndex.from_device(polys, stream=stream)
    # STRONG scaling is the headline (BASELINE.json: "10M pts x 1k polys PIP, 1/2/4/8 GPU" — the 10M-point problem is fixed): rank r owns
    # rows [r n / W, (r + 1) n / W) of the SAME 10M points and emits pairs with left_row_base = its first row; the weak-scaled form
    # (10M points per GPU) is measured in the same run and reported beside it (config.weak_scaling).  At N = 1 they are one measurement.
    W = ctx.world
    lo, hi = (ctx.rank * n) // W, ((ctx.rank + 1) * n) // W
    if args.as_shard:  # test hook: this single process plays shard r of w of the strong-scaled problem (the row split, the pairs' row base and
        r_, w_ = (int(v) for v in args.as_shard.split("/"))  # the parity check of a shard run on a one-GPU box; the line is not a measurement)
        lo, hi = (r_ * n) // w_, ((r_ + 1) * n) // w_
    R = max(1, args.rotate)

    def build_sets(rows_lo: int, rows_hi: int, seed_rank: int, time_h2d: bool):
        """`rotate` distinct input / output sets: each step reads points it has not seen for rotate-1 steps and writes outputs nobody
        has read (3 x (160 + 40 + 80) MB + the library's scratch >> the 256 MiB Infinity Cache)"""
        out, t_h2d = [], None
        k = rows_hi - rows_lo
        for r in range(R):
            pts_all = synth.uniform_points(n, seed=synth.SEED + 1 + seed_rank + 1000 * r)
            pts_host = pts_all if (rows_lo, rows_hi) == (0, n) else pts_all.take(np.arange(rows_lo, rows_hi))
            if time_h2d and r == 0 and ctx.rank == 0:
                pinned = torch.from_numpy(pts_host.xy).pin_memory()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                xy = pinned.to(dev, non_blocking=True)
                torch.cuda.synchronize()
                t_h2d = time.perf_counter() - t0  # the PCIe leg a host-buffer boundary would add per step (never part of `value`)
                del pinned
            else:
                xy = torch.from_numpy(pts_host.xy).to(dev)
            out.append(
                {
                    "host": pts_host,
                    "pts": DeviceGeoArray.from_device_buffers(_abi.GEOM_POINT, xy, stream=stream),
                    "counts": torch.empty(k, dtype=torch.int32, device=dev),
                    "pairs": torch.empty((max(k, 1), 2), dtype=torch.int32, device=dev),  # capacity: one hit per point (disjoint polygons)
                    "total": torch.zeros(1, dtype=torch.int64, device=dev),
                    "base": rows_lo,
                }
            )
        torch.cuda.synchronize()
        return out, t_h2d

    sets, t_h2d = build_sets(lo, hi, 0, args.full)  # (strong: every rank slices the SAME columns — seed independent of the rank)
    sync_steps = args.sync_steps or args.index_per_step
    last = {"set": 0, "h": 0}
    cur = {"sets": sets}

    def step(i: int) -> None:
        """One full pass: this rank's points -> counts + sorted (l, r) pairs + total, all written to HBM.  Default: the
        stream-ordered entry point (steps queue up on the HIP stream; the timed region ends with a synchronise, so
        every step has completed); --sync-steps: the blocking entry point, one host round trip per step."""
        s = cur["sets"][i % R]
        last["set"] = i % R
        if sync_steps:
            idx = SpatialIndex.from_device(polys, stream=stream, light=True) if args.index_per_step else index
            last["h"] = join_pairs_device(s["pts"], polys, idx, "intersects", s["counts"], s["pairs"], left_row_base=s["base"], stream=stream)
            if args.index_per_step:
                idx.free()
        else:
            join_pairs_enqueue(s["pts"], polys, index, "intersects", s["counts"], s["pairs"], s["total"], left_row_base=s["base"], stream=stream)

    # (a step of the fused join is the one launch `gpk_pip_tile`; with GPK_TILE_KERNEL=chain — chain tile kernel + writer — the writer shows up)
    elapsed, k_tile, n_tile, warm = ctx.timed(step, "gpk_pip_tile", args.steps, args.warmup, profile=not args.no_profile,
                                              one_launch_steps=lambda w: "gpk_pip_write" not in w and not sync_steps)
    fused = "gpk_pip_write" not in warm
    rank_seconds_main = list(getattr(ctx, "rank_seconds", []))
    s_last = sets[last["set"]]  # what the last timed step wrote
    h = last["h"] if sync_steps else int(s_last["total"].item())
    if args.dump_outputs and ctx.rank == 0:
        dump_join(args.dump_outputs, s_last["counts"], s_last["pairs"], h, base=s_last["base"])
    weak = None
    if args.full and (W > 1 or args.force_weak) and not args.no_weak:  # the weak-scaled form beside the headline: 10M points PER GPU (rank-dependent seeds)
        del sets
        torch.cuda.empty_cache()
        cur["sets"], _ = build_sets(0, n, ctx.rank + 1, False)
        w_elapsed, w_tile, _, _ = ctx.timed(step, "gpk_pip_tile", args.steps, args.warmup, profile=not args.no_profile,
                                            one_launch_steps=lambda w: "gpk_pip_write" not in w and not sync_steps)
        weak = {"value": float(W) * n * m * args.steps / w_elapsed, "unit": "evals/s", "ms_per_step": w_elapsed / args.steps * 1e3, "points_per_gpu": n,
                "gpk_pip_tile_ms": w_tile, "ms_per_step_per_rank": [t / args.steps * 1e3 for t in getattr(ctx, "rank_seconds", [])]}
        cur["sets"], _ = build_sets(lo, hi, 0, False)
        ctx.rank_seconds = rank_seconds_main
    sets = cur["sets"]
    # the reference's DEFAULT call shape — SpatialJoinArgs::default() has r_index: None (spatial_index.rs:24-35,60-71): the index is
    # built inside every call — measured beside the prepared-index step on the N = 1 line (blocking entry point, index built and freed
    # per step; a second, shorter timed region)
    default_shape = None
    if args.full and W == 1 and not args.index_per_step and not args.no_default_shape:
        def step_default(i: int) -> None:
            s_ = sets[i % R]
            idx = SpatialIndex.from_device(polys, stream=stream, light=True)
            join_pairs_device(s_["pts"], polys, idx, "intersects", s_["counts"], s_["pairs"], left_row_base=0, stream=stream)
            idx.free()
        for i in range(3):
            step_default(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k_def = max(5, args.steps // 2)
        for i in range(k_def):
            step_default(i)
        torch.cuda.synchronize()
        d_ms = (time.perf_counter() - t0) / k_def * 1e3
        # ... and the call itself with right_index = NULL, repeated against the same right-side handle: the library keeps the index it
        # built on the handle (handles are immutable), so every call after the first finds it
        join_pairs_device(sets[0]["pts"], polys, None, "intersects", sets[0]["counts"], sets[0]["pairs"], left_row_base=0, stream=stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(k_def):
            s_ = sets[i % R]
            join_pairs_device(s_["pts"], polys, None, "intersects", s_["counts"], s_["pairs"], left_row_base=0, stream=stream)
        torch.cuda.synchronize()
        m_ms = (time.perf_counter() - t0) / k_def * 1e3
        default_shape = {"ms_per_step": d_ms, "evals_per_s": n * m / (d_ms * 1e-3), "steps": k_def,
                         "what": "gpk_spatial_join with r_index = None's work done per call: index built (GPK_INDEX_PIP_LIGHT), join, index freed; blocking entry point",
                         "repeated_against_the_same_right_handle": {"ms_per_step": m_ms, "evals_per_s": n * m / (m_ms * 1e-3),
                                                                    "what": "gpk_spatial_join(right_index = NULL) called again and again with the same right-side handle: the index built by the first call stays on the handle (blocking entry point: one host round trip per call)"}}
    # what the exact phase did, measured on one extra untimed step (a few atomics per tile: never inside the timed region)
    st = (C.c_int64 * 4)()
    join_stats = args.full and not args.no_join_stats
    if join_stats:
        lib.gpk_join_stats_enable(1)
        lib.gpk_join_stats(st, 1)
        step(args.warmup + args.steps)  # same set the next timed step would have used
        lib.gpk_join_stats(st, 1)
        lib.gpk_join_stats_enable(0)
    torch.cuda.synchronize()
    if args.full:  # (parity checks a blocking call over the set the last step used)
        s_last = sets[last["set"]]
        h = join_pairs_device(s_last["pts"], polys, index, "intersects", s_last["counts"], s_last["pairs"], left_row_base=s_last["base"], stream=stream)
    if ctx.rank != 0:
        ctx.finish()
        return

    n_local = hi - lo
    evals = float(n) * m * args.steps  # the whole job: the fixed 10M-point problem, whatever the number of ranks
    ms_per_step = elapsed / args.steps * 1e3
    v_total = polys_host.n_coords
    # algorithmic bytes (each distinct byte once): points in, polygon coords + offsets in, hit counts out,
    # and the 8H pair bytes — all of it belongs to the ONE launch of the fused join; with the round-3 pair of kernels the pair
    # bytes belong to gpk_pip_write and the dominant launch owns the rest
    bytes_join = 16 * n_local + 16 * v_total + 2 * 4 * (m + 1) + 4 * n_local + 8 * h  # (of THIS rank's launch: rank 0's kernel is the one timed)
    bytes_tile = bytes_join if fused else bytes_join - 8 * h
    achieved = bytes_tile / (k_tile * 1e-3) / 1e9 if k_tile > 0 else 0.0
    traffic, valu_busy, traffic_note = None, None, None
    if n == 10_000_000 and m == 1000 and args.verts == 64:
        rec, traffic_note = pmc_record("gpk_pip_tile")
        if rec is not None:
            traffic, valu_busy = rec.get("traffic_bytes_per_launch"), rec.get("valu_busy")
            traffic_note = rec.get("calibration")
            if rec.get("traffic_bytes_split_estimate"):
                traffic_note += f"; upper bound — with the read factor applied to the point stream only: {rec['traffic_bytes_split_estimate']} B"
    k_write = warm.get("gpk_pip_write", 0.0)
    queued, edges = int(st[0]), int(st[1])
    step_s = ms_per_step * 1e-3
    config = {
        "workload": f"C2: {n} uniform points contains() against {m} {args.verts}-vertex star polygons" + (f", the points row-sharded over {W} GPUs ({n_local} rows on rank 0)" if W > 1 else ""),
        "points_total": n,
        "points_per_gpu": n_local,
        "rows_of_this_rank": [lo, hi],
        "polygons": m,
        "vertices_per_polygon": args.verts,
        "hits_per_step": h,
        "algorithm": "ONE launch per join (pip_tile_flow_kernel, persistent work-groups): two-level exact raster routing (level 1 from an LDS image, level 2 = one 16-byte half-cell record) -> a row with a polygon to be in is a hit at once (4-byte entry in the tile's slots of a global pool, count 1); `test` points wait on the wave's LDS list and are decided in dense passes from the half cell's local chain (base winding + about two ring edges, exact orientation filter; uncertifiable rows go through the generic exact walk), a failed test kills its entry -> work-group totals chained through epoch-tagged words, sorted (l,r) pairs written from the pool 64 entries at a time by the same launch; N x M logical pairs counted, raster-rejected pairs included"
        if fused
        else "chain tile kernel + writer (GPK_TILE_KERNEL=chain)",
        "index_tables": index.describe(),
        "index": "rebuilt per step" if args.index_per_step else "prebuilt r_index (spatial_index.rs:20-21)",
        "call": "gpk_spatial_join (blocking)" if sync_steps else "gpk_spatial_join_async (stream-ordered; the timed region ends synchronised)",
        "parallelism": f"left rows sharded x{ctx.world} (strong scaling: the {n}-point problem is fixed), right side replicated, no data-path collective",
        "weak_scaling": weak,
        "default_call_shape_r_index_none": default_shape,
        "input_rotation": f"{R} distinct 10M-point inputs and output sets ({R * (16 * n + 4 * n + 8 * n) / 2**20:.0f} MiB): inputs come from HBM, not from the 256 MiB Infinity Cache",
        "join_bytes_per_step": bytes_join,
        "join_GBps_end_to_end": bytes_join / step_s / 1e9,
        "kernel_ms": {"gpk_pip_tile": k_tile, "gpk_pip_write (warm-up steps)": k_write, "gpk_join_prep (warm-up steps)": warm.get("gpk_join_prep", 0.0)},
        "exact_phase": {"test_points_per_step": queued, "edge_tests_per_step": edges, "rows_deferred_to_the_generic_walk_per_step": int(st[2])} if join_stats else None,
        "edge_tests_per_s": edges / step_s if join_stats and step_s > 0 else None,
        "valu_busy": valu_busy,
        "pcie_inclusive": None
        if t_h2d is None
        else {"h2d_ms_160MB_pinned": t_h2d * 1e3, "evals_per_s": n * m / (t_h2d + step_s), "note": "what a host-buffer boundary would deliver per GPU: one 160 MB upload per step; never reported as `value`"},
    }
    roofline = {
        "bound": "hbm",
        "kernel": "gpk_pip_tile",
        "achieved": achieved,
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBS,
        "traffic": traffic,
        "traffic_note": traffic_note,
        "launch_ms": k_tile,
        "launches": n_tile,
        "launch_ms_method": "one HIP event pair on the launching stream around the K back-to-back launches / K (a step is one launch; gaps included)"
        if getattr(ctx, "span_events", False)
        else "HIP event pair per launch (gpk_profile_*)",
        "frac_of_achievable": achieved / 6300.0,
        "algorithmic_bytes": bytes_tile,
        "source_hash": source_hash(),
    }
    out = base_line(ctx, "predicate evals/sec (10M pts x 1k polys point-in-polygon)", evals / elapsed, "evals/s", ms_per_step, "strong", config, roofline)
    if args.full:
        out["parity"] = parity_point_join(s_last["host"], polys_host, "intersects", s_last["counts"], s_last["pairs"], h, args.parity_rows, base=s_last["base"])
    if args.full and ctx.world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_join(s_last["host"], polys_host, "intersects", s_last["counts"], args.cpu_seconds)
    ctx.finish()  # (RCCL may print its banner while the group goes down: the JSON line stays the last line of stdout)
    emit_line(out)


def parity_point_join(pts_host, right_host, predicate: str, gpu_counts, gpu_pairs, h: int, rows: int, base: int = 0) -> dict:
    """GPU counts + (l, r) pairs of a RANDOM sample of left rows vs the CPU oracle on exactly those rows: bit-exact or no number.
    `base`: the left_row_base the join ran with (a rank's shard of the left rows: its pairs carry global row numbers)."""
    from oracle import pyoracle

    pyoracle.build()
    n = len(pts_host)
    idx = sample_rows(n, rows, seed=4242)
    ep, ec, _ = pyoracle.spatial_join(pts_host.take(idx), right_host, predicate, mode=1, n_threads=0)
    gc = gpu_counts.cpu().numpy().astype(np.uint32)
    gp = gpu_pairs[:h].cpu().numpy().astype(np.uint32)
    if base:
        gp = gp.copy()
        gp[:, 0] -= np.uint32(base)
    got = pairs_of_rows(gp, idx.astype(np.uint32))
    if not np.array_equal(gc[idx], ec) or not np.array_equal(got, ep) or int(gc.sum()) != h:
        raise SystemExit("bench.py: GPU join differs from the CPU oracle on the parity sample — no speed reported")
    return {"rows": int(len(idx)), "sampling": "uniform random without replacement (seed 4242)", "pairs_checked": int(len(ep)), "bit_exact": True}


def cpu_baseline_join(left_host, right_host, predicate: str, gpu_counts, target_s: float) -> dict:
    """The CPU oracle (oracle/gpk_oracle.c: C restatement of the geo-0.27 path, grid directory + exact refine, OpenMP over
    all host cores) on a bounded prefix of the same left rows; also asserts bit-exact hit counts on that prefix."""
    from oracle import pyoracle

    pyoracle.build()
    n, m = len(left_host), len(right_host)
    probe = min(n, 500_000)
    t0 = time.perf_counter()
    pyoracle.spatial_join(left_host.take(np.arange(probe)), right_host, predicate, mode=1, n_threads=0, capacity=4 * probe)
    dt = max(time.perf_counter() - t0, 1e-3)
    sample = int(min(n, max(probe, probe * target_s / (2.0 * dt))))  # two timed runs of ~target_s/2 each
    sub = left_host.take(np.arange(sample))
    best, runs, spent, threads, counts, times = None, 0, 0.0, 0, None, []
    while runs < 2 or (runs < 9 and spent < target_s / 4):  # the whole job is a fraction of a second on a big host: repeat
        t0 = time.perf_counter()
        _, counts, threads = pyoracle.spatial_join(sub, right_host, predicate, mode=1, n_threads=0, capacity=4 * sample)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        times.append(dt)
        runs += 1
        spent += dt
    got = gpu_counts[:sample].cpu().numpy().astype(np.uint32)
    if not np.array_equal(got, counts):
        raise SystemExit("bench.py: GPU hit counts differ from the CPU oracle on the baseline sample — no speed reported")
    s1 = min(sample, 400_000)
    t0 = time.perf_counter()
    pyoracle.spatial_join(left_host.take(np.arange(s1)), right_host, predicate, mode=1, n_threads=1, capacity=4 * s1)
    t_single = time.perf_counter() - t0
    return {
        "value": sample * m / best,
        "unit": "evals/s",
        "cores": threads,
        "kind": "port",
        "sample": f"first {sample} of the {n} left rows x {m} right rows, min of {runs} runs, grid directory + exact refine, OpenMP dynamic",
        "seconds": best,
        "value_median": sample * m / float(np.median(times)),
        "seconds_median": float(np.median(times)),
        "host": host_description(),
        "parity_checked_rows": sample,
        "single_thread": {"value": s1 * m / t_single, "unit": "evals/s", "sample_rows": s1, "seconds": t_single},
    }


def host_description() -> dict:
    """what the CPU baseline ran on: logical CPUs, the model string, the thread placement asked for"""
    model = ""
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        usable = None
    return {"nproc": os.cpu_count(), "cpus_this_process_may_use": usable, "cpu_model": model, "OMP_PROC_BIND": os.environ.get("OMP_PROC_BIND"), "OMP_PLACES": os.environ.get("OMP_PLACES")}


# ======================================================================================================
# C3 — row-wise distance, 10M points x 100k linestrings
# ======================================================================================================
def run_c3(ctx: Ctx) -> None:
    torch, args, lib = ctx.torch, ctx.args, ctx.lib
    from geopolars_amd import _abi, synth

    n, L, dev, stream = args.points, args.lines, ctx.dev, ctx.stream
    ls_host = synth.random_linestrings(L)
    pts_host = synth.uniform_points(n, seed=synth.SEED + 1 + ctx.rank)
    ls, pts = dev_array(torch, ls_host, dev, stream), dev_array(torch, pts_host, dev, stream)
    rows_mod = (np.arange(n, dtype=np.uint32) % L).astype(np.uint32)  # row-wise semantics: row i pairs with linestring i mod L
    rows_shuf = np.random.default_rng(1).permutation(rows_mod)
    from geopolars_amd.geoseries import RowMap

    out = torch.empty(n, dtype=torch.float64, device=dev)
    results = {}
    legs = (("rows = i mod L", rows_mod), ("rows shuffled", rows_shuf)) if args.full else (("rows = i mod L", rows_mod),)
    for label, rows in legs:
        r_dev = torch.from_numpy(rows.view(np.int32)).to(dev)
        # the row map is an input that stays the same from step to step (a foreign-key column): ordered once, like a prebuilt
        # r_index (spatial_index.rs:558-624); the one-shot call that orders it inside is timed next to it
        torch.cuda.synchronize()
        build = []
        rmap = None
        for _ in range(3 if args.full else 1):
            if rmap is not None:
                rmap.free()
            t0 = time.perf_counter()
            rmap = RowMap.from_device(ls, r_dev, stream=stream)
            torch.cuda.synchronize()
            build.append((time.perf_counter() - t0) * 1e3)

        def step(i: int) -> None:
            _abi.check(lib.gpk_distance_rowmap(pts.handle, ls.handle, rmap.handle, out.data_ptr(), _abi.MEM_DEVICE, stream))

        # (a step is one launch of gpk_distance_grouped: one event pair around the K launches — a pair per launch measured 0.565 ms
        # where the warm-up saw 0.493 and rocprofv3 0.515: the line now has ONE number for the kernel, gaps included)
        elapsed, k_ms, k_n, warm = ctx.timed(step, "gpk_distance_grouped", args.steps, args.warmup, one_launch_steps=lambda w: set(w) == {"gpk_distance_grouped"})
        results[label] = {"elapsed": elapsed, "k_ms": k_ms, "launches": k_n, "warm": warm, "parity": None, "rowmap_build_ms": min(build), "one_shot_ms": None}
        if args.dump_outputs and ctx.rank == 0 and label == "rows = i mod L":
            torch.cuda.synchronize()
            idx = sample_rows(n, DUMP_ROWS, seed=DUMP_SEED)
            dump_arrays(args.dump_outputs, {"sample_rows": idx, "distance": out.cpu().numpy()[idx]})
        if not args.full:
            rmap.free()
            break
        if ctx.rank == 0:
            results[label]["parity"] = parity_distance(pts_host, ls_host, rows, out, args.parity_rows)
        out.zero_()
        one = []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _abi.check(lib.gpk_distance_rowwise(pts.handle, ls.handle, r_dev.data_ptr(), out.data_ptr(), _abi.MEM_DEVICE, stream))
            torch.cuda.synchronize()
            one.append((time.perf_counter() - t0) * 1e3)
        results[label]["one_shot_ms"] = min(one[1:])
        if ctx.rank == 0:
            parity_distance(pts_host, ls_host, rows, out, 50_000)  # the one-shot path answers the same
        rmap.free()
    if ctx.rank != 0:
        ctx.finish()
        return
    main = results["rows = i mod L"]
    ms_per_step = main["elapsed"] / args.steps * 1e3
    v = ls_host.n_coords
    seg = float((np.diff(ls_host.geom_offsets)[rows_mod] - 1).clip(min=0).sum())  # segment evaluations of one step
    # 16N + 4N + 16 V_ls + 4 (L+1) + 8N, each distinct byte once
    nbytes = 16 * n + 4 * n + 16 * v + 4 * (L + 1) + 8 * n
    k_s = main["k_ms"] * 1e-3
    achieved = nbytes / k_s / 1e9 if k_s > 0 else 0.0
    instr_per_seg = 17.0  # vector instructions per segment step of gpk_distance_grouped, counted in the ISA (13 always + 6 when the projection falls inside the segment, ~60 % of the steps, + 2 when it is nearer)
    valu = seg * instr_per_seg / k_s if k_s > 0 else 0.0
    config = {
        "workload": f"C3: {n} points euclidean_distance to {L} linestrings (4-256 segments, {v} coordinates), row i -> linestring i mod L, per GPU",
        "points_per_gpu": n,
        "linestrings": L,
        "segment_evaluations_per_step": seg,
        "call": "gpk_distance_rowmap (device outputs) with a row map ordered once by gpk_rowmap_build; `one_shot_ms` = gpk_distance_rowwise with b_rows, which orders the map inside the call",
        "rowmap_build_ms": main["rowmap_build_ms"],
        "one_shot_ms": main["one_shot_ms"],
        "parallelism": f"row-sharded x{ctx.world}, right side replicated",
        "kernel_ms_per_step": main["warm"],
        "shuffled_row_map": {
            "ms_per_step": results["rows shuffled"]["elapsed"] / args.steps * 1e3,
            "rows_per_s": ctx.world * n * args.steps / results["rows shuffled"]["elapsed"],
            "kernel_ms_per_step": results["rows shuffled"]["warm"],
            "rowmap_build_ms": results["rows shuffled"]["rowmap_build_ms"],
            "one_shot_ms": results["rows shuffled"]["one_shot_ms"],
            "parity": results["rows shuffled"]["parity"],
        } if args.full else None,
    }
    roofline = {
        "bound": "hbm",
        "kernel": "gpk_distance_grouped",
        "achieved": achieved,
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBS,
        "traffic": None,
        "launch_ms": main["k_ms"],
        "launches": main["launches"],
        "launch_ms_method": "one HIP event pair around the K back-to-back launches / K" if getattr(ctx, "span_events", False) else "HIP event pair per launch",
        "frac_of_achievable": achieved / 6300.0,
        "algorithmic_bytes": nbytes,
        "valu": {"note": "the kernel is bound by f64 vector issue, not HBM", "achieved": valu, "peak": F64_VALU_PEAK, "unit": "f64 instr/s", "frac": valu / F64_VALU_PEAK, "instr_per_segment": instr_per_seg},
        "source_hash": source_hash(),
    }
    if n == 10_000_000 and args.lines == 100_000:
        roofline_traffic(roofline, "c3")
    line = base_line(ctx, "row-wise point-linestring distances/sec (10M pts x 100k linestrings)", ctx.world * n * args.steps / main["elapsed"], "rows/s", ms_per_step, "weak", config, roofline)
    if args.full:
        line["parity"] = main["parity"]
    if args.full and ctx.world == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline_distance(pts_host, ls_host, rows_mod, args.cpu_seconds)
    ctx.finish()  # (RCCL may print its banner while the group goes down: the JSON line stays the last line of stdout)
    emit_line(line)


def parity_distance(pts_host, ls_host, rows, gpu_out, k: int) -> dict:
    from oracle import pyoracle

    pyoracle.build()
    idx = sample_rows(len(pts_host), k, seed=4243)
    exp = pyoracle.distance_rowwise(pts_host.take(idx), ls_host, rows[idx], n_threads=0)
    got = gpu_out.cpu().numpy()[idx]
    rel = np.abs(got - exp) / np.maximum(np.abs(exp), 1e-300)
    ok = bool(np.all((rel <= 1e-9) | (got == exp)) and np.array_equal(got == 0.0, exp == 0.0) and np.array_equal(np.isnan(got), np.isnan(exp)))
    if not ok and os.environ.get("GPK_BENCH_ABLATION"):  # tuning builds that answer wrong on purpose (tools/): timing only, said on the line
        return {"rows": int(len(idx)), "ablation_build": True, "max_rel_err": float("nan")}
    if not ok:
        raise SystemExit("bench.py: GPU distances differ from the CPU oracle beyond 1e-9 on the parity sample — no speed reported")
    return {"rows": int(len(idx)), "sampling": "uniform random without replacement (seed 4243)", "tolerance": "1e-9 relative, zero / non-zero exact", "max_rel_err": float(rel[np.isfinite(rel)].max(initial=0.0))}


def cpu_baseline_distance(pts_host, ls_host, rows, target_s: float) -> dict:
    from oracle import pyoracle

    n = len(pts_host)
    probe = min(n, 200_000)
    t0 = time.perf_counter()
    pyoracle.distance_rowwise(pts_host.take(np.arange(probe)), ls_host, rows[:probe], n_threads=0)
    dt = max(time.perf_counter() - t0, 1e-3)
    sample = int(min(n, max(probe, probe * target_s / (2.0 * dt))))
    sub = pts_host.take(np.arange(sample))
    best, runs, spent = None, 0, 0.0
    while runs < 2 or (runs < 9 and spent < target_s / 4):
        t0 = time.perf_counter()
        pyoracle.distance_rowwise(sub, ls_host, rows[:sample], n_threads=0)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        runs += 1
        spent += dt
    s1 = min(sample, 200_000)
    t0 = time.perf_counter()
    pyoracle.distance_rowwise(pts_host.take(np.arange(s1)), ls_host, rows[:s1], n_threads=1)
    t_single = time.perf_counter() - t0
    return {
        "value": sample / best,
        "unit": "rows/s",
        "cores": os.cpu_count(),
        "kind": "port",
        "sample": f"first {sample} of the {n} rows, min of {runs} runs, oracle/gpk_oracle.c point-linestring distance, OpenMP over rows",
        "seconds": best,
        "single_thread": {"value": s1 / t_single, "unit": "rows/s", "sample_rows": s1, "seconds": t_single},
    }


# ======================================================================================================
# C4 — polygon x polygon intersects join, left side row-sharded, right side gathered once
# ======================================================================================================
def run_c4(ctx: Ctx) -> None:
    torch, args, lib = ctx.torch, ctx.args, ctx.lib
    from geopolars_amd import _abi, synth
    from geopolars_amd.dist import Comm, GeoBuffers, all_gather_leaves, all_gatherv_buffers, shard_rows, slice_rows
    from geopolars_amd.spatial_index import SpatialIndex, join_pairs_device

    n, dev, stream, W = args.polygons, ctx.dev, ctx.stream, ctx.world
    left_full = synth.clustered_polygons(n, seed=41, mean_neighbours=4.0)
    right_full = synth.clustered_polygons(n, seed=42, mean_neighbours=4.0)
    # left: contiguous row ranges balanced by vertex count; right: every rank owns a row range and the ranks exchange them
    wl = np.diff(left_full.ring_offsets)[left_full.geom_offsets[:-1]]  # exterior vertex count per row (one ring per polygon here)
    lo, hi = shard_rows(n, W, ctx.rank, weights=wl)
    left_host = slice_rows(left_full, lo, hi)
    rlo, rhi = shard_rows(n, W, ctx.rank)
    right_shard = GeoBuffers.from_host(slice_rows(right_full, rlo, rhi), dev)
    exchange = {"ms": 0.0, "bytes": 0}
    torch.cuda.synchronize()
    if ctx.use_dist:
        # what each rank built for its shard — the boxes (R-tree leaves) — travels with the geometry: one all-gatherv over xGMI
        shard_arr = right_shard.to_device_geoarray(stream)
        box = torch.empty((rhi - rlo, 4), dtype=torch.float64, device=dev)
        _abi.check(lib.gpk_bounds(shard_arr.handle, box.data_ptr(), _abi.MEM_DEVICE, stream))
        # (the unique id travels over the torch group: any side channel would do; bounded wait + agreed fallback: open_comm_guarded)
        comm, comm_note = open_comm_guarded(ctx, args.comm_timeout) if args.comm == "abi" else (None, "")
        ctx.barrier()
        t0 = time.perf_counter()
        stats = {}
        if comm is not None:  # the exchange through the C ABI: gpk_allgatherv_geoarray / gpk_allgatherv_rows_f64 (RCCL opened by the library)
            right, _, gathered = comm.all_gatherv(shard_arr, stream=stream)
            leaves = comm.all_gather_rows(box, stream=stream)
            stats["gathered_bytes"] = gathered
        else:
            right_buf = all_gatherv_buffers(right_shard, stats=stats)
            leaves = all_gather_leaves(box)
            right = right_buf.to_device_geoarray(stream)
        ctx.barrier()
        exchange = {"ms": ctx.max_over_ranks(time.perf_counter() - t0) * 1e3, "bytes": stats["gathered_bytes"] + leaves.numel() * 8,
                    "through": "C ABI (gpk_allgatherv_*)" if comm is not None else "torch.distributed (geopolars_amd.dist)" + (f" — fallback: {comm_note}" if comm_note else "")}
    else:
        right, leaves = right_shard.to_device_geoarray(stream), None
    left = dev_array(torch, left_host, dev, stream)
    nl = hi - lo
    build_ms = []
    index = None
    for _ in range(3 if args.full else 1):
        if index is not None:
            index.free()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = SpatialIndex.from_device(right, stream=stream, for_points=False, bboxes=leaves)  # bbox + grid directory: what this arm reads
        torch.cuda.synchronize()
        build_ms.append((time.perf_counter() - t0) * 1e3)
    counts = torch.empty(nl, dtype=torch.int32, device=dev)
    cap = max(8 * nl, 1024)
    pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    hits = {"h": 0}

    def step(i: int) -> None:
        hits["h"] = join_pairs_device(left, right, index, "intersects", counts, pairs, left_row_base=lo, stream=stream)

    elapsed, k_ms, k_n, warm = ctx.timed(step, "gpk_pair_refine", args.steps, args.warmup)
    h = hits["h"]
    if args.dump_outputs and ctx.rank == 0:
        dump_join(args.dump_outputs, counts, pairs, h, base=lo)
    total_pairs = ctx.sum_over_ranks(float(h))
    parity = parity_poly_join(left_host, right_full, counts, pairs, h, lo, args.parity_rows) if args.full and ctx.rank == 0 else None
    if ctx.rank != 0:
        ctx.finish()
        return
    ms_per_step = elapsed / args.steps * 1e3
    # both coordinate sets once + bbox arrays (32 B / geometry) + 8 B per output pair (this rank's share of the left side)
    nbytes = 16 * (left_host.n_coords + right_full.n_coords) + 32 * (nl + n) + 8 * h
    k_s = k_ms * 1e-3
    config = {
        "workload": f"C4: {n} x {n} polygons (8-64 vertices, ~4 bbox neighbours) intersects() spatial join; left side row-sharded x{W} by vertex weight, right side exchanged once",
        "left_rows_this_rank": nl,
        "right_rows": n,
        "pairs_total": int(total_pairs),
        "pairs_this_rank": h,
        "call": "gpk_spatial_join (blocking; candidate generation + 16-lane exact refine + sorted pair emit), prebuilt r_index",
        "index": "gpk_index_build_ex(GPK_INDEX_BBOX_GRID" + (", leaves from the exchange)" if leaves is not None else ")"),
        "index_build_ms": min(build_ms),
        "join_ms": ms_per_step,
        "build_plus_join_ms": min(build_ms) + ms_per_step,
        "note_build": "spatial_join without r_index pays build + join (spatial_index.rs:47-71); `value` is the join with a prebuilt r_index (spatial_index.rs:558-624)",
        "right_side_exchange": {"ms": exchange["ms"], "bytes": exchange["bytes"], "through": exchange.get("through"), "what": "all-gatherv of the right GeoArrow buffers + the per-geometry boxes, device-resident, outside the timed region"},
        "kernel_ms_per_step": warm,
        "parallelism": f"left row-sharded x{W} (strong scaling: the 1M x 1M problem is fixed), right side all-gathered",
    }
    achieved = nbytes / k_s / 1e9 if k_s > 0 else 0.0
    roofline = {
        "bound": "hbm",
        "kernel": "gpk_pair_refine",
        "achieved": achieved,
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBS,
        "traffic": None,
        "launch_ms": k_ms,
        "launches": k_n,
        "algorithmic_bytes": nbytes,
        "note": "candidate refine is VALU-bound (exact segment-pair tests), the candidate passes are gather-bound; the HBM fraction is reported as the contract asks",
        "source_hash": source_hash(),
    }
    if args.polygons == 1_000_000 and W == 1:
        roofline_traffic(roofline, "c4")
    line = base_line(ctx, "polygon-pair intersects() join rows/sec (1M x 1M polygons)", n * args.steps / elapsed, "left rows/s", ms_per_step, "strong", config, roofline)
    if args.full:
        line["parity"] = parity
    if args.full and W == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline_polyjoin(left_host, right_full, counts, args.cpu_seconds)
    ctx.finish()  # (RCCL may print its banner while the group goes down: the JSON line stays the last line of stdout)
    emit_line(line)


def parity_poly_join(left_host, right_host, gpu_counts, gpu_pairs, h: int, base: int, rows: int) -> dict:
    from oracle import pyoracle

    pyoracle.build()
    idx = sample_rows(len(left_host), rows, seed=4244)
    ep, ec, _ = pyoracle.spatial_join(left_host.take(idx), right_host, "intersects", mode=1, n_threads=0)
    gc = gpu_counts.cpu().numpy().astype(np.uint32)
    gp = gpu_pairs[:h].cpu().numpy().astype(np.uint32)
    got = pairs_of_rows(gp, (idx + base).astype(np.uint32))
    if not np.array_equal(gc[idx], ec) or not np.array_equal(got, ep) or int(gc.sum()) != h:
        raise SystemExit("bench.py: GPU polygon join differs from the CPU oracle on the parity sample — no speed reported")
    return {"rows": int(len(idx)), "sampling": "uniform random without replacement (seed 4244)", "pairs_checked": int(len(ep)), "bit_exact": True}


def cpu_baseline_polyjoin(left_host, right_host, gpu_counts, target_s: float) -> dict:
    from oracle import pyoracle

    n = len(left_host)
    probe = min(n, 20_000)
    t0 = time.perf_counter()
    pyoracle.spatial_join(left_host.take(np.arange(probe)), right_host, "intersects", mode=1, n_threads=0)
    dt = max(time.perf_counter() - t0, 1e-3)
    sample = int(min(n, max(probe, probe * target_s / dt)))
    t0 = time.perf_counter()
    _, counts, threads = pyoracle.spatial_join(left_host.take(np.arange(sample)), right_host, "intersects", mode=1, n_threads=0)
    best = time.perf_counter() - t0
    if not np.array_equal(gpu_counts[:sample].cpu().numpy().astype(np.uint32), counts):
        raise SystemExit("bench.py: GPU hit counts differ from the CPU oracle on the baseline sample — no speed reported")
    return {
        "value": sample / best,
        "unit": "left rows/s",
        "cores": threads,
        "kind": "port",
        "sample": f"first {sample} of the {n} left rows against all {len(right_host)} right rows (the time includes the oracle's own grid directory build over the right side), OpenMP dynamic",
        "seconds": best,
        "parity_checked_rows": sample,
    }


# ======================================================================================================
# C5 — points within power-law multipolygons + area
# ======================================================================================================
def c5_chunk(k: int, rows: int):
    from geopolars_amd import synth

    return synth.powerlaw_multipolygons(rows, seed=51 + k, size_n=rows * C5_CHUNKS)  # sized as part of ONE 5M-row column


def run_c5(ctx: Ctx) -> None:
    torch, args, lib = ctx.torch, ctx.args, ctx.lib
    from geopolars_amd import _abi, synth
    from geopolars_amd.dist import GeoBuffers, all_gatherv_buffers
    from geopolars_amd.geoarrow import GeoArrowArray
    from geopolars_amd.spatial_index import SpatialIndex, join_pairs_device, join_pairs_enqueue

    n, M, dev, stream, W = args.points, args.multipolygons, ctx.dev, ctx.stream, ctx.world
    if C5_CHUNKS % W:
        raise SystemExit("bench.py --config c5: --gpus must divide 8")
    rows_per_chunk = M // C5_CHUNKS
    mine = range(ctx.rank * C5_CHUNKS // W, (ctx.rank + 1) * C5_CHUNKS // W)
    t0 = time.perf_counter()
    shard_host = GeoArrowArray.concat([c5_chunk(k, rows_per_chunk) for k in mine])
    gen_s = time.perf_counter() - t0
    shard = GeoBuffers.from_host(shard_host, dev)
    exchange = {"ms": 0.0, "bytes": 0}
    torch.cuda.synchronize()
    if ctx.use_dist:
        ctx.barrier()
        t0 = time.perf_counter()
        stats = {}
        right_buf = all_gatherv_buffers(shard, stats=stats)
        ctx.barrier()
        exchange = {"ms": ctx.max_over_ranks(time.perf_counter() - t0) * 1e3, "bytes": stats["gathered_bytes"]}
    else:
        right_buf = shard
    right = right_buf.to_device_geoarray(stream)
    area_share = shard.to_device_geoarray(stream)  # area() is a per-row map: every rank keeps the rows it generated
    n_share = shard.n_geoms
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = SpatialIndex.from_device(right, stream=stream)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    # the same build once more: the first one also grows the library's scratch arenas and size-classifies the column (one-off per process / column)
    build_again_ms = None
    if args.full:
        t0 = time.perf_counter()
        again = SpatialIndex.from_device(right, stream=stream)
        torch.cuda.synchronize()
        build_again_ms = (time.perf_counter() - t0) * 1e3
        again.free()
    pts_host = synth.uniform_points(n, seed=52 + ctx.rank)
    if args.diag_sorted_points:  # diagnosis only (never the reported configuration): the same points in raster order
        xy = pts_host.xy
        key = (np.floor(xy[:, 1] / synth.DOMAIN * 4096).astype(np.int64) << 12) | np.floor(xy[:, 0] / synth.DOMAIN * 4096).astype(np.int64)
        pts_host = pts_host.take(np.argsort(key, kind="stable"))
    pts = dev_array(torch, pts_host, dev, stream)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    pairs = torch.empty((4 * n, 2), dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    area = torch.empty(n_share, dtype=torch.float64, device=dev)

    def step(i: int) -> None:
        join_pairs_enqueue(pts, right, index, "within", counts, pairs, total, left_row_base=0, stream=stream)
        _abi.check(lib.gpk_area(area_share.handle, area.data_ptr(), _abi.MEM_DEVICE, stream))

    elapsed, k_ms, k_n, warm = ctx.timed(step, "gpk_pip_tile", args.steps, args.warmup)
    torch.cuda.synchronize()
    h = int(total.item())
    if h > pairs.shape[0]:
        raise SystemExit(f"bench.py --config c5: {h} pairs exceed the pair buffer")
    if args.dump_outputs and ctx.rank == 0:
        dump_join(args.dump_outputs, counts, pairs, h, per_row={"area": area})
    st = (C.c_int64 * 4)()  # what the exact phase did, on one extra untimed join
    join_stats = args.full and not args.no_join_stats
    if join_stats:
        lib.gpk_join_stats_enable(1)
        lib.gpk_join_stats(st, 1)
        join_pairs_enqueue(pts, right, index, "within", counts, pairs, total, left_row_base=0, stream=stream)
        lib.gpk_join_stats(st, 1)
        lib.gpk_join_stats_enable(0)
        torch.cuda.synchronize()
    # area over ALL multipolygons of the gathered right side, once (what one GPU would do alone)
    area_all_ms = None
    if args.full:
        area_all = torch.empty(right_buf.n_geoms, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            _abi.check(lib.gpk_area(right.handle, area_all.data_ptr(), _abi.MEM_DEVICE, stream))
        torch.cuda.synchronize()
        area_all_ms = (time.perf_counter() - t0) * 1e3 / 3
    # the same join against an index WITH the per-entry records of its list cells (GPK_INDEX_PIP_FULL): reported, not the headline
    index_full = None
    if args.full and W == 1 and not args.no_index_variants:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        full = SpatialIndex.from_device(right, stream=stream, full=True)
        torch.cuda.synchronize()
        full_build_ms = (time.perf_counter() - t0) * 1e3
        for _ in range(2):
            join_pairs_enqueue(pts, right, full, "within", counts, pairs, total, left_row_base=0, stream=stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            join_pairs_enqueue(pts, right, full, "within", counts, pairs, total, left_row_base=0, stream=stream)
        torch.cuda.synchronize()
        index_full = {"parts": "GPK_INDEX_BBOX_GRID | GPK_INDEX_PIP | GPK_INDEX_PIP_FULL", "build_ms": full_build_ms, "bytes": full.nbytes(),
                      "join_ms": (time.perf_counter() - t0) * 1e3 / 5, "pairs_equal_the_default_index": int(total.item()) == h}
        full.free()
    # ---- the ONE-SHOT cost with the RIGHT side partitioned (dist.join_partition_right): every rank indexes its own shard of the
    # multipolygons (1 / N of the build) and joins ALL points against it.  At N = 1 the work of rank 0 of `--simulate-ranks` ranks
    # is measured on this GPU (its shard of the right side = the first 1 / K of the rows, all K x n points) — the collective that
    # replicates the points (16 bytes a row) is the one thing that cannot be timed on one GPU.
    one_shot = None
    if args.full and not args.no_one_shot:
        try:
            from geopolars_amd.dist import join_partition_right

            K = W if W > 1 else max(1, args.simulate_ranks)
            if W > 1:
                my_shard, my_base, xy_mine = shard, ctx.rank * (M // W), torch.from_numpy(pts_host.xy).to(dev)
            else:
                sh_host = c5_chunk(0, rows_per_chunk) if K == C5_CHUNKS else GeoArrowArray.concat([c5_chunk(k, rows_per_chunk) for k in range(C5_CHUNKS // K)])
                my_shard, my_base = GeoBuffers.from_host(sh_host, dev), 0
                xy_mine = torch.cat([torch.from_numpy(synth.uniform_points(n, seed=52 + r).xy).to(dev) for r in range(K)])
            my_dev = my_shard.to_device_geoarray(stream)
            join_partition_right(xy_mine[: min(len(xy_mine), 100_000)], my_dev, my_base, "within", stream=stream)  # (arenas, size classes: one-off per process / column)
            ctx.barrier()
            t0 = time.perf_counter()
            res = join_partition_right(xy_mine, my_dev, my_base, "within", stream=stream, pair_capacity=int(xy_mine.shape[0]) if W == 1 else None)
            ctx.barrier()
            wall = ctx.max_over_ranks(time.perf_counter() - t0) * 1e3
            one_shot = {
                "what": f"dist.join_partition_right: points replicated, rank r indexes 1/{K} of the multipolygons and joins all {int(res['counts'].shape[0])} points against them" + ("" if W > 1 else f" — rank 0 of {K}, measured on this one GPU (no collective)"),
                "ranks": K,
                "index_build_ms": res["ms"]["index"],
                "join_ms": res["ms"]["join"],
                "gather_points_ms": res["ms"]["gather"] if W > 1 else None,
                "wall_ms_max_over_ranks": wall,
                "pairs_on_this_rank": int(res["pairs"].shape[0]),
                "compare": {"replicated_right_one_shot_ms": build_ms + elapsed / args.steps * 1e3, "note": "index over ALL multipolygons on every rank + one step"},
            }
            if W == 1:  # parity of the partitioned join on a random sample of its rows against the oracle on the same shard
                from oracle import pyoracle

                pyoracle.build()
                nn = int(res["counts"].shape[0])
                idx = sample_rows(nn, min(args.parity_rows, 100_000), seed=99)
                sub = GeoArrowArray.from_points(xy_mine[torch.from_numpy(idx).to(dev)].cpu().numpy())
                ep, ec, _ = pyoracle.spatial_join(sub, my_shard.to_host(), "within", mode=1, n_threads=0)
                gc = res["counts"].cpu().numpy().astype(np.uint32)
                got = pairs_of_rows(res["pairs"].cpu().numpy().astype(np.uint32), idx.astype(np.uint32))
                if not np.array_equal(gc[idx], ec) or not np.array_equal(got, ep):
                    raise SystemExit("bench.py: the right-partitioned join differs from the CPU oracle on its parity sample")
                one_shot["parity"] = {"rows": int(len(idx)), "pairs": int(len(ep)), "bit_exact": True}
            del res, xy_mine
        except SystemExit:
            raise
        except Exception as e:  # (a measurement next to the line, never the line itself)
            one_shot = {"error": repr(e)}
    if ctx.rank != 0:
        ctx.finish()
        return
    right_host = right_buf.to_host() if W > 1 else shard_host
    ms_per_step = elapsed / args.steps * 1e3
    nbytes = 16 * n + 16 * right_host.n_coords + 4 * (right_host.n_geoms + right_host.n_parts + right_host.n_rings + 3) + 4 * n
    k_s = k_ms * 1e-3
    achieved = nbytes / k_s / 1e9 if k_s > 0 else 0.0
    area_bytes = 16 * shard_host.n_coords + 4 * (shard_host.n_geoms + shard_host.n_parts + shard_host.n_rings + 3) + 8 * n_share
    area_ms = sum(v for k, v in warm.items() if "area" in k or "seq_long" in k)
    config = {
        "workload": ("DIAGNOSIS (points in raster order) " if args.diag_sorted_points else "") + f"C5: {n} points (one rank's share of 50M) within() all {right_host.n_geoms} power-law multipolygons ({right_host.n_coords} coordinates) + area() of {n_share} of them, per GPU",
        "points_per_gpu": n,
        "multipolygons": right_host.n_geoms,
        "coordinates": right_host.n_coords,
        "hits_per_step": h,
        "exact_phase": {"queued_point_part_pairs_per_step": int(st[0]), "edge_tests_per_step": int(st[1])} if join_stats else None,
        "call": "gpk_spatial_join_async(within) + gpk_area, one stream",
        "index_build_ms": build_ms,
        "index_build_again_ms": build_again_ms,
        "index_bytes": index.nbytes(),
        "index_describe": index.describe(),
        "index_full_variant": index_full,
        "join_ms_per_step": sum(v for k, v in warm.items() if "pip_" in k),
        "area_ms_per_step": area_ms,
        "area_GBps": area_bytes / (area_ms * 1e-3) / 1e9 if area_ms > 0 else None,
        "area_all_multipolygons_ms": area_all_ms,
        "build_plus_step_ms": build_ms + ms_per_step,
        "one_shot_right_partitioned": one_shot,
        "right_side_exchange": {"ms": exchange["ms"], "bytes": exchange["bytes"], "what": "all-gatherv of the right GeoArrow buffers, device-resident, outside the timed region; every rank then builds the index over the gathered column"},
        "host_generation_s": gen_s,
        "kernel_ms_per_step": warm,
        "parallelism": f"points row-sharded x{W} (weak: 6.25M per GPU, 50M at 8), multipolygons replicated by the exchange",
    }
    roofline = {
        "bound": "hbm",
        "kernel": "gpk_pip_tile",
        "achieved": achieved,
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBS,
        "traffic": None,
        "launch_ms": k_ms,
        "launches": k_n,
        "algorithmic_bytes": nbytes,
        "note": "latency-bound gathers into a multi-gigabyte index (raster words, level-2 records, edge slabs), not a streaming kernel; the streaming part of the step is area()",
        "source_hash": source_hash(),
    }
    if n == 6_250_000 and args.multipolygons == 5_000_000:
        roofline_traffic(roofline, "c5")
        rec, _ = pmc_config_record("c5")
        if rec and rec.get("fetch_bytes_raw") and k_s > 0:
            # The kernel does not stream its algorithmic bytes — it never reads most of the right side's coordinates — it gathers
            # scattered cache lines out of a multi-gigabyte index.  Its stated roofline is therefore the rate of scattered 64-byte
            # lines (TCC_EA0_RDREQ = FETCH_SIZE / 64 B, from the committed counter record) against what the memory system delivers
            # for INDEPENDENT scattered lines at this footprint (tools/micro/random_lines.hip: 50 G lines/s = 3.2 TB/s at 3 GB).
            # Round 5: `frac` is stated against the guide's 8 TB/s like every other line (algorithmic bytes / launch time); the
            # scattered-line view — what the memory system delivers for INDEPENDENT scattered 64-byte lines at this footprint
            # (tools/micro/random_lines.hip: 50 G lines/s = 3.2 TB/s at 3 GB) — is a secondary field.
            lines = rec["fetch_bytes_raw"] / 64.0
            roofline["scattered_lines"] = {"lines_per_launch": lines, "lines_per_s": lines / k_s, "achieved_GBps": lines * 64.0 / k_s / 1e9, "peak_GBps": RANDOM_LINE_PEAK_GBS,
                                           "frac": lines * 64.0 / k_s / 1e9 / RANDOM_LINE_PEAK_GBS,
                                           "note": "counted TCC_EA0_RDREQ lines x 64 B / launch time against 50 G independent random lines/s x 64 B"}
    line = base_line(ctx, "predicate evals/sec (points within power-law multipolygons, + area)", float(W) * n * right_host.n_geoms * args.steps / elapsed, "evals/s", ms_per_step, "weak", config, roofline)
    if args.full:
        line["parity"] = parity_point_join(pts_host, right_host, "within", counts, pairs, h, args.parity_rows)
        line["parity"]["area"] = parity_area(shard_host, area)
    if args.full and W == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline_join(pts_host, right_host, "within", counts, args.cpu_seconds)
    ctx.finish()  # (RCCL may print its banner while the group goes down: the JSON line stays the last line of stdout)
    emit_line(line)


def parity_area(host, gpu_area) -> dict:
    from oracle import pyoracle

    exp = pyoracle.area(host)
    got = gpu_area.cpu().numpy()
    rel = np.abs(got - exp) / np.maximum(np.abs(exp), 1e-300)
    if not bool(np.all((rel <= 1e-9) | (got == exp))):
        raise SystemExit("bench.py: GPU areas differ from the CPU oracle beyond 1e-9 — no speed reported")
    return {"rows": int(len(exp)), "tolerance": "1e-9 relative", "max_rel_err": float(rel.max(initial=0.0))}


# ------------------------------------------------------------------------------------------------------
def self_launch(n: int) -> int:
    """`python bench.py --gpus N` without a launcher: re-run this very command line as N ranks of one node under
    torch.distributed.run (one process per GPU, RCCL over xGMI, rendezvous on 127.0.0.1 at a free port).  Rank 0's JSON line
    comes through on stdout unchanged; the exit status is the launcher's."""
    import socket
    import subprocess

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__), *sys.argv[1:]]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # the host driver only supports dmabuf IPC (RCCL needs it across processes)
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // n)))
    print(f"bench.py: --gpus {n} without WORLD_SIZE: launching {n} ranks under torch.distributed.run (port {port})", file=sys.stderr)
    return subprocess.call(cmd, env=env)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["c2", "c3", "c4", "c5"], default="c2")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="also run what the headline figure does not need: oracle parity, the CPU baseline and every secondary measurement the configuration reports (the --no-* options below trim a full run)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write what the last timed step computed (rank 0; per-row outputs at a fixed sample of rows) as DIR/<name>.npy")
    ap.add_argument("--points", type=int, default=None, help="left rows per GPU (c2/c3: 10M, c5: 6.25M)")
    ap.add_argument("--polys", type=int, default=1000, help="c2: right-side polygons")
    ap.add_argument("--verts", type=int, default=64, help="c2: vertices per polygon")
    ap.add_argument("--lines", type=int, default=100_000, help="c3: right-side linestrings")
    ap.add_argument("--polygons", type=int, default=1_000_000, help="c4: polygons per side")
    ap.add_argument("--multipolygons", type=int, default=5_000_000, help="c5: right-side multipolygons (all of them on every GPU)")
    ap.add_argument("--rotate", type=int, default=3, help="c2: distinct input/output sets cycled through by the steps (cold inputs)")
    ap.add_argument("--diag-sorted-points", action="store_true", help="c5, diagnosis: feed the points in raster order (how much of the tile kernel is locality)")
    ap.add_argument("--no-index-variants", action="store_true", help="c5: skip the extra build + joins of the GPK_INDEX_PIP_FULL index")
    ap.add_argument("--parity-rows", type=int, default=300_000, help="random sample of left rows compared with the oracle")
    ap.add_argument("--no-one-shot", action="store_true", help="c5: skip the right-partitioned one-shot measurement")
    ap.add_argument("--simulate-ranks", type=int, default=8, help="c5 at N = 1: whose work the right-partitioned one-shot join measures (rank 0 of this many)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target wall time of the cpu_baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--index-per-step", action="store_true", help="c2: rebuild the right-side index inside every step")
    ap.add_argument("--sync-steps", action="store_true", help="c2: use the synchronous gpk_spatial_join (host waits for every step)")
    ap.add_argument("--no-profile", action="store_true", help="tuning only: no HIP events around the kernels (the roofline leg reads zero)")
    ap.add_argument("--no-join-stats", action="store_true", help="c2: skip the extra untimed step that counts the exact phase's work (its atomics make that one launch ~7x longer: kernel-trace averages of a profiler run stay clean without it)")
    ap.add_argument("--force-dist", action="store_true", help="initialise RCCL and run the exchange even at world size 1 (path test)")
    ap.add_argument("--as-shard", default="", metavar="R/W", help="c2, test hook: run shard R of W of the strong-scaled problem in this one process")
    ap.add_argument("--force-weak", action="store_true", help="c2, test hook: run the weak-scaled measurement at N = 1 too (the code path of N > 1 on a one-GPU box)")
    ap.add_argument("--no-weak", action="store_true", help="c2 at N > 1: skip the weak-scaled measurement (10M points per GPU) reported beside the strong-scaled headline")
    ap.add_argument("--no-default-shape", action="store_true", help="c2 at N = 1: skip the r_index = None measurement (index built inside every call)")
    ap.add_argument("--comm", choices=["torch", "abi"], default="abi", help="c4: the right-side exchange through torch.distributed (geopolars_amd.dist) or through the library's own RCCL entry points (gpk_allgatherv_*)")
    ap.add_argument("--comm-timeout", type=float, default=120.0, help="c4: seconds to wait for the library's communicator (gpk_comm_init + a probe collective) before every rank falls back to --comm torch")
    ap.add_argument("--watchdog", type=float, default=3000.0, help="seconds after which rank 0 prints the JSON line with an `error` field and every rank exits (also when another rank has died)")
    ap.add_argument("--spawn", action="store_true", help="launch the rank(s) under torch.distributed.run even for --gpus 1 (what --gpus N > 1 does by itself when there is no launcher)")
    args = ap.parse_args()
    if args.steps is None:
        args.steps = {"c2": 20, "c3": 10, "c4": 10, "c5": 10}[args.config]
    if args.points is None:
        args.points = {"c2": 10_000_000, "c3": 10_000_000, "c4": 0, "c5": 6_250_000}[args.config]
    if (args.gpus > 1 or args.spawn) and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    start_watchdog(args, rank, args.watchdog)
    try:
        if os.environ.get("GPK_BENCH_RAISE"):  # test hooks (tests/test_host_cpu.py): a rank that dies / a run that never ends
            raise RuntimeError(os.environ["GPK_BENCH_RAISE"])
        if os.environ.get("GPK_BENCH_HANG"):
            time.sleep(1e6)
        ctx = Ctx(args)
        {"c2": run_c2, "c3": run_c3, "c4": run_c4, "c5": run_c5}[args.config](ctx)
    except SystemExit:
        raise
    except BaseException as e:  # noqa: BLE001 — whatever happened, rank 0 prints ONE JSON line that says so
        import traceback

        traceback.print_exc()
        msg = f"rank {rank}: {type(e).__name__}: {e}"
        try:
            with open(os.path.join(_marker_dir(), f"rank{rank}.err"), "w") as f:
                f.write(msg)
        except OSError:
            pass
        if rank == 0:
            emit_line(error_line(args, msg))
        os._exit(5)  # (not sys.exit: a rank stuck inside a collective on another thread must not keep the process alive)


if __name__ == "__main__":
    main()
