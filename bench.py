#!/usr/bin/env python3
"""bench.py -- disparity maps/sec of the MI355X-native stereo-matching hot path.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]

Workload (BASELINE.json): synthetic 1242x375 grayscale pairs, D=128, K=2 (config C2's shape);
one "step" = one pass of the whole hot path (prologue -> cost volume + aggregation + WTA ->
secondary matching -> bilateral fills) over a batch of PAIRS_PER_GPU distinct pairs that are
already resident in HBM (float32 gray, as B_alg = 12*H*W bytes/pair assumes).

Multi-GPU: one process per GPU, no data-path collective and no RCCL (north_star: "per-GPU HIP
streams only").  `python bench.py --gpus N` starts its own N rank processes (before anything
touches a GPU); under `torch.distributed.run` (RANK set) it is one of the ranks.  Either way the
ranks meet in a gloo group that carries ONLY the barrier and the MAX over ranks of the elapsed
time.  Rank r owns the pairs sharding.shard_indices() gives it (pair i -> device i mod N); every
rank processes PAIRS_PER_GPU pairs per step, so scaling is weak and at N = 8 one step is
BASELINE config 3 (512 pairs).  Rank 0 prints ONE JSON line.

Besides `value` the line carries (rank 0):
  single_pair_latency_us   config C2 literally: one pair per call, median of 200 HIP-event timings
  value_noise / value_slanted   same batch shape on pure-noise / scene-like pairs (worst case of the sparse pass)
  value_rgb                config C5 (D=192) through the RGB entry -- the reference's real call path
  value_real / value_real_rgb   the reference's own sample pair (real texture, 1242x375 crop, disparities 75..262)
  c3                       512 distinct pairs over the N devices, wall-clock incl. every sync, and the
                           same with uint8 inputs uploaded from pinned host memory (PCIe-inclusive)
  roofline, cpu_baseline   as the measurement contract asks; device copy bandwidth beside the peak

The HIP library is the only compute path; the CPU oracle is used solely for `cpu_baseline`.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd")]

H, W, K, D = 375, 1242, 2, 128
PAIRS_PER_GPU = 64
C3_PAIRS = 512
HBM_PEAK_GBPS = 8000.0           # MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)
B_ALG_PER_PAIR = 12 * H * W      # 2 gray f32 inputs + 1 f32 output
DUMP_BYTES = 64 * 10**6          # --dump-outputs: at most this much in all ranks' files together
DUMP_SEED = 0                    # --dump-outputs: which pairs of a batch are written

CONFIGS = [
    # name, H, W, K, dmin, dmax, entry, batch          (BASELINE.md section 2.2 + the reference's defaults)
    ("C1 320x240 D=32 K=1", 240, 320, 1, 0, 31, "gray", 256),
    ("C2 1242x375 D=128 K=2", 375, 1242, 2, 0, 127, "gray", 64),
    ("C4 3840x2160 D=256 K=4", 2160, 3840, 4, 0, 255, "gray", 16),
    ("C5 1242x375 D=192 K=2 RGB", 375, 1242, 2, 0, 191, "rgb", 32),
    ("C5 shape, gray entry", 375, 1242, 2, 0, 191, "gray", 64),
    ("ref-native 384x1280 D=0..64 K=2", 384, 1280, 2, 0, 64, "gray", 64),
    ("ref-native 384x1280 D=0..64 K=2 RGB", 384, 1280, 2, 0, 64, "rgb", 32),
    ("ref-default 1920x1080 D=75..262 K=2", 1080, 1920, 2, 75, 262, "gray", 16),
    ("ref-default 1920x1080 D=75..262 K=2 RGB", 1080, 1920, 2, 75, 262, "rgb", 8),
]


# ----------------------------------------------------------------------------- multi-process plumbing
def rank_env():
    """(rank, local_rank, world_size) from the launcher's environment."""
    return (int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")),
            int(os.environ.get("WORLD_SIZE", "1")))


def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n: int, argv) -> int:
    """Self-launch: n fresh processes of this script, one per device.  The parent never touches a GPU
    (no torch import at all) and only waits; rank 0 inherits stdout and prints the JSON line."""
    port = free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
    rc = 0
    for p in procs:
        rc = p.wait() or rc
    return rc


class TimingGroup:
    """Barrier + MAX-reduce of one scalar over the ranks, on gloo (CPU): timing only, never data."""

    def __init__(self, rank: int, world: int):
        self.world = world
        self.dist = None
        if world > 1:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29555")
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
            self.dist = dist

    def barrier(self) -> None:
        if self.dist is not None:
            self.dist.barrier()

    def max(self, x: float) -> float:
        if self.dist is None:
            return float(x)
        import torch
        t = torch.tensor([x], dtype=torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def close(self) -> None:
        if self.dist is not None:
            self.dist.destroy_process_group()


def timed_steps(step, device_sync, group: TimingGroup, steps: int, warmup: int) -> float:
    """The contract's timed region: `warmup` untimed steps, then exactly `steps` steps bracketed by
    device sync + barrier on both sides; returns the MAX over ranks of the elapsed seconds."""
    for _ in range(warmup):
        step()
    device_sync()
    group.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    device_sync()
    elapsed = time.perf_counter() - t0
    group.barrier()
    return group.max(elapsed)


# ----------------------------------------------------------------------------- host-side data
def _pair_job(a):
    import stereo_synthetic as syn
    kind, idx = a
    if kind == "band":
        return syn.make_pair(H, W, D, K, idx)[:2]
    if kind == "noise":
        return syn.make_noise_pair(H, W, idx)
    return syn.make_slanted_pair(H, W, D, K, idx)[:2]


def _pool_allowed() -> bool:
    """A fork pool is only safe while nothing in this process has initialised the GPU.  Under rocprofv3 the
    profiler's preloaded library has done so before main() runs (forked children then hang), so profiled
    runs generate their inputs serially."""
    env = os.environ
    return not (any(k.startswith(("ROCPROF", "ROCP_", "ROCTRACER")) for k in env) or "rocprof" in env.get("LD_PRELOAD", "")
                or env.get("SMX_BENCH_SERIAL") == "1")


def make_pairs(kind: str, indices, parallel: bool = True):
    """[n,H,W] float32 left / right for the global pair indices (seed 1234 + index), generated by a
    small process pool BEFORE this process initialises the GPU."""
    import numpy as np
    jobs = [(kind, int(i)) for i in indices]
    workers = min(8, os.cpu_count() or 1, max(1, len(jobs) // 8)) if (parallel and _pool_allowed()) else 1
    if workers > 1:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(workers) as pool:
            res = pool.map(_pair_job, jobs, chunksize=4)
    else:
        res = [_pair_job(j) for j in jobs]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


# ----------------------------------------------------------------------------- rank-0 extras
def _time_oracle(o, cfg, left, right, threads, budget_s, max_runs=16):
    """pairs/s of the C oracle at `threads` OpenMP threads: one run to size the sample, then up to max_runs within budget_s."""
    o.set_threads(threads)
    t0 = time.perf_counter()
    o.run(cfg, left, right)
    first = time.perf_counter() - t0
    n = max(1, min(max_runs, int(budget_s / max(first, 1e-3))))
    if n == 1:
        return 1.0 / first, 1
    t0 = time.perf_counter()
    for _ in range(n):
        o.run(cfg, left, right)
    return n / (time.perf_counter() - t0), n


def cpu_baseline(budget_s: float = 10.0):
    """The oracle (OpenMP build of oracle/stereo_oracle.c) timed on the host cores: a reported baseline
    only.  The reference ships no CPU path for this algorithm.  `value` is config C2 (the headline's
    workload); `configs` adds the other CPU figures BASELINE.md 2.1 / SURVEY 8(d) list: C1 through the NumPy restatement
    and the C port, C5 through the RGB entry, C4 (one iteration)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_lib
    import stereo_numpy
    import stereo_synthetic as syn
    o = oracle_lib.get(parallel=True)
    # the GPU box gives one GPU's job a 16-core share of the host (more threads only oversubscribe)
    cores = min(o.max_threads(), os.cpu_count() or 1, 16)
    cfg = oracle_lib.OracleConfig(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
    left, right, _ = syn.make_pair(H, W, D, K, 0)
    one_thread, _ = _time_oracle(o, cfg, left, right, 1, 0.0)
    rate, n = _time_oracle(o, cfg, left, right, cores, budget_s)
    configs = {}
    # C1 literally ("NumPy CPU path ... plumbing, no GPU"): the NumPy restatement, and the C port beside it
    c1 = oracle_lib.OracleConfig(height=240, width=320, downscale_factor=1, min_disparity=0, max_disparity=31)
    l1, r1, _ = syn.make_pair(240, 320, 32, 1, 0)
    t0 = time.perf_counter()
    stereo_numpy.run(c1, l1, r1)
    configs["C1 320x240 D=32 K=1, oracle/stereo_numpy.py"] = {"pairs_per_s": 1.0 / (time.perf_counter() - t0), "threads": 1, "runs": 1}
    for threads in (1, cores):
        v, k = _time_oracle(o, c1, l1, r1, threads, 1.0)
        configs[f"C1 320x240 D=32 K=1, C port, {threads} thread(s)"] = {"pairs_per_s": v, "threads": threads, "runs": k}
    c5 = oracle_lib.OracleConfig(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=191)
    l5, r5 = syn.random_rgb_pair(H, W, 192, K, 0)
    v, k = _time_oracle(o, c5, l5, r5, cores, 2.0)
    configs["C5 1242x375 D=192 K=2 RGB, C port"] = {"pairs_per_s": v, "threads": cores, "runs": k}
    c4 = oracle_lib.OracleConfig(height=2160, width=3840, downscale_factor=4, min_disparity=0, max_disparity=255)
    l4, r4, _ = syn.make_pair(2160, 3840, 256, 4, 0)
    v, k = _time_oracle(o, c4, l4, r4, cores, 0.0)
    configs["C4 3840x2160 D=256 K=4, C port"] = {"pairs_per_s": v, "threads": cores, "runs": k}
    o.set_threads(cores)
    return {"value": rate, "unit": "pairs/s", "cores": cores, "kind": "port", "value_1thread": one_thread,
            "sample": f"{n} x C2 pair (1242x375, D=128, K=2) through oracle/stereo_oracle.c "
                      f"(-O3 -mavx2 -fopenmp, {cores} threads; value_1thread: 1 pair, 1 thread); "
                      "the reference has no CPU implementation",
            "configs": configs}


def profile_record(suffix: str):
    """Latest committed profile summary profiles/rNN_<suffix> (the highest round number wins)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_" + suffix)))
    if not files:
        return None
    try:
        rec = json.load(open(files[-1]))
        rec["_file"] = "profiles/" + os.path.basename(files[-1])
        return rec
    except (OSError, ValueError):
        return None


def measured_traffic(kernel: str, pairs: int):
    """HBM bytes per launch of the dominant kernel from the rocprofv3 PMC passes committed under
    profiles/ (tools/pmc_traffic.py: separate --pmc FETCH_SIZE / WRITE_SIZE runs of this same
    command, gfx950 corrections per MI355X_MICROARCH.md).  (None, why) if no matching record exists."""
    rec = profile_record("traffic.json")
    if not rec:
        return None, "no profiles/rNN_traffic.json"
    k = rec.get("kernels", {}).get(kernel)
    if not k or rec.get("pairs_per_launch") != pairs or "hbm_bytes_per_launch" not in k:
        return None, f"{rec['_file']} holds no record for this kernel / batch"
    return k["hbm_bytes_per_launch"], ("committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command "
                                       f"({rec['_file']}: {rec.get('source', '?')}); not re-measured by this run")


def copy_bandwidth(torch) -> float:
    """On-device copy of 1 GiB (read + write counted), GB/s: the achievable-HBM yardstick of SURVEY 8(d)."""
    n = 1 << 28
    src = torch.empty(n, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(2):
        dst.copy_(src)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(5):
        dst.copy_(src)
    b.record()
    torch.cuda.synchronize()
    return 5 * 2 * n * 4 / (a.elapsed_time(b) * 1e-3) / 1e9


def event_median_us(torch, fn, iters: int, warm: int) -> float:
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2] * 1e3


def batch_rate(torch, engine, left, right, out, iters: int = 10) -> float:
    """pairs/s of `iters` back-to-back batch calls, submitted like the headline region (engine streams).  `out`: one
    tensor, or a list the calls take turns with -- calls that are in flight together (small calls alternate between the
    stream lanes) need outputs of their own, the engine orders calls that write the same memory."""
    outs = list(out) if isinstance(out, (list, tuple)) else [out]
    torch.cuda.synchronize()                      # engine-stream calls need complete inputs (they may come from device-side ops)
    t_settle = time.perf_counter()
    while True:                                   # at least 2 calls and 20 ms of load (clock ramp, see run_rank's region())
        for k in range(2):
            engine.compute_disparity_map_batch(left, right, outs[k % len(outs)], engine_streams=True)
        engine.join()
        torch.cuda.synchronize()
        if (time.perf_counter() - t_settle) * 1e3 >= 20.0:
            break
    t0 = time.perf_counter()
    for k in range(iters):
        engine.compute_disparity_map_batch(left, right, outs[k % len(outs)], engine_streams=True)
    engine.join()
    torch.cuda.synchronize()
    return left.shape[0] * iters / (time.perf_counter() - t0)


def run_configs(torch, cuda_depth, syn, device):
    """Every BASELINE configuration (and the reference's own defaults) on one GPU: single-call latency
    (median, HIP events) and batched throughput, device-resident inputs."""
    out = {}
    for name, h_, w_, k_, dmin, dmax, entry, batch in CONFIGS:
        cfg = cuda_depth.StereoMatchingConfiguration(height=h_, width=w_, downscale_factor=k_,
                                                     min_disparity=dmin, max_disparity=dmax)
        if entry == "rgb":
            l, r = syn.random_rgb_pair(h_, w_, dmax + 1, k_, 0, dmin=dmin)
        else:
            l, r, _ = syn.make_pair(h_, w_, dmax + 1, k_, 0, dmin=dmin)
        tl, tr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
        sm1 = cuda_depth.StereoMatching(cfg, device=device)
        one = (lambda: sm1.compute_disparity_map(tl, tr)) if entry == "rgb" else (lambda: sm1.compute_disparity_map_gray(tl, tr))
        lat = event_median_us(torch, one, 50 if h_ * w_ > 4e6 else 200, 5)
        # the same single-pair calls submitted to the stream lanes (an engine with two pair slots: consecutive calls
        # alternate between the lanes and run side by side) -- frames per second of a caller that pipelines its frames
        sm2 = cuda_depth.StereoMatching(cfg, max_batch=2, device=device)
        piped = batch_rate(torch, sm2, tl.unsqueeze(0), tr.unsqueeze(0), [torch.empty((1, h_, w_), device="cuda") for _ in range(2)],
                           50 if h_ * w_ > 4e6 else 200)
        del sm2
        smb = cuda_depth.StereoMatching(cfg, max_batch=batch, device=device)
        bl = tl.unsqueeze(0).repeat(batch, *([1] * tl.dim())).contiguous()
        br = tr.unsqueeze(0).repeat(batch, *([1] * tr.dim())).contiguous()
        ob = torch.empty((batch, h_, w_), device="cuda")
        pps = batch_rate(torch, smb, bl, br, ob, 5 if h_ * w_ > 1e6 else 20)
        b_alg = (28 if entry == "rgb" else 12) * h_ * w_
        out[name] = {"single_call_latency_us": lat, "single_calls_pipelined_per_s": piped, "batch": batch, "pairs_per_s": pps, "B_alg_bytes": b_alg,
                     "hbm_frac_of_8TBps": b_alg * pps / 8e12, "match_mode": smb.last_match_mode()}
        del sm1, smb, bl, br, ob
        torch.cuda.empty_cache()
    return out


# ----------------------------------------------------------------------------- one rank
def run_rank(args) -> None:
    rank, local_rank, world = rank_env()
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    import numpy as np
    import sharding

    if world > 1 and os.environ.get("SMX_BENCH_NO_PIN") != "1":
        # before anything touches the GPU: this rank's host threads (and the pinned staging buffers they fill) stay on
        # the cores next to its GPU; without topology information a contiguous 1/world slice
        try:
            os.sched_setaffinity(0, sharding.rank_cpu_slice(local_rank, world))
        except OSError:
            pass
    n = args.pairs
    extras = not args.quick
    # ---- host data first (process pool; nothing has touched the GPU yet)
    mine = sharding.shard_indices(n * world, world, rank)             # this rank's pairs of one step
    Lh, Rh = make_pairs("band", mine, parallel=extras)        # --quick (profiler runs): never a process pool
    c3_mine = sharding.shard_indices(C3_PAIRS, world, rank) if extras and not args.no_c3 else []
    c3_new = [i for i in c3_mine if i not in set(mine)]
    if c3_new:
        L3n, R3n = make_pairs("band", c3_new)
    if rank == 0 and extras and world == 1:
        Ln, Rn = make_pairs("noise", range(n))
        Ls, Rs = make_pairs("slanted", range(min(n, 16)))

    group = TimingGroup(rank, world)           # gloo rendezvous: works without a GPU (CPU dry run)
    import torch
    if not torch.cuda.is_available():
        group.barrier()
        group.close()
        raise SystemExit(f"bench.py rank {rank}/{world}: needs a GPU -- the HIP path has no CPU fallback")
    import cuda_depth
    import stereo_synthetic as syn
    shared_gpu = os.environ.get("SMX_BENCH_SHARE_GPU") == "1" and world > torch.cuda.device_count()
    if shared_gpu:
        # rehearsal of the N-rank path on a box with fewer GPUs: ranks share devices (the line says so)
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)

    left, right = torch.from_numpy(Lh).cuda(), torch.from_numpy(Rh).cuda()
    cfg = cuda_depth.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K,
                                                 min_disparity=0, max_disparity=D - 1)
    E = max(1, args.engines)
    if n % E:
        raise SystemExit(f"--pairs {n} must be a multiple of --engines {E}")
    per = n // E
    engines = [cuda_depth.StereoMatching(cfg, max_batch=per, match_mode=args.mode, device=local_rank) for _ in range(E)]
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(E - 1)]
    sm = engines[0]
    out = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
    SETTLE_MS = 40.0          # untimed load before each timed region (clock ramp, see region())
    PROFILED_STEPS = 3        # event brackets cost ~3 us each (10 per step = 3.4 % of a step): sample, do not bracket every step

    def region(on_engine, repeats=1):
        """`warmup` untimed steps, then `repeats` timed regions of exactly `steps` steps each (device sync + barrier on
        both sides of every one); ([elapsed seconds, MAX over ranks, per region], kernel profile of the last region)."""
        nprof = min(args.steps, PROFILED_STEPS)
        timed_step = [None]               # index of the next timed step; None while warming up / outside the last region

        def step():
            if timed_step[0] is not None:
                if timed_step[0] == args.steps - nprof:
                    sm.profile_begin(nprof)    # HIP events around every kernel of the LAST nprof steps (steady state), on the launch stream
                timed_step[0] += 1
            for i, (eng, st) in enumerate(zip(engines, streams)):
                with torch.cuda.stream(st):
                    eng.compute_disparity_map_batch(left[i * per:(i + 1) * per], right[i * per:(i + 1) * per],
                                                    out[i * per:(i + 1) * per], engine_streams=on_engine)

        def finish():                     # every step's output complete: join the engine's streams, then the device
            for eng, st in zip(engines, streams):
                with torch.cuda.stream(st):
                    eng.join()
            torch.cuda.synchronize()

        for _ in range(args.warmup):
            step()
        finish()
        # steady state: after an idle device the shader clock takes ~10 ms of load to come up (the first steps of a region
        # run 7 % slower: match_fast 0.68 vs 0.636 ms), so keep the device busy for SETTLE_MS before the timed steps
        t_settle = time.perf_counter()
        while (time.perf_counter() - t_settle) * 1e3 < SETTLE_MS:
            for _ in range(4):
                step()
            finish()
        runs = []
        for rep in range(repeats):
            if rep == repeats - 1:
                timed_step[0] = 0          # the event brackets go into the last region only
            runs.append(timed_steps(step, finish, group, args.steps, 0))
        return runs, sm.profile_end()

    # ---- the timed region (all ranks).  --submit engine: the calls go to the engine's own two stream lanes (the inputs
    #      are resident and complete), so consecutive steps pipeline; --submit stream: every call on the caller's stream
    pipelined = args.submit == "engine"
    runs, prof = region(pipelined, max(1, args.repeats))
    elapsed = sorted(runs)[len(runs) // 2]          # `value` is priced on the median region
    dumped = dump_outputs(torch, args.dump_outputs, out, mine, rank, world) if args.dump_outputs else None
    # ---- the same steps once more on the caller's stream: one launch per kernel and step, nothing beside it -- the
    #      per-kernel durations the roofline is priced on (on the lanes every launch shares the chip with the other lane's)
    prof_lanes, elapsed_serial = None, elapsed
    if pipelined and not args.no_serial_pass:
        prof_lanes = prof
        serial_runs, prof = region(False)
        elapsed_serial = serial_runs[0]
    mode_used = sm.last_match_mode()

    # ---- config C3: 512 distinct pairs over the `world` devices, first launch -> last sync, all ranks
    c3 = None
    if c3_mine:
        pos = {g: i for i, g in enumerate(mine)}
        newpos = {g: i for i, g in enumerate(c3_new)}
        L3 = np.stack([Lh[pos[g]] if g in pos else L3n[newpos[g]] for g in c3_mine])
        R3 = np.stack([Rh[pos[g]] if g in pos else R3n[newpos[g]] for g in c3_mine])
        c3 = run_c3(torch, group, sm, per, L3, R3, world)

    line = None
    if rank == 0:
        pairs = n * world * args.steps
        value = pairs / elapsed
        dominant = max((k for k in prof if prof[k][1] > 0), key=lambda k: prof[k][0])
        dom_ms, dom_launches = prof[dominant]
        achieved = (B_ALG_PER_PAIR * per) / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0   # per launch: `per` pairs
        traffic, traffic_source = measured_traffic(dominant, per)
        line = {
            "metric": "disparity maps/sec (stereo pairs/sec) at 1242x375 D=128",
            "value": value, "unit": "pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "settle_ms": SETTLE_MS,
            "value_runs": [round(pairs / t, 1) for t in runs],
            "value_runs_note": f"{len(runs)} timed regions of exactly {args.steps} steps each, back to back, every one bracketed by "
                               "device sync + barrier (MAX over ranks); `value` / `ms_per_step` are the median region",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"C2 shape 1242x375 gray f32, D=128, K=2, {n} distinct device-resident pairs per GPU "
                                   f"per step through the batch C ABI (= config C3 at 8 GPUs); match_mode={args.mode}; "
                                   + {"engine": "calls submitted to the engine's own two stream lanes (SMX_STREAM_ENGINE), joined "
                                                "and synchronised at the end of the timed region",
                                      "stream": "calls on the caller's stream"}[args.submit]
                                   + (f", {E} engines x {per} pairs on {E} streams" if E > 1 else ""),
                       "pairs_per_gpu_per_step": n,
                       "parallelism": f"independent pairs, pair i -> device i mod {world}; no collective, no RCCL "
                                      "(gloo barrier + MAX of the elapsed time only)"},
            **({"rehearsal": "SMX_BENCH_SHARE_GPU=1: ranks share GPUs -- not a scaling measurement"} if shared_gpu else {}),
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic, "traffic_source": traffic_source,
                         "kernel": dominant, "kernel_ms": dom_ms, "launches": dom_launches,
                         "algorithmic_bytes_per_launch": B_ALG_PER_PAIR * per,
                         "region": ("the timed region" if prof_lanes is None else
                                    f"a second region of the same {args.steps} steps on the caller's stream ({per} pairs per launch, "
                                    "nothing running beside it); the launches of the pipelined region are under `pipelined`"),
                         "events": f"HIP events around every kernel of the last {min(args.steps, PROFILED_STEPS)} steps of the region"},
            "kernel_ms": {k: round(v[0], 5) for k, v in prof.items() if v[1] > 0},
            "whole_path_hbm_frac": (B_ALG_PER_PAIR * value / world) / 1e9 / HBM_PEAK_GBPS,
            "match_mode_used": mode_used,
        }
        if prof_lanes is not None:
            lanes = sm.overlap_lanes(per)
            pd_ms = prof_lanes[dominant][0]
            pa = (B_ALG_PER_PAIR * per / lanes) / (pd_ms * 1e-3) / 1e9 if pd_ms > 0 else 0.0
            line["value_serial"] = n * world * args.steps / elapsed_serial
            line["roofline"]["pipelined"] = {
                "pairs_per_launch": per // lanes, "kernel_ms": pd_ms, "achieved": pa, "frac": pa / HBM_PEAK_GBPS,
                "kernel_ms_all": {k: round(v[0], 5) for k, v in prof_lanes.items() if v[1] > 0},
                "note": "per launch inside the timed region: two half-batch launches per kernel and step on two streams, each "
                        "sharing the chip with the other lane's launches (durations overlap and do not add up to the step)"}
        valu = profile_record("valu.json")
        geo = sm.match_geometry(per)           # of the launches the roofline is priced on
        line["roofline"]["valu"] = {
            "useful_fraction": geo.get("useful_fraction") if geo else None,
            "issue_busy": valu.get("issue_busy") if valu else None,
            "source": "useful_fraction: output (pixel, disparity) cells / marched cells of this launch's geometry "
                      "(smx_get_match_geometry); issue_busy: committed SQ counter pass (" + (valu["_file"] if valu else "none") + "), not re-measured",
        }
        if geo:
            line["roofline"]["match_geometry"] = geo
        line["bound_note"] = ("the HBM fraction is a ceiling indicator only: the match kernel is VALU-issue bound "
                              "(no MFMA: integer abs-diff reductions), see roofline.valu and NOTES.md section 3.4")
    if c3 is not None and line is not None:
        line["c3"] = c3
    if dumped is not None and line is not None:
        line["dump_outputs"] = dumped

    # With several ranks the others wait in the closing barrier while rank 0 runs its extra legs: keep those to the
    # latency and copy-bandwidth measurements (< 1 s); the content / RGB / per-configuration legs belong to the N = 1 run.
    lean = world > 1
    if rank == 0 and extras:
        if not args.no_latency:
            sm1 = cuda_depth.StereoMatching(cfg, max_batch=1, match_mode=args.mode, device=local_rank)
            line["single_pair_latency_us"] = event_median_us(
                torch, lambda: sm1.compute_disparity_map_gray(left[0], right[0]), 200, 20)
            line["single_pair_latency_note"] = "config C2: one gray pair per call, median of 200 HIP-event-timed calls after 20 warm-ups"
            del sm1
            sm2 = cuda_depth.StereoMatching(cfg, max_batch=2, match_mode=args.mode, device=local_rank)
            line["single_pair_calls_pipelined_per_s"] = batch_rate(torch, sm2, left[:1], right[:1], [out[:1], out[1:2]], 400)
            line["single_pair_calls_pipelined_note"] = ("the same one-pair calls submitted to the stream lanes (engine with two pair slots: "
                                                        "consecutive calls alternate between the lanes and between two output buffers), calls per second")
            del sm2
            # the transition call: one off-grid f32 gray pair after on-grid ones (the one-launch AUTO kernel's off-grid branch)
            sm3 = cuda_depth.StereoMatching(cfg, max_batch=1, match_mode=args.mode, device=local_rank)
            off = left[0] + 0.3
            trans = []
            for _ in range(7):                                  # every cycle: five on-grid calls (the hint settles), then the transition call
                for _ in range(5):
                    sm3.compute_disparity_map_gray(left[0], right[0])
                torch.cuda.synchronize()
                ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ea.record()
                sm3.compute_disparity_map_gray(off, right[0])
                eb.record()
                torch.cuda.synchronize()
                trans.append(ea.elapsed_time(eb) * 1e3)
            line["first_offgrid_call_us"] = sorted(trans[1:])[len(trans[1:]) // 2]
            line["first_offgrid_call_cold_us"] = trans[0]
            line["first_offgrid_call_note"] = ("config C2, f32 gray, AUTO: the first pair that is NOT on the exact 1/K^2 grid after five that are; "
                                               "median of six such transitions (HIP events); _cold_us: the very first one of the process, which also "
                                               "loads the code of the off-grid kernels; steady off-grid calls: tools/latency_offgrid.py")
            del sm3
        else:
            line["single_pair_latency_us"] = None
    if rank == 0 and extras and not lean:
        tn, tr_ = torch.from_numpy(Ln).cuda(), torch.from_numpy(Rn).cuda()
        line["value_noise"] = batch_rate(torch, sm, tn[:per], tr_[:per], out[:per])
        noise_dense = sm.route_info().get("fast_dense")
        ns = Ls.shape[0]
        reps = (per + ns - 1) // ns
        ts, tsr = torch.from_numpy(np.concatenate([Ls] * reps)[:per]).cuda(), torch.from_numpy(np.concatenate([Rs] * reps)[:per]).cuda()
        line["value_slanted"] = batch_rate(torch, sm, ts, tsr, out[:per])
        line["value_noise_route"] = {"fast_dense_after_noise": noise_dense, "fast_dense_after_slanted": sm.route_info().get("fast_dense"),
                                     "note": "1: the engine moved these batches to the form of the fast kernel that keeps the winner's "
                                             "neighbours during pass 1 (chosen from what the sparse second pass reported; same bits)"}
        if not args.no_latency:
            smc = cuda_depth.StereoMatching(cfg, max_batch=1, match_mode=args.mode, device=local_rank)
            line["single_pair_latency_by_content_us"] = {
                "scene-like": event_median_us(torch, lambda: smc.compute_disparity_map_gray(ts[0], tsr[0]), 200, 20),
                "noise": event_median_us(torch, lambda: smc.compute_disparity_map_gray(tn[0], tr_[0]), 200, 20),
                "note": "config C2, one f32 gray pair per call as single_pair_latency_us (which is the banded pair), other content"}
            del smc
        line["value_noise_note"] = (f"pairs/s, same {per}-pair C2 batch shape: value_noise = independent uniform-noise "
                                    "images (arg-max anywhere: worst case of the sparse neighbour pass), value_slanted = "
                                    "multi-scale texture over a ground-plane disparity ramp with two objects")
        del tn, tr_, ts, tsr
        # config C5 through the RGB entry: what cuda_stereo_matching_backend.py:13-17 calls
        nb = 32
        cfg5 = cuda_depth.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=191)
        sm5 = cuda_depth.StereoMatching(cfg5, max_batch=nb, device=local_rank)
        l5 = np.stack([syn.random_rgb_pair(H, W, 192, K, i)[0] for i in range(4)])
        r5 = np.stack([syn.random_rgb_pair(H, W, 192, K, i)[1] for i in range(4)])
        t5l, t5r = torch.from_numpy(np.concatenate([l5] * (nb // 4))).cuda(), torch.from_numpy(np.concatenate([r5] * (nb // 4))).cuda()
        line["value_rgb"] = batch_rate(torch, sm5, t5l, t5r, out[:nb], 5)
        line["value_rgb_note"] = (f"pairs/s, config C5 (1242x375, D=192, K=2) through the [3,H,W] f32 RGB entry, {nb} pairs per "
                                  f"call, B_alg = 28*H*W; match_mode={sm5.last_match_mode()}")
        del sm5, t5l, t5r
        real = real_scene_rates(torch, cuda_depth, out, local_rank)
        if real:
            line.update(real)
        if args.configs:
            line["configs"] = run_configs(torch, cuda_depth, syn, local_rank)
        if world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline()
    if rank == 0 and extras:
        bw = copy_bandwidth(torch)
        line["roofline"]["copy_bandwidth_GBps"] = bw
        line["roofline"]["frac_of_achievable"] = line["roofline"]["achieved"] / bw
    if rank == 0:
        print(json.dumps(line), file=getattr(args, "result_stream", sys.stdout), flush=True)
    group.barrier()
    group.close()


def dump_outputs(torch, directory, out, mine, rank, world):
    """--dump-outputs: what the timed path returned in its last step, the [n,H,W] float32 disparity maps of this rank's
    pairs, as DIR/disparity.npy (DIR/disparity_rank<r>.npy with several ranks).  A whole batch is larger than
    DUMP_BYTES, so the file holds a fixed sample of its pairs (seeded, in ascending order): with the same arguments
    the same pairs, built from the same inputs, in every run.  Returns the record rank 0 puts into the result line."""
    import numpy as np
    n = out.shape[0]
    per_pair = out[0].numel() * out.element_size()
    take = min(n, max(1, (DUMP_BYTES // world - 4096) // per_pair))
    idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=take, replace=False))
    maps = out.index_select(0, torch.from_numpy(idx).to(out.device)).cpu().numpy().astype(np.float32, copy=False)
    name = "disparity" if world == 1 else f"disparity_rank{rank}"
    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, name + ".npy"), maps)
    return {"dir": os.path.abspath(directory), "files": [name + ".npy"], "dtype": "float32", "shape": list(maps.shape),
            "pair_index": [int(mine[i]) for i in idx],
            "note": f"disparity maps of the last timed step, {take} of the {n} pairs of each rank (seed {DUMP_SEED}); "
                    "pair_index: global pair indices (rank 0's), inputs seeded by pair index"}


def real_scene_rates(torch, cuda_depth, out, device):
    """The one real pair the reference ships (src/python/data, cut to C2's shape: tests/golden/real/), at its
    calibrated disparity range 75..262: 64 gray pairs (the scene shifted by i columns, cyclically) through the
    f32 gray entry in AUTO mode, and 32 pairs through the uint8 RGB entry (the reference's own call)."""
    import numpy as np
    path = os.path.join(ROOT, "tests", "golden", "real", "real_crop_c2.npz")
    if not os.path.exists(path):
        return None
    z = np.load(path)
    l, r = z["left_rgb"], z["right_rgb"]
    vmin, vmax = (int(v) for v in z["disparity_range"])
    cfg = cuda_depth.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=vmin, max_disparity=vmax)
    n = 64
    sm = cuda_depth.StereoMatching(cfg, max_batch=n, device=device)
    gray = lambda x: np.rint(0.2989 * x[0] + 0.5870 * x[1] + 0.1140 * x[2]).astype(np.float32)   # noqa: E731
    gl = torch.from_numpy(np.stack([np.roll(gray(l), i, axis=1) for i in range(n)])).cuda()
    gr = torch.from_numpy(np.stack([np.roll(gray(r), i, axis=1) for i in range(n)])).cuda()
    res = {"value_real": batch_rate(torch, sm, gl, gr, out[:n])}
    del gl, gr
    nb = 32
    tl = torch.from_numpy(np.stack([np.roll(l, i, axis=2) for i in range(nb)])).cuda()
    tr = torch.from_numpy(np.stack([np.roll(r, i, axis=2) for i in range(nb)])).cuda()
    res["value_real_rgb"] = batch_rate(torch, sm, tl, tr, out[:nb], 5)
    ri = sm.route_info()
    res["value_real_rgb_route"] = {"route": "dense exact-order" if ri["route_dense"] else "filtered exact-order",
                                   "candidate_density": round(ri["candidate_density"], 3),
                                   "note": "chosen by the engine from the density its filtered launches reported (exact_filter = 0)"}
    res["value_real_note"] = (f"pairs/s on the reference's own sample pair (real texture), 1242x375 crop at full resolution, calibrated "
                              f"disparity range {vmin}..{vmax}, K=2: value_real = {n} integer-valued gray pairs per call (f32 gray entry, AUTO), "
                              f"value_real_rgb = {nb} uint8 RGB pairs per call (exact summation order; route: value_real_rgb_route)")
    return res


def run_c3(torch, group, sm, max_batch, L3, R3, world):
    """BASELINE config 3 / SURVEY 8(d)-C3: this rank's share of 512 distinct pairs, (a) device-resident
    f32, (b) uint8 from pinned host memory with the uploads on a second stream.  Wall-clock from the
    first launch to the last stream sync, MAX over ranks."""
    import sharding
    n = L3.shape[0]
    calls = sharding.calls_for_shard(n, max_batch)
    left, right = torch.from_numpy(L3).cuda(), torch.from_numpy(R3).cuda()
    out = torch.empty((n, H, W), dtype=torch.float32, device="cuda")

    def resident():
        for c in calls:
            sm.compute_disparity_map_batch(left[c.start:c.stop], right[c.start:c.stop], out[c.start:c.stop],
                                           engine_streams=True)       # resident and complete: calls pipeline

    def joined_sync():
        sm.join()
        torch.cuda.synchronize()

    t_res = timed_steps(resident, joined_sync, group, 1, 3)       # 3 untimed passes (~20 ms) first: clock ramp
    del left, right
    # (b) uint8 over PCIe: double-buffered staging, copies on their own stream, compute waits on events
    l8 = torch.from_numpy(L3.astype("uint8")).pin_memory()
    r8 = torch.from_numpy(R3.astype("uint8")).pin_memory()
    chunk = min(32, max_batch)
    chunks = sharding.calls_for_shard(n, chunk)
    stage = [(torch.empty((chunk, H, W), dtype=torch.uint8, device="cuda"),
              torch.empty((chunk, H, W), dtype=torch.uint8, device="cuda")) for _ in range(2)]
    copy_stream = torch.cuda.Stream()
    main = torch.cuda.current_stream()

    def over_pcie():
        done = [None, None]
        for k, c in enumerate(chunks):
            m = c.stop - c.start
            sl, sr = stage[k % 2]
            with torch.cuda.stream(copy_stream):
                if done[k % 2] is not None:
                    copy_stream.wait_event(done[k % 2])       # the staging buffer is free again
                sl[:m].copy_(l8[c.start:c.stop], non_blocking=True)
                sr[:m].copy_(r8[c.start:c.stop], non_blocking=True)
                up = torch.cuda.Event()
                up.record(copy_stream)
            main.wait_event(up)
            sm.compute_disparity_map_batch(sl[:m], sr[:m], out[c.start:c.stop])
            done[k % 2] = torch.cuda.Event()
            done[k % 2].record(main)

    t_pcie = timed_steps(over_pcie, torch.cuda.synchronize, group, 1, 2)
    return {"pairs": C3_PAIRS, "n_gpus": world, "pairs_this_rank": n,
            "pairs_per_s": C3_PAIRS / t_res, "pairs_per_s_incl_h2d_u8": C3_PAIRS / t_pcie,
            "note": "512 distinct pairs (seed 1234+i), pair i -> device i mod N, calls of <= "
                    f"{max_batch} pairs; wall-clock first launch -> last sync, MAX over ranks; incl_h2d_u8: uint8 gray "
                    f"inputs from pinned host memory in chunks of {chunk} pairs on a copy stream (never part of `value`)"}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=PAIRS_PER_GPU, help="pairs per GPU per step")
    ap.add_argument("--mode", default="auto", choices=["auto", "exact_order", "fast_grid"])
    ap.add_argument("--engines", type=int, default=1,
                    help="engines (each on its own HIP stream, an equal share of the step's pairs) per GPU; 2 lets the "
                         "tail of one engine's kernels overlap the other's but blurs per-kernel durations")
    ap.add_argument("--submit", default="engine", choices=["engine", "stream"],
                    help="engine: batch calls go to the engine's own two stream lanes (SMX_STREAM_ENGINE) and consecutive "
                         "steps pipeline; stream: every call on the caller's stream, one launch per kernel and step (what "
                         "the roofline is priced on and the profiler runs use)")
    ap.add_argument("--no-serial-pass", action="store_true",
                    help="skip the second region (caller's stream) that prices the roofline; profiler runs of the pipelined region")
    ap.add_argument("--quick", action="store_true",
                    help="timed region only (no latency / noise / rgb / c3 / copy-bandwidth / cpu legs): for rocprofv3 runs")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-latency", action="store_true",
                    help="skip the single-pair latency leg (a rocprofv3 run then sees batch launches only)")
    ap.add_argument("--no-c3", action="store_true")
    ap.add_argument("--repeats", type=int, default=5,
                    help="timed regions of exactly --steps steps each; `value` is their median, `value_runs` lists all")
    ap.add_argument("--no-configs", dest="configs", action="store_false",
                    help="skip the per-configuration leg (every BASELINE configuration + the reference's default "
                         "configuration: single-call latency and batched throughput, line['configs']); ~3 s")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write the disparity maps the timed path returned in its last step to "
                         "DIR/disparity.npy (float32, a fixed seeded sample of the batch's pairs, at most 64 MB in all) "
                         "so that two builds can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    # stdout carries the ONE JSON line and nothing else: libraries that write to file descriptor 1
    # (gloo's "Rank 0 is connected to ..." for instance) are sent to stderr
    sys.stdout.flush()
    args.result_stream = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    run_rank(args)


if __name__ == "__main__":
    main()
