#!/usr/bin/env python3
"""Cost of writing one TSDF volume's state into another (smx_tsdf_merge), on one caller stream:
    python tools/tsdf_merge_throughput.py [--repeats 7] [--iters 10]
The volume is the 512x256x512 colour volume of 0.1 m voxels of tools/tsdf_throughput.py (805 MB of state), filled by its
8 maps.  The box is what shift((0, 0, 32), spill=True) cuts out: the 33 layers z = 0..32 over the whole cross-section.
Timed, each captured `iters` times into one HIP graph and replayed `repeats` times after a warm-up (median, min, max per
call); what a merge changed is put back before every replay, outside the clock:
  window   the yardstick: smx_tsdf_window cutting that box out of the volume (reads and writes 12 bytes per voxel)
  fill     restoring the box's 32 owned layers into empty layers of the volume, as TSDFSpillStore does after the shift
           back (each of the graph's merges has its own empty slab of 32 layers, so every one of them does the work)
  average  merging the box into the layers it was cut from, where both are measured
  average_mid_volume  the same with a box of the same size from the middle of the volume, where far more is measured
           (reported beside the two; the aim is stated for the spill box)
Counted traffic of a merge, per voxel of the region that has a destination: 4 bytes (the source's weight); where the
source is measured 8 more of the source and 4 of the destination's weight; where the voxel is written a 12-byte store;
in average mode 8 more of destination reads where the source is measured.  The aim for each merge: no more than the
window's time times the ratio of counted traffic (`aim_us`); `aim_met` says whether both meet it.  `one_voxel_rows` is
the floor under any of them: a merge of the same rows, one voxel wide -- the launch and a wave per row without traffic.
Also: TSDFSpillStore.shift there and back -- (0, 0, 32), then (0, 0, -32), which restores the box -- against two plain
shifts, as host time with a synchronisation after each pair.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np, torch, cuda_depth   # noqa: E401,E402
from cuda_depth import _native           # noqa: E402
import tsdf_throughput as base           # noqa: E402

H, W, FOCAL, BASELINE = base.H, base.W, base.FOCAL, base.BASELINE
DIMS, VS, ORIGIN = base.DIMS, base.VS, base.ORIGIN
LAYERS, MARGIN = 32, 1
BOX = (DIMS[0], DIMS[1], LAYERS + MARGIN)
OWNED = (DIMS[0], DIMS[1], LAYERS)


def time_replays(fn, reset, iters, repeats, warmup):
    """fn(i) for i < iters captured into one graph; reset() runs before every replay, outside the clock."""
    reset()
    fn(0)
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    reset()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        for i in range(iters):
            fn(i)
    per_call = []
    for r in range(warmup + repeats):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        if r >= warmup:
            per_call.append(a.elapsed_time(b) * 1e3 / iters)
    return base.stats(per_call)


def merge_call(dst, box, z0, region_dims, mode):
    lib = _native.LIB
    rc = lib.smx_tsdf_merge(dst.device.index, *dst.dims, dst.tsdf.data_ptr(), dst.weight.data_ptr(), dst.color.data_ptr(),
                            *box.dims, box.tsdf.data_ptr(), box.weight.data_ptr(), box.color.data_ptr(), 0, 0, z0, 0, 0, 0,
                            *region_dims, _native.TSDF_MERGE_MODES[mode], dst.max_weight,
                            torch.cuda.current_stream().cuda_stream)
    _native.check(rc)


def counted_bytes(src_w, dst_w, mode):
    """The counted traffic of one merge of the region whose source weights are src_w onto dst_w (same shape)."""
    pairs = src_w.numel()
    measured = src_w > 0
    written = measured if mode == "average" else measured & ~(dst_w > 0)
    m, w = int(measured.sum().item()), int(written.sum().item())
    return 4 * pairs + 12 * m + 12 * w + (8 * m if mode == "average" else 0), m / pairs, w / pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not 1 <= args.iters <= DIMS[2] // LAYERS - 1:
        ap.error(f"--iters must be in 1..{DIMS[2] // LAYERS - 1}: each merge of the fill case has its own slab of the volume")
    rng = np.random.default_rng(0)
    n = 8
    z = rng.uniform(3.0, 50.0, (n, H, W))
    d = (FOCAL * BASELINE / z).astype(np.float32)
    d[rng.random((n, H, W)) < 0.10] = -1.0
    disp = torch.from_numpy(d).cuda()
    rgb = torch.from_numpy(rng.integers(0, 256, (n, 3, H, W)).astype(np.uint8)).cuda()
    Q = cuda_depth.reprojection_matrix(FOCAL, W / 2.0, H / 2.0, BASELINE)
    c2w = np.stack([np.eye(4)] * n)
    c2w[:, 2, 3] = 0.5 * np.arange(n)
    w2c = torch.from_numpy(cuda_depth.world_to_camera_poses(c2w)).cuda()
    vol = cuda_depth.TSDFVolume(DIMS, VS, ORIGIN, truncation=0.3)
    base.Integrator(vol, disp, rgb, w2c, Q)()
    torch.cuda.synchronize()
    voxels = DIMS[0] * DIMS[1] * DIMS[2]
    result = {"volume": "512x256x512 @ 0.1 m, u8 RGB", "box": f"{BOX[0]}x{BOX[1]}x{BOX[2]}",
              "measured_voxel_fraction": round(int(vol.weight.count_nonzero().item()) / voxels, 3),
              "stream": "one caller stream", "repeats": args.repeats, "iters": args.iters,
              "gpu": torch.cuda.get_device_name(0)}
    box = vol.window((0, 0, 0), BOX)
    box_voxels = BOX[0] * BOX[1] * BOX[2]

    # the yardstick: the windowed copy that cuts the box out
    out = vol._state_like(BOX)
    t = time_replays(lambda i: vol._window_into((0, 0, 0), BOX, *out), lambda: None, args.iters, args.repeats, args.warmup)
    window_bytes = 24 * box_voxels
    t["mbytes"] = round(window_bytes / 1e6, 1)
    t["tb_per_s"] = round(window_bytes / (t["us_median"] * 1e-6) / 1e12, 3)
    result["window"] = t
    del out

    # fill: slab i of the destination, layers [32 i, 32 i + 32), is empty before every replay
    dst = vol.window((0, 0, 0), DIMS)
    slabs = LAYERS * args.iters

    def empty_slabs():
        for a in (dst.tsdf, dst.weight, dst.color):
            a[:slabs].zero_()

    t = time_replays(lambda i: merge_call(dst, box, LAYERS * i, OWNED, "fill"), empty_slabs, args.iters, args.repeats,
                     args.warmup)
    nbytes, measured, written = counted_bytes(box.weight[:LAYERS], torch.zeros_like(box.weight[:LAYERS]), "fill")
    result["fill"] = dict(t, mbytes=round(nbytes / 1e6, 1), tb_per_s=round(nbytes / (t["us_median"] * 1e-6) / 1e12, 3),
                          source_measured=round(measured, 3), written=round(written, 3),
                          aim_us=round(result["window"]["us_median"] * nbytes / window_bytes, 2))

    # average: the box into the layers it was cut from; they are put back before every replay
    # (the graph's later merges find the earlier ones' means there: the same traffic, since a mean is stored whenever
    # the source is measured)
    dst = vol.window((0, 0, 0), DIMS)
    first = tuple(a[:BOX[2]].clone() for a in (dst.tsdf, dst.weight, dst.color))

    def put_back():
        for a, b in zip((dst.tsdf, dst.weight, dst.color), first):
            a[:BOX[2]].copy_(b)

    t = time_replays(lambda i: merge_call(dst, box, 0, BOX, "average"), put_back, args.iters, args.repeats, args.warmup)
    nbytes, measured, written = counted_bytes(box.weight, first[1], "average")
    result["average"] = dict(t, mbytes=round(nbytes / 1e6, 1), tb_per_s=round(nbytes / (t["us_median"] * 1e-6) / 1e12, 3),
                             source_measured=round(measured, 3), written=round(written, 3),
                             aim_us=round(result["window"]["us_median"] * nbytes / window_bytes, 2))
    # the same merge where the volume is full: a box of the same size from the middle of the volume into its own layers
    mid = (DIMS[2] - BOX[2]) // 2
    dense = vol.window((0, 0, mid), BOX)
    first = tuple(a[mid:mid + BOX[2]].clone() for a in (dst.tsdf, dst.weight, dst.color))

    def put_back_mid():
        for a, b in zip((dst.tsdf, dst.weight, dst.color), first):
            a[mid:mid + BOX[2]].copy_(b)

    t = time_replays(lambda i: merge_call(dst, dense, mid, BOX, "average"), put_back_mid, args.iters, args.repeats,
                     args.warmup)
    nbytes, measured, written = counted_bytes(dense.weight, first[1], "average")
    result["average_mid_volume"] = dict(t, mbytes=round(nbytes / 1e6, 1),
                                        tb_per_s=round(nbytes / (t["us_median"] * 1e-6) / 1e12, 3),
                                        source_measured=round(measured, 3), written=round(written, 3),
                                        aim_us=round(result["window"]["us_median"] * nbytes / window_bytes, 2))
    del dense

    # the floor: the same rows, one voxel wide -- the launch and a wave per row without the traffic
    t = time_replays(lambda i: merge_call(dst, box, 0, (1, BOX[1], BOX[2]), "average"), lambda: None, args.iters,
                     args.repeats, args.warmup)
    result["one_voxel_rows"] = t
    result["aim"] = "each merge in no more than the window's time x the ratio of counted traffic (aim_us)"
    result["aim_met"] = all(result[k]["us_median"] <= result[k]["aim_us"] for k in ("fill", "average"))
    del dst, first, box
    torch.cuda.empty_cache()

    # the store there and back against two plain shifts: host time, a synchronisation per pair
    def pair_ms(step):
        per = []
        for r in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step((0, 0, LAYERS))
            step((0, 0, -LAYERS))
            torch.cuda.synchronize()
            if r >= args.warmup:
                per.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(per)), 3)

    store = cuda_depth.TSDFSpillStore()
    restored = []
    plain = pair_ms(lambda d: vol.shift(d))
    vol = cuda_depth.TSDFVolume(DIMS, VS, ORIGIN, truncation=0.3)    # the plain pairs emptied the first 32 layers
    base.Integrator(vol, disp, rgb, w2c, Q)()
    through = pair_ms(lambda d: restored.append(store.shift(vol, d)[1]))
    result["there_and_back"] = {"plain_shifts_ms": plain, "store_shifts_ms": through,
                                "store_over_plain": round(through / plain, 3), "restored_per_pair": sum(restored) / (len(restored) / 2),
                                "entries_left": len(store)}
    torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
