#!/usr/bin/env python3
"""Cost of moving a TSDF volume with the camera (TSDFVolume.shift: one smx_tsdf_window launch into the spare state), on
one caller stream:
    python tools/tsdf_shift_throughput.py [--repeats 7] [--iters 10] [--no-sequence]
The volume is the 512x256x512 colour volume of 0.1 m voxels of tools/tsdf_throughput.py (805 MB of state), filled by its
8 maps.  Timed: shift((0, 0, 32)), shift((32, 0, 0)), shift((5, -3, 32)) and shift((0, 0, 32), spill=True) (which also
cuts out the 33 leaving layers as a volume of its own).  Each is captured `iters` times into one HIP graph (no host
overhead in the numbers), replayed after a warm-up, `repeats` times: the median and the spread (min, max) per call.
Bytes counted for a shift: the staying part of the three arrays read and the whole of them written; for the spill the
box read and written on top.
The yardstick, in the same run and timed the same way, is torch's copy_ of the same three state tensors into
preallocated ones, which reads and writes all of them.  A shift reads less -- it skips what leaves and only writes
what enters -- so the aim is a shift in no more time than that copy: `ratio` per case is shift / copy, and aim_met says
whether every plain shift is <= 1 (the spill case does more than a shift and is reported beside it).
Sequence: the per-frame time of DepthEstimationPipeline.process (matching replaced by the analytic scene's exact maps,
32 C2 frames 0.33 m apart along +z from the volume's centre, the caller's poses, the same volume and the default
follow threshold of 32 voxels) with and without follow_camera: host time with a synchronisation per frame, the mean,
the median and the slowest frame (a frame that shifts).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np, torch, cuda_depth   # noqa: E401,E402
import tsdf_ref                          # noqa: E402
import tsdf_throughput as base           # noqa: E402

H, W, FOCAL, BASELINE = base.H, base.W, base.FOCAL, base.BASELINE
DIMS, VS, ORIGIN = base.DIMS, base.VS, base.ORIGIN
SHIFTS = (("shift_z32", (0, 0, 32), False), ("shift_x32", (32, 0, 0), False), ("shift_5_-3_32", (5, -3, 32), False),
          ("shift_z32_spill", (0, 0, 32), True))


def shift_bytes(d, spill, colour=True):
    """(read, written) bytes of one shift: the voxels that stay are read, every voxel is written; a spill box (one per
    moved axis, margin 1) is read and written once more."""
    per = 12 if colour else 8
    stay = 1
    for n, c in zip(DIMS, d):
        stay *= max(0, n - abs(c))
    read, written = stay * per, DIMS[0] * DIMS[1] * DIMS[2] * per
    if spill:
        for _, (bx, by, bz) in cuda_depth.tsdf_spill_boxes(DIMS, d, 1):
            read, written = read + bx * by * bz * per, written + bx * by * bz * per
    return read, written


def sequence_time(frames=32, step=0.33):
    """Mean host time per process() call over the analytic sequence, without and with follow_camera."""
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    scene = tsdf_ref.Scene(ground_y=1.65, boxes=[((-3.0, -0.2, 8.0 + 6.0 * k), (-1.0, 1.65, 10.0 + 6.0 * k)) for k in range(4)] +
                           [((1.0, -0.5, 11.0 + 6.0 * k), (3.5, 1.65, 13.0 + 6.0 * k)) for k in range(4)])
    Q = cuda_depth.reprojection_matrix(FOCAL, W / 2.0, H / 2.0, BASELINE)
    poses = np.stack([np.eye(4)] * frames)
    poses[:, 2, 3] = 25.6 + step * np.arange(frames)                  # from the volume's centre along +z
    maps = [torch.from_numpy(scene.render(p, H, W, FOCAL, W / 2.0, H / 2.0, BASELINE)).cuda() for p in poses]
    image = torch.zeros((3, H, W), dtype=torch.uint8, device="cuda")
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=0, max_disparity=base.D - 1)
    out = {"frames": frames, "step_m": step}
    for name, follow in (("fixed", False), ("follow", True)):
        vol = cuda_depth.TSDFVolume(DIMS, VS, ORIGIN, truncation=0.3)
        extra = dict(follow_camera=True) if follow else {}            # the default threshold: 32 voxels, 3.2 m
        pipe = DepthEstimationPipeline(cfg, reprojection_matrix=Q, tsdf_volume=vol, point_cloud_depth_range=(0.5, 50.0),
                                       **extra)
        feed = iter(maps + maps)
        pipe._stereo_matching.process = lambda left, right: next(feed)
        if follow:                                                    # the spare exists before the clock starts
            vol.shift((0, 0, 1))
            vol.shift((0, 0, -1))
        pipe.process(image, image, camera_pose=poses[0])              # warm-up
        torch.cuda.synchronize()
        per, shifts = [], 0
        for p in poses:
            t0 = time.perf_counter()
            res = pipe.process(image, image, camera_pose=p)
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) * 1e3)
            shifts += res.volume_shift != (0, 0, 0)
        out[name] = {"ms_per_frame_mean": round(float(np.mean(per)), 3), "ms_per_frame_median": round(float(np.median(per)), 3),
                     "ms_per_frame_max": round(float(np.max(per)), 3), "shifts": shifts}
        del pipe, vol
        torch.cuda.empty_cache()
    out["follow_over_fixed"] = round(out["follow"]["ms_per_frame_mean"] / out["fixed"]["ms_per_frame_mean"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-sequence", action="store_true", help="the shift cases and the yardstick only")
    args = ap.parse_args()
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
    result = {"volume": "512x256x512 @ 0.1 m, u8 RGB", "state_mbytes": round(DIMS[0] * DIMS[1] * DIMS[2] * 12 / 1e6, 1),
              "measured_voxel_fraction": round(int(vol.weight.count_nonzero().item()) / (DIMS[0] * DIMS[1] * DIMS[2]), 3),
              "stream": "one caller stream", "repeats": args.repeats, "iters": args.iters,
              "gpu": torch.cuda.get_device_name(0)}
    src = (vol.tsdf, vol.weight, vol.color)
    dst = tuple(torch.empty_like(t) for t in src)
    t = base.time_graph(lambda: [b.copy_(a) for a, b in zip(src, dst)], args.iters, args.repeats, args.warmup)
    nbytes = 2 * DIMS[0] * DIMS[1] * DIMS[2] * 12
    t["mbytes"] = round(nbytes / 1e6, 1)
    t["tb_per_s"] = round(nbytes / (t["us_median"] * 1e-6) / 1e12, 3)
    result["torch_copy"] = t
    del dst
    torch.cuda.empty_cache()
    for name, step, spill in SHIFTS:
        t = base.time_graph(lambda: vol.shift(step, spill=spill), args.iters, args.repeats, args.warmup)
        read, written = shift_bytes(step, spill)
        t["mbytes"] = round((read + written) / 1e6, 1)
        t["tb_per_s"] = round((read + written) / (t["us_median"] * 1e-6) / 1e12, 3)
        t["ratio"] = round(t["us_median"] / result["torch_copy"]["us_median"], 3)
        result[name] = t
    result["aim"] = "every plain shift in no more time than torch's copy_ of the state (ratio <= 1)"
    result["aim_met"] = all(result[name]["ratio"] <= 1.0 for name, _, spill in SHIFTS if not spill)
    del vol
    torch.cuda.empty_cache()
    if not args.no_sequence:
        result["sequence"] = sequence_time()
    torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
