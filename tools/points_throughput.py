#!/usr/bin/env python3
"""Cost of metric 3D points and voxel downsampling at C2 (1242x375) with KITTI-like intrinsics (f = 721.5 px,
B = 0.54 m), on one caller stream:
    python tools/points_throughput.py [--repeats 7] [--iters 20]
Synthetic maps: disparities uniform in 1..96 px with 10 % invalid pixels, a u8 RGB left frame.  Times
smx_reproject_points (cuda_depth.reproject_to_3d_batched, no pixel indices) of 1 and 32 maps, without and with colour,
and smx_voxel_downsample (cuda_depth.voxel_downsample_batched, with colour) of the 32 maps' points at 0.05, 0.1 and
0.2 m.  Each timed call is captured `iters` times into one HIP graph (no host overhead in the numbers), replayed after a
warm-up, `repeats` times: the median and the spread (min, max) of the time per call.  The yardstick is the LR call of
32 pairs (f32 gray, 128 disparities, K = 2) timed the same way but eagerly.  Bytes counted for the reprojection: the
map read twice (count and scatter passes), the points written, and with colour the three planes read and the colours
written; TB/s = those bytes over the median time.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd")]
import numpy as np, torch, cuda_depth   # noqa: E401,E402

H, W, D, K = 375, 1242, 128, 2
FOCAL, BASELINE = 721.5, 0.54


def stats(per_call):
    per_call = sorted(per_call)
    return {"us_median": round(per_call[len(per_call) // 2], 2), "us_min": round(per_call[0], 2),
            "us_max": round(per_call[-1], 2)}


def time_graph(fn, iters, repeats, warmup):
    """fn captured `iters` times into one graph; the time per call of its replays."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.graph(g, stream=s):
        for _ in range(iters):
            fn()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        per_call.append(a.elapsed_time(b) * 1e3 / iters)
    return stats(per_call)


def time_eager(fn, iters, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        per_call.append(a.elapsed_time(b) * 1e3 / iters)
    return stats(per_call)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    n_max = 32
    d = rng.uniform(1.0, 96.0, (n_max, H, W)).astype(np.float32)
    d[rng.random((n_max, H, W)) < 0.10] = -1.0
    disp = torch.from_numpy(d).cuda()
    rgb = torch.from_numpy(rng.integers(0, 256, (n_max, 3, H, W)).astype(np.uint8)).cuda()
    Q = cuda_depth.reprojection_matrix(FOCAL, W / 2.0, H / 2.0, BASELINE)
    result = {"config": f"C2 {W}x{H}", "stream": "one caller stream", "f": FOCAL, "baseline_m": BASELINE,
              "invalid_fraction": 0.1, "repeats": args.repeats, "iters": args.iters, "gpu": torch.cuda.get_device_name(0)}
    _, _, _, off, _ = cuda_depth.reproject_to_3d_batched(disp, Q, indices=False)
    points_per_map = float(off[-1].item()) / n_max
    result["points_per_map"] = round(points_per_map)
    for n in (1, 32):
        for name, img in (("no_colour", None), ("rgb_u8", rgb)):
            dd, ii = disp[:n], None if img is None else img[:n]
            t = time_graph(lambda: cuda_depth.reproject_to_3d_batched(dd, Q, image=ii, indices=False), args.iters,
                           args.repeats, args.warmup)
            pts = points_per_map * n
            nbytes = 2 * 4 * n * H * W + 12 * pts + (0 if img is None else 3 * n * H * W + 3 * pts)
            t["mbytes"] = round(nbytes / 1e6, 1)
            t["tb_per_s"] = round(nbytes / (t["us_median"] * 1e-6) / 1e12, 3)
            result[f"reproject_n{n}_{name}"] = t
    pts, cols, _, off, _ = cuda_depth.reproject_to_3d_batched(disp, Q, image=rgb, indices=False)
    for vs in (0.05, 0.1, 0.2):
        t = time_graph(lambda: cuda_depth.voxel_downsample_batched(pts, off, vs, colors=cols), args.iters,
                       args.repeats, args.warmup)
        _, _, _, vo, dr = cuda_depth.voxel_downsample_batched(pts, off, vs, colors=cols)
        t["voxels"] = int(vo[-1].item())
        result[f"voxel_n32_{vs}m"] = t
    cfg = cuda_depth.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=0,
                                                 max_disparity=D - 1)
    sm = cuda_depth.StereoMatching(cfg, max_batch=2 * n_max)
    gl = torch.from_numpy(rng.integers(0, 256, (n_max, H, W)).astype(np.float32)).cuda()
    gr = torch.roll(gl, -8, dims=2).contiguous()
    result["lr_n32"] = time_eager(lambda: sm.compute_disparity_map_batch_lr(gl, gr), max(2, args.iters // 4),
                                  args.repeats, args.warmup)
    result["voxel_0.1m_over_lr_n32"] = round(result["voxel_n32_0.1m"]["us_median"] / result["lr_n32"]["us_median"], 3)
    torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
