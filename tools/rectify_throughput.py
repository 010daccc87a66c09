#!/usr/bin/env python3
"""Cost of rectifying raw stereo frames (smx_remap_pairs) at KITTI raw sizes, on one caller stream:
    python tools/rectify_throughput.py [--repeats 7] [--iters 20]
Input: RGB uint8 pairs of 1392x512 raw frames, rectified to 1242x375 through the maps of a mildly distorted, rotated
synthetic rig (cuda_depth.rectification_map + quantize_map), n = 1, 8 and 64 pairs per call.  The plain 64-pair match
call of the rectified batch (C2, 128 disparities, RGB uint8 entry; random raw content, so the engine takes its exact
route) and a 64-pair gray f32 call of synthetic pairs (bench.py's flagship content and route) are timed in the same
process, as the yardsticks.
Device events around `iters` back-to-back calls after a warm-up, `repeats` times; prints one JSON line with the median
and spread (min, max) of the time per call, the bytes each call moves (computed from the shapes: raw frames read once,
rectified frames written, both maps read once) and that over the median time.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run: the k_remap rows."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd")]
import numpy as np, torch, cuda_depth, stereo_synthetic as syn   # noqa: E401,E402

HI, WI, HO, WO, C = 512, 1392, 375, 1242, 3
D, K = 128, 2


def time_calls(fn, iters, repeats, warmup):
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
        per_call.append(a.elapsed_time(b) * 1e3 / iters)          # us
    per_call.sort()
    return {"us_median": round(per_call[len(per_call) // 2], 2), "us_min": round(per_call[0], 2),
            "us_max": round(per_call[-1], 2)}


def rig(k):
    """(K, dist, R, P) of camera k of a KITTI-like raw rig."""
    a = (0.004, -0.006, 0.003) if k == 0 else (-0.003, 0.005, -0.002)
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    R = (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
         np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))
    Kc = np.array([[960.0, 0.0, 696.0 + k], [0.0, 960.0, 224.0 - k], [0.0, 0.0, 1.0]])
    P = np.array([[720.0, 0.0, 609.5], [0.0, 720.0, 172.8], [0.0, 0.0, 1.0]])
    return Kc, np.array([-0.37, 0.2, 1e-3, 4e-4, -0.07]), R, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rectify_throughput needs a GPU")
    rect = cuda_depth.StereoRectification.from_calibration(rig(0), rig(1), (HI, WI), (HO, WO))
    gen = torch.Generator(device="cuda").manual_seed(0)
    raw_l = torch.randint(0, 256, (64, C, HI, WI), dtype=torch.uint8, device="cuda", generator=gen)
    raw_r = torch.randint(0, 256, (64, C, HI, WI), dtype=torch.uint8, device="cuda", generator=gen)
    out = (torch.empty((64, C, HO, WO), dtype=torch.uint8, device="cuda"),
           torch.empty((64, C, HO, WO), dtype=torch.uint8, device="cuda"))
    result = {"config": f"raw {WI}x{HI} -> {WO}x{HO}, RGB uint8 pairs", "stream": "one caller stream",
              "left_valid_fraction": round(float(rect.left_valid.float().mean()), 4), "repeats": args.repeats,
              "iters": args.iters, "gpu": torch.cuda.get_device_name(0)}
    for n in (1, 8, 64):
        src_l, src_r, dst = raw_l[:n], raw_r[:n], (out[0][:n], out[1][:n])
        t = time_calls(lambda: rect.rectify(src_l, src_r, out=dst), args.iters, args.repeats, args.warmup)
        moved = 2 * n * C * (HI * WI + HO * WO) + 2 * HO * WO * 8
        t["bytes_per_call"] = moved
        t["GB_per_s"] = round(moved / (t["us_median"] * 1e3), 1)
        t["us_per_pair"] = round(t["us_median"] / n, 3)
        result[f"rectify_n{n}"] = t
    cfg = cuda_depth.StereoMatchingConfiguration(height=HO, width=WO, downscale_factor=K, min_disparity=0,
                                                 max_disparity=D - 1)
    sm = cuda_depth.StereoMatching(cfg, max_batch=64)
    disp = torch.empty((64, HO, WO), device="cuda")
    result["match_n64"] = time_calls(lambda: sm.compute_disparity_map_batch(out[0], out[1], disp), args.iters,
                                     args.repeats, args.warmup)
    result["rectify_n64_over_match_n64"] = round(result["rectify_n64"]["us_median"] /
                                                 result["match_n64"]["us_median"], 3)
    gl, gr = (torch.from_numpy(a).cuda() for a in syn.make_batch(64, HO, WO, D, K))
    result["match_gray_synthetic_n64"] = time_calls(lambda: sm.compute_disparity_map_batch(gl, gr, disp), args.iters,
                                                    args.repeats, args.warmup)
    result["rectify_n64_over_match_gray_synthetic_n64"] = round(
        result["rectify_n64"]["us_median"] / result["match_gray_synthetic_n64"]["us_median"], 3)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
