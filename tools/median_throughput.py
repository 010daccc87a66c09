#!/usr/bin/env python3
"""Cost of the image-guided weighted median at C2 (1242x375), on one caller stream:
    python tools/median_throughput.py [--repeats 7] [--iters 20] [--radius 9]
Input: the LR-checked output of scene-like synthetic pairs (stereo_synthetic, 128 disparities, K = 2), speckle-filtered
(max_speckle_size 100, max_diff 1) and filled, with the left gray images as the guide and the tables of
median_weight_tables(radius, 10, 5).  Times smx_weighted_median on 32 maps and on one map in holes mode (holes = the
speckle-filtered map: only the pixels the fill wrote) and in whole-map mode (every valid pixel).  The LR call of 32 pairs
that produces the input is timed too, as the yardstick.  Device events around `iters` back-to-back calls after a
warm-up, `repeats` times; prints one JSON line with the median and the spread (min, max) of the time per call.  Under
`rocprofv3 --kernel-trace --stats` the k_median rows give the per-kernel split."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd")]
import numpy as np, torch, cuda_depth, stereo_synthetic as syn   # noqa: E401,E402

H, W, D, K = 375, 1242, 128, 2
SPECKLE, MAX_DIFF = 100, 1.0
SIGMA_COLOR, SIGMA_SPACE = 10.0, 5.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--radius", type=int, default=9)
    args = ap.parse_args()
    cfg = cuda_depth.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
    prs = [syn.make_pair(H, W, D, K, i)[:2] for i in range(8)]
    L = torch.from_numpy(np.stack([p[0] for p in prs])).cuda().repeat(4, 1, 1).contiguous()     # 32 pairs
    R = torch.from_numpy(np.stack([p[1] for p in prs])).cuda().repeat(4, 1, 1).contiguous()
    sm = cuda_depth.StereoMatching(cfg, max_batch=64)
    checked = torch.empty((32, H, W), device="cuda")
    result = {"config": f"C2 {W}x{H}", "stream": "one caller stream", "radius": args.radius,
              "sigma_color": SIGMA_COLOR, "sigma_space": SIGMA_SPACE, "repeats": args.repeats, "iters": args.iters,
              "gpu": torch.cuda.get_device_name(0)}
    result["lr_n32"] = time_calls(lambda: sm.compute_disparity_map_batch_lr(L, R, checked), args.iters, args.repeats,
                                  args.warmup)
    torch.cuda.synchronize()
    spk = cuda_depth.filter_speckles(checked, max_speckle_size=SPECKLE, max_diff=MAX_DIFF)
    filled = cuda_depth.fill_invalid(spk)
    torch.cuda.synchronize()
    result["filled_fraction"] = round(float((spk == -1.0).float().mean()), 4)
    rw, sw = cuda_depth.median_weight_tables(args.radius, SIGMA_COLOR, SIGMA_SPACE)
    ws = cuda_depth._median_workspace(32, H, W, checked.device)
    out = torch.empty((32, H, W), device="cuda")
    for mode, holes in (("holes", spk), ("whole_map", None)):
        res = {}
        for n in (32, 1):
            src, dst, hl, gd = filled[:n], out[:n], None if holes is None else holes[:n], L[:n]
            iters = args.iters if n > 1 else 5 * args.iters
            if mode == "whole_map":
                iters = max(1, iters // 5)
            res[f"median_n{n}"] = time_calls(
                lambda: cuda_depth._launch_weighted_median(src, hl, gd, dst, n, H, W, args.radius, rw, sw, -1.0, ws),
                iters, args.repeats, args.warmup)
        res["median_n32_over_lr_n32"] = round(res["median_n32"]["us_median"] / result["lr_n32"]["us_median"], 3)
        res["pixels_filtered_n32"] = int((spk == -1.0).sum()) if holes is not None else \
            int((torch.isfinite(filled) & (filled != -1.0)).sum())
        res["ns_per_filtered_pixel_n32"] = round(res["median_n32"]["us_median"] * 1e3 / res["pixels_filtered_n32"], 3)
        result[mode] = res
    print(json.dumps(result))


if __name__ == "__main__":
    main()
