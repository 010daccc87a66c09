#!/usr/bin/env python3
"""Cost of the speckle filter and the hole fill at C2 (1242x375), on one caller stream:
    python tools/postprocess_throughput.py [--repeats 7] [--iters 20]
Times smx_filter_speckles (max_speckle_size 100, max_diff 1) and smx_fill_invalid on 32 maps and on one map, for three
inputs: the LR-checked output of scene-like synthetic pairs (stereo_synthetic, 128 disparities, K = 2), a constant map
(one region of every pixel: the contention case) and a checkerboard (every pixel its own region).  The LR call of 32 pairs
that produces the first input is timed too, as the yardstick.  Device events around `iters` back-to-back calls after a
warm-up, `repeats` times; prints one JSON line with the median and the spread (min, max) of the time per call.  The
workspace is allocated once, outside the timed loop.  Under `rocprofv3 --kernel-trace --stats` the k_spk_* / k_fill_*
rows give the per-kernel split."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd")]
import numpy as np, torch, cuda_depth, stereo_synthetic as syn   # noqa: E401,E402

H, W, D, K = 375, 1242, 128, 2
SPECKLE, MAX_DIFF = 100, 1.0


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
    args = ap.parse_args()
    cfg = cuda_depth.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
    prs = [syn.make_pair(H, W, D, K, i)[:2] for i in range(8)]
    L = torch.from_numpy(np.stack([p[0] for p in prs])).cuda().repeat(4, 1, 1).contiguous()     # 32 pairs
    R = torch.from_numpy(np.stack([p[1] for p in prs])).cuda().repeat(4, 1, 1).contiguous()
    sm = cuda_depth.StereoMatching(cfg, max_batch=64)
    checked = torch.empty((32, H, W), device="cuda")
    result = {"config": f"C2 {W}x{H}", "stream": "one caller stream", "max_speckle_size": SPECKLE, "max_diff": MAX_DIFF,
              "repeats": args.repeats, "iters": args.iters, "gpu": torch.cuda.get_device_name(0)}
    result["lr_n32"] = time_calls(lambda: sm.compute_disparity_map_batch_lr(L, R, checked), args.iters, args.repeats,
                                  args.warmup)
    torch.cuda.synchronize()
    inputs = {
        "scene_lr": checked,
        "constant": torch.full((32, H, W), 17.5, device="cuda"),
        "checkerboard": ((torch.arange(H, device="cuda")[:, None] + torch.arange(W, device="cuda")[None]) % 2 * 10.0)
        .float().expand(32, H, W).contiguous(),
    }
    result["scene_lr_invalid_fraction"] = round(float((checked == -1.0).float().mean()), 4)
    ws = cuda_depth._postprocess_workspace(32, H, W, checked.device)
    out = torch.empty((32, H, W), device="cuda")
    for name, maps in inputs.items():
        res = {}
        for n in (32, 1):
            src, dst = maps[:n], out[:n]
            iters = args.iters if n > 1 else 5 * args.iters
            res[f"speckles_n{n}"] = time_calls(
                lambda: cuda_depth._launch_filter_speckles(src, dst, n, H, W, SPECKLE, MAX_DIFF, -1.0, ws),
                iters, args.repeats, args.warmup)
            res[f"fill_n{n}"] = time_calls(lambda: cuda_depth._launch_fill_invalid(src, dst, n, H, W, -1.0, ws),
                                           iters, args.repeats, args.warmup)
        res["speckles_n32_over_lr_n32"] = round(res["speckles_n32"]["us_median"] / result["lr_n32"]["us_median"], 3)
        result[name] = res
    print(json.dumps(result))


if __name__ == "__main__":
    main()
