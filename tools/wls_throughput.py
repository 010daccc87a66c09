#!/usr/bin/env python3
"""Cost of the image-guided weighted least squares filter at C2 (1242x375), on one caller stream:
    python tools/wls_throughput.py [--repeats 7] [--iters 20]
Input: the LR-checked output of scene-like synthetic pairs (stereo_synthetic, 128 disparities, K = 2), speckle-filtered
(max_speckle_size 100, max_diff 1), with the left gray images as the guide and the tables of wls_tables(8000, 1.5, T)
(binary confidence, min_weight 1e-3: the pipeline's settings).  Times smx_wls_filter on 32 maps and on one map at T = 3,
and both again at T = 1.  The LR call of 32 pairs that produces the input is timed too, as the yardstick.  Device events
around `iters` back-to-back calls after a warm-up, `repeats` times; prints one JSON line with the median and the spread
(min, max) of the time per call.  Under `rocprofv3 --kernel-trace --stats` the k_wls_rows / k_wls_cols rows give the
split between the row and the column passes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd")]
import numpy as np, torch, cuda_depth, stereo_synthetic as syn   # noqa: E401,E402

H, W, D, K = 375, 1242, 128, 2
SPECKLE, MAX_DIFF = 100, 1.0
LAM, SIGMA_COLOR, MIN_WEIGHT = 8000.0, 1.5, 1e-3


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
    result = {"config": f"C2 {W}x{H}", "stream": "one caller stream", "lam": LAM, "sigma_color": SIGMA_COLOR,
              "min_weight": MIN_WEIGHT, "repeats": args.repeats, "iters": args.iters,
              "gpu": torch.cuda.get_device_name(0)}
    result["lr_n32"] = time_calls(lambda: sm.compute_disparity_map_batch_lr(L, R, checked), args.iters, args.repeats,
                                  args.warmup)
    torch.cuda.synchronize()
    spk = cuda_depth.filter_speckles(checked, max_speckle_size=SPECKLE, max_diff=MAX_DIFF)
    torch.cuda.synchronize()
    result["invalid_fraction"] = round(float((spk == -1.0).float().mean()), 4)
    ws = cuda_depth._wls_workspace(32, H, W, checked.device)
    out = torch.empty((32, H, W), device="cuda")
    for T in (3, 1):
        lam, rw = cuda_depth.wls_tables(LAM, SIGMA_COLOR, T)
        res = {}
        for n in (32, 1):
            src, dst, gd = spk[:n], out[:n], L[:n]
            iters = args.iters if n > 1 else 5 * args.iters
            res[f"wls_n{n}"] = time_calls(
                lambda: cuda_depth._launch_wls(src, None, gd, dst, n, H, W, lam, rw, MIN_WEIGHT, -1.0, ws),
                iters, args.repeats, args.warmup)
        res["wls_n32_over_lr_n32"] = round(res["wls_n32"]["us_median"] / result["lr_n32"]["us_median"], 3)
        result[f"T{T}"] = res
    torch.cuda.synchronize()
    result["invalid_fraction_after_T1"] = round(float((out == -1.0).float().mean()), 5)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
