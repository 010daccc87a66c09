#!/usr/bin/env python3
"""Cost of semi-global matching (cuda_depth.StereoSGM) at C2 (1242x375), D = 128, on one caller stream:
    python tools/sgm_throughput.py [--repeats 7] [--iters 10]
Input: scene-like synthetic pairs (stereo_synthetic.make_slanted_pair), as u8 gray ([1,H,W]) and as f32 RGB ([3,H,W]).
Times StereoSGM.compute with the defaults (P1 10, P2 120, subpixel, no uniqueness or LR check) for 4 and 8 paths, on
one pair and on a batch of 16, and a 16-pair engine call (StereoMatching.compute_disparity_map_batch, u8 gray, K = 2)
of the same pairs as the yardstick.  Device events around `iters` back-to-back calls after a warm-up, `repeats` times;
prints one JSON line with the median and the spread (min, max) of the time per call, and pairs/s of the batches.
Under `rocprofv3 --kernel-trace --stats` the k_sgm_* rows give the per-kernel split."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd")]
import numpy as np, torch, cuda_depth, stereo_synthetic as syn   # noqa: E401,E402

H, W, D, K, N = 375, 1242, 128, 2, 16


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    prs = [syn.make_slanted_pair(H, W, D, 1, i)[:2] for i in range(4)]
    gl = np.stack([prs[i % 4][0] for i in range(N)])[:, None]           # [16, 1, H, W]
    gr = np.stack([prs[i % 4][1] for i in range(N)])[:, None]
    inputs = {
        "u8_gray": (torch.from_numpy(gl.astype(np.uint8)).cuda(), torch.from_numpy(gr.astype(np.uint8)).cuda()),
        "f32_rgb": (torch.from_numpy(np.repeat(gl, 3, 1)).cuda(), torch.from_numpy(np.repeat(gr, 3, 1)).cuda()),
    }
    result = {"config": f"C2 {W}x{H} D={D}", "stream": "one caller stream", "repeats": args.repeats,
              "iters": args.iters, "gpu": torch.cuda.get_device_name(0)}
    out = torch.empty((N, H, W), device="cuda")
    for paths in (4, 8):
        sgm = cuda_depth.StereoSGM(0, D - 1, paths=paths)
        for name, (L, R) in inputs.items():
            res = {}
            res["n1"] = time_calls(lambda: sgm.compute(L[0], R[0], out=out[0]), args.iters, args.repeats, args.warmup)
            res[f"n{N}"] = time_calls(lambda: sgm.compute(L, R, out=out), args.iters, args.repeats, args.warmup)
            res[f"pairs_per_s_n{N}"] = round(N / (res[f"n{N}"]["us_median"] * 1e-6), 1)
            result[f"paths{paths}_{name}"] = res
    cfg = cuda_depth.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=0,
                                                 max_disparity=D - 1)
    sm = cuda_depth.StereoMatching(cfg, max_batch=N)
    L8, R8 = inputs["u8_gray"][0][:, 0].contiguous(), inputs["u8_gray"][1][:, 0].contiguous()
    eng = time_calls(lambda: sm.compute_disparity_map_batch(L8, R8, out), args.iters, args.repeats, args.warmup)
    eng[f"pairs_per_s_n{N}"] = round(N / (eng["us_median"] * 1e-6), 1)
    result[f"engine_u8_gray_n{N}"] = eng
    result["aims"] = {"pairs_per_s_n16_u8_gray": 2500, "us_n1": 1000}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
