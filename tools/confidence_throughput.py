#!/usr/bin/env python3
"""Cost and use of the per-pixel confidence at C2 (1242x375), on one caller stream:
    python tools/confidence_throughput.py [--repeats 7] [--iters 20]
Input: the LR-checked output of scene-like synthetic pairs (stereo_synthetic, 128 disparities, K = 2) with the engine's
right-view maps and the left gray images as the guide.  Times smx_confidence_map on 32 maps and on one map, with the
guide (radius 2) and without; smx_sgm_with_right_map against smx_sgm for one u8 gray pair (128 disparities, 8 paths),
with the LR check and without; and one pipeline frame (cuda backend, LR check, speckle filter, WLS filter) with
confidence=True against confidence=False.  Device events around `iters` back-to-back calls after a warm-up, `repeats`
times; the median and the spread (min, max) of the time per call.  Quality, against the ground truth of a slanted
synthetic scene (columns right of the largest disparity; the engine's map with the LR check opened wide): the bad-pixel
rate (|error| > 1) of the pixels with confidence >= 0.5 against that of every valid pixel, and the MAE of the WLS filter
with binary confidence against the one weighted by the confidence.
Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats` the k_confidence row gives the kernel's own time."""
import argparse
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd")]
import numpy as np, torch, cuda_depth, stereo_synthetic as syn   # noqa: E401,E402

H, W, D, K = 375, 1242, 128, 2
SPECKLE, MAX_DIFF = 100, 1.0
LAM, SIGMA_COLOR = 8000.0, 1.5


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


def quality(sm):
    """Bad-pixel rates and WLS MAE on a slanted scene (stereo_synthetic.make_slanted_pair: multi-scale texture, a ground
    ramp, two objects), scored right of the largest disparity.  The left map is the engine's LR call with the check
    opened wide (max_diff 1e6), so the confidence, not the check, has to find the mismatches."""
    l, r, truth = syn.make_slanted_pair(H, W, D, K, 0)
    lt, rt = torch.from_numpy(l[None]).cuda(), torch.from_numpy(r[None]).cuda()
    right = torch.empty((1, H, W), device="cuda")
    lr = sm.compute_disparity_map_batch_lr(lt, rt, right_out=right, max_diff=1e6)[0].clone()
    guide = lt[0]
    spk = cuda_depth.filter_speckles(lr, max_speckle_size=SPECKLE, max_diff=MAX_DIFF)
    conf = cuda_depth.confidence_map(spk, right[0], guide)
    binary = cuda_depth.wls_filter(spk, guide, lam=LAM, sigma_color=SIGMA_COLOR)
    weighted = cuda_depth.wls_filter(spk, guide, lam=LAM, sigma_color=SIGMA_COLOR, confidence=conf)
    d, c, t = spk.cpu().numpy(), conf.cpu().numpy(), truth
    scored = np.zeros((H, W), bool)
    scored[:, D:] = True
    valid = scored & (d != -1.0)
    bad = np.abs(d - t) > 1
    sure = valid & (c >= 0.5)
    b, w = binary.cpu().numpy(), weighted.cpu().numpy()
    both = scored & (b != -1.0) & (w != -1.0)
    return {"bad_rate_valid": round(float(bad[valid].mean()), 5), "bad_rate_conf_ge_0.5": round(float(bad[sure].mean()), 5),
            "fraction_conf_ge_0.5": round(float(sure.sum() / valid.sum()), 4),
            "wls_mae_binary": round(float(np.abs(b - t)[both].mean()), 4),
            "wls_mae_confidence": round(float(np.abs(w - t)[both].mean()), 4),
            "wls_scored_fraction": round(float(both.sum() / scored.sum()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    cfg = cuda_depth.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
    prs = [syn.make_pair(H, W, D, K, i) for i in range(8)]
    L = torch.from_numpy(np.stack([p[0] for p in prs])).cuda().repeat(4, 1, 1).contiguous()     # 32 pairs
    R = torch.from_numpy(np.stack([p[1] for p in prs])).cuda().repeat(4, 1, 1).contiguous()
    sm = cuda_depth.StereoMatching(cfg, max_batch=64)
    checked, right = torch.empty((32, H, W), device="cuda"), torch.empty((32, H, W), device="cuda")
    result = {"config": f"C2 {W}x{H}", "stream": "one caller stream", "radius": 2, "lr_scale": 1.0,
              "texture_scale": 10.0, "repeats": args.repeats, "iters": args.iters, "gpu": torch.cuda.get_device_name(0)}
    sm.compute_disparity_map_batch_lr(L, R, checked, right_out=right)
    guides = L                                                        # gray inputs are their own gray planes
    out = torch.empty((32, H, W), device="cuda")
    for name, gd in (("guide", guides), ("no_guide", None)):
        for n in (32, 1):
            g = None if gd is None else gd[:n]
            iters = args.iters if n > 1 else 5 * args.iters
            result[f"conf_n{n}_{name}"] = time_calls(
                lambda: cuda_depth._launch_confidence(checked[:n], right[:n], g, out[:n], n, H, W, 2, 1.0, 10.0, -1.0),
                iters, args.repeats, args.warmup)
    result["quality"] = quality(sm)
    # SGM: the right-view map beside the plain call
    lu8, ru8 = L[:1, None].to(torch.uint8).contiguous(), R[:1, None].to(torch.uint8).contiguous()
    sgm_out, sgm_right = torch.empty((1, H, W), device="cuda"), torch.empty((1, H, W), device="cuda")
    for lr in (1.0, None):
        sgm = cuda_depth.StereoSGM(0, D - 1, paths=8, lr_max_diff=lr)
        key = "sgm_lr" if lr is not None else "sgm_no_lr"
        result[key] = {
            "plain": time_calls(lambda: sgm.compute(lu8, ru8, out=sgm_out), args.iters, args.repeats, 2),
            "with_right_map": time_calls(lambda: sgm.compute(lu8, ru8, out=sgm_out, right_out=sgm_right), args.iters,
                                         args.repeats, 2)}
    # pipeline frame: LR check, speckle filter, WLS, with and without the confidence
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    pcfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=0, max_disparity=D - 1,
                                         left_right_check=True)
    rgb_l = torch.from_numpy(syn.gray_to_rgb(prs[0][0])).cuda()
    rgb_r = torch.from_numpy(syn.gray_to_rgb(prs[0][1])).cuda()
    for flag in (False, True):
        with contextlib.redirect_stdout(io.StringIO()):                 # the backend banner: one JSON line only
            pipe = DepthEstimationPipeline(pcfg, speckle_max_size=SPECKLE, speckle_max_diff=MAX_DIFF, wls_lambda=LAM,
                                           wls_sigma_color=SIGMA_COLOR, confidence=flag)
        result[f"pipeline_confidence_{str(flag).lower()}"] = time_calls(lambda: pipe.process(rgb_l, rgb_r),
                                                                        args.iters, args.repeats, 3)
    torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
