#!/usr/bin/env python3
"""Cost of the right-view synthesis head at the reference's native size (384x1280, D = 65, S = 4, C = 3), on one caller
stream:
    python tools/synthesis_throughput.py [--repeats 7] [--iters 20]
Input: softmax of N(0, 3^2) logits as the probability volume and uniform frames (seeded).  Times
smx_synthesize_right_view on one frame and on 32, with float32 and with uint8 frames, and, in the same run, the torch
expression of what Deep3D computes after its softmax (F.interpolate of the volume, 65 shifted copies of the frame, mul,
sum, `* 255 + 0.5`, clamp) on one frame and looped over the 32 frames (its stack is 383 MB per frame, so it is not
batched).  Device events around `iters` back-to-back calls after a warm-up, `repeats` times; the median and the spread
(min, max) of the time per call.  Also: the counted traffic of a call (prob + left + out, each moved once), the rate it
amounts to, the time it would take at 2.2 TB/s (the aim for 32 frames: the rate README.md records for the tile-staged
confidence kernel with a guide), the ratio to the torch expression, and the largest difference between the two results.
Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats` the k_synthesis row gives the kernel's own time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd")]
import torch, torch.nn.functional as F, cuda_depth   # noqa: E401,E402

H, W, D, S, C = 384, 1280, 65, 4, 3
AIM_BYTES_PER_S = 2.2e12


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


def torch_expression(prob, left):
    """prob [1, D, h, w], left [1, C, H, W] in 0..1 -> [1, C, H, W] in 0..255, as the reference computes it."""
    up = F.interpolate(prob, scale_factor=S, mode="bilinear")
    shifted = []
    for d in range(D):
        s = torch.zeros_like(left)
        if d == 0:
            s = left
        else:
            s[..., :-d] = left[..., d:]
        shifted.append(s)
    view = torch.sum(torch.mul(up.unsqueeze(2), torch.stack(shifted, dim=1)), dim=1)
    return torch.clamp(view * 255 + 0.5, 0, 255)


def counted_bytes(n, left_bytes_per_value):
    return n * (D * (H // S) * (W // S) * 4 + C * H * W * left_bytes_per_value + C * H * W * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("synthesis_throughput.py needs a GPU: a time measured elsewhere says nothing")
    N = 32
    h, w = H // S, W // S
    gen = torch.Generator(device="cuda").manual_seed(0)
    prob = torch.softmax(torch.randn((N, D, h, w), device="cuda", generator=gen) * 3.0, dim=1).contiguous()
    left = torch.rand((N, C, H, W), device="cuda", generator=gen)
    left8 = (left * 255.0).round().to(torch.uint8)
    out = torch.empty((N, C, H, W), device="cuda")
    result = {"config": f"{W}x{H} D{D} S{S} C{C}", "stream": "one caller stream", "repeats": args.repeats,
              "iters": args.iters, "gpu": torch.cuda.get_device_name(0), "aim_TBps": AIM_BYTES_PER_S / 1e12}
    for name, frames, width in (("f32", left, 4), ("u8", left8, 1)):
        for n in (1, N):
            t = time_calls(lambda: cuda_depth._launch_synthesis(prob[:n], frames[:n], out[:n], n, C, D, h, w, S),
                           args.iters if n > 1 else 5 * args.iters, args.repeats, args.warmup)
            t["counted_MB"] = round(counted_bytes(n, width) / 1e6, 2)
            t["counted_GBps"] = round(counted_bytes(n, width) / t["us_median"] / 1e3, 1)
            t["us_at_aim"] = round(counted_bytes(n, width) / AIM_BYTES_PER_S * 1e6, 2)
            result[f"head_n{n}_{name}"] = t
    result["aim_met_n32_f32"] = result[f"head_n{N}_f32"]["us_median"] <= result[f"head_n{N}_f32"]["us_at_aim"]
    result["aim_met_n32_u8"] = result[f"head_n{N}_u8"]["us_median"] <= result[f"head_n{N}_u8"]["us_at_aim"]
    # the yardstick: the reference's expression, one frame per call
    result["torch_n1"] = time_calls(lambda: torch_expression(prob[:1], left[:1]), max(2, args.iters // 4), args.repeats, 2)

    def torch_loop():
        for k in range(N):
            torch_expression(prob[k:k + 1], left[k:k + 1])
    result[f"torch_n{N}_looped"] = time_calls(torch_loop, 1, args.repeats, 1)
    result["speedup_n1_f32"] = round(result["torch_n1"]["us_median"] / result["head_n1_f32"]["us_median"], 1)
    result[f"speedup_n{N}_f32"] = round(result[f"torch_n{N}_looped"]["us_median"] / result[f"head_n{N}_f32"]["us_median"], 1)
    ours = cuda_depth.synthesize_right_view(prob[:1], left[:1], scale=S)
    result["max_abs_diff_to_torch"] = float((ours - torch_expression(prob[:1], left[:1])).abs().max())
    torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
