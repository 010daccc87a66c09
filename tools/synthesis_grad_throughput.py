#!/usr/bin/env python3
"""Cost of training through the synthesis head at the reference's native size (384x1280, D = 65, S = 4, C = 3), on one
caller stream:
    python tools/synthesis_grad_throughput.py [--repeats 7] [--iters 10]
Input: softmax of N(0, 3^2) logits as the probability volume, uniform frames and the gradient of an L1 loss (random
signs over the pixel count), seeded.  Times, on one frame and on 32: the training-form forward
(smx_synthesis_head_forward), the backward (smx_synthesis_head_backward) and, in the same run, the inference head
(smx_synthesize_right_view).  Then forward plus backward of the reference's torch expression (F.interpolate of the
volume, 65 shifted copies of the frame, mul, sum, autograd) on one frame and on the largest batch (at most 32) whose
measured peak fits the free memory.  Device events around `iters` back-to-back calls after a warm-up, `repeats` times;
the median and the spread (min, max) of the time per call.  Also: torch.cuda.max_memory_allocated over one forward plus
backward of one frame, fused and torch, above what the operands take; the largest difference between the two gradients;
and the aim: the backward rule has 10 float32 operations per pixel and plane against the forward rule's 15,
so 32 frames of backward should take no more than 10 / 15 of the inference head's 32 frames.
Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats` the k_synthesis_grad row gives the kernel's own time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd")]
import torch, torch.nn.functional as F, cuda_depth   # noqa: E401,E402
from cuda_depth import _native as N_                 # noqa: E402

H, W, D, S, C = 384, 1280, 65, 4, 3
OPS_BACKWARD, OPS_FORWARD = 10, 15                    # float32 operations per pixel and plane, from the header's rules


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


def torch_view(prob, left):
    """prob [n, D, h, w], left [n, C, H, W] in 0..1 -> the view in 0..1, as the reference's training graph computes it."""
    up = F.interpolate(prob, scale_factor=S, mode="bilinear")
    shifted = []
    for d in range(D):
        s = torch.zeros_like(left)
        if d == 0:
            s = left
        else:
            s[..., :-d] = left[..., d:]
        shifted.append(s)
    return torch.sum(torch.mul(up.unsqueeze(2), torch.stack(shifted, dim=1)), dim=1)


def peak_of(step):
    """max_memory_allocated over one call of step(), above what is allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("synthesis_grad_throughput.py needs a GPU: a time measured elsewhere says nothing")
    N = 32
    h, w = H // S, W // S
    gen = torch.Generator(device="cuda").manual_seed(0)
    prob = torch.softmax(torch.randn((N, D, h, w), device="cuda", generator=gen) * 3.0, dim=1).contiguous()
    left = torch.rand((N, C, H, W), device="cuda", generator=gen)
    grad = torch.where(torch.rand((N, C, H, W), device="cuda", generator=gen) < 0.5, -1.0, 1.0) / (C * H * W)
    view, grad_prob = torch.empty((N, C, H, W), device="cuda"), torch.empty((N, D, h, w), device="cuda")
    dev, stream = 0, torch.cuda.current_stream().cuda_stream
    result = {"config": f"{W}x{H} D{D} S{S} C{C}", "stream": "one caller stream", "repeats": args.repeats,
              "iters": args.iters, "gpu": torch.cuda.get_device_name(0),
              "ops_per_pixel_plane": {"backward": OPS_BACKWARD, "forward": OPS_FORWARD}}
    for n in (1, N):
        iters = args.iters if n > 1 else 5 * args.iters
        result[f"head_n{n}"] = time_calls(
            lambda: cuda_depth._launch_synthesis(prob[:n], left[:n], view[:n], n, C, D, h, w, S), iters, args.repeats, args.warmup)
        result[f"forward_n{n}"] = time_calls(
            lambda: N_.check(N_.LIB.smx_synthesis_head_forward(dev, n, C, N_.DTYPE_F32, D, h, w, S, prob.data_ptr(),
                                                               left.data_ptr(), view.data_ptr(), stream)),
            iters, args.repeats, args.warmup)
        result[f"backward_n{n}"] = time_calls(
            lambda: N_.check(N_.LIB.smx_synthesis_head_backward(dev, n, C, N_.DTYPE_F32, D, h, w, S, grad.data_ptr(),
                                                                left.data_ptr(), grad_prob.data_ptr(), stream)),
            iters, args.repeats, args.warmup)
    aim = result[f"head_n{N}"]["us_median"] * OPS_BACKWARD / OPS_FORWARD
    result[f"aim_us_backward_n{N}"] = round(aim, 2)
    result["aim_met"] = result[f"backward_n{N}"]["us_median"] <= aim

    # one forward plus backward through autograd, fused and torch: memory, agreement, time
    def fused_step(n=1):
        p = prob[:n].detach().requires_grad_()
        cuda_depth.synthesis_head(p, left[:n], scale=S).backward(grad[:n])
        return p.grad

    def torch_step(n=1):
        p = prob[:n].detach().requires_grad_()
        torch_view(p, left[:n]).backward(grad[:n])
        return p.grad

    result["peak_bytes_fused_n1"] = peak_of(fused_step)
    result["peak_bytes_torch_n1"] = peak_of(torch_step)
    result["max_abs_diff_of_gradients"] = float((fused_step() - torch_step()).abs().max())
    result["max_abs_gradient"] = float(torch_step().abs().max())
    free = torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
    fit = max(1, min(N, int(0.8 * free) // max(1, result["peak_bytes_torch_n1"])))
    result["torch_largest_batch"] = fit
    result["fused_step_n1"] = time_calls(fused_step, args.iters, args.repeats, 2)
    result["torch_step_n1"] = time_calls(torch_step, max(2, args.iters // 4), args.repeats, 2)
    result[f"fused_step_n{fit}"] = time_calls(lambda: fused_step(fit), max(2, args.iters // 2), args.repeats, 2)
    result[f"torch_step_n{fit}"] = time_calls(lambda: torch_step(fit), 1, args.repeats, 1)
    result["speedup_step_n1"] = round(result["torch_step_n1"]["us_median"] / result["fused_step_n1"]["us_median"], 1)
    result[f"speedup_step_n{fit}"] = round(result[f"torch_step_n{fit}"]["us_median"] /
                                          result[f"fused_step_n{fit}"]["us_median"], 1)
    torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
