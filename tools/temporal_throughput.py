#!/usr/bin/env python3
"""Cost and effect of the motion-gated temporal filter at C2 (1242x375), on one caller stream:
    python tools/temporal_throughput.py [--repeats 7] [--iters 20] [--frames 24]
Times smx_temporal_filter (cuda_depth.TemporalFilter.apply, radius 1, guide_out written) on one map and on 32 maps,
with a confidence and without.  Device events around `iters` back-to-back calls after a warm-up, `repeats` times; the
median and the spread (min, max) of the time per call.  Bytes counted: every plane read or written once (d, g, G, D, A
read, c read with a confidence; out, D', A', guide_out written), nothing for the halo; TB/s = those bytes over the
median time.
Quality, on the synthetic sequences of stereo_sequences (static: fresh +-2 noise per frame; moving: an object moving
3 px per frame), matched by the engine (128 disparities, K = 2) with the LR check and the speckle filter, the left
gray frames as the guide: the temporal standard deviation of the pixels valid in every frame, the valid / invalid
toggle rate and the MAE against the truth, of the raw maps and of the filtered ones, scored right of the largest
disparity and after 4 warm-up frames.  Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats` the k_temporal
row gives the kernel's own time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch, cuda_depth, stereo_sequences as seqs   # noqa: E401,E402
import temporal_ref   # noqa: E402  (the quality measures only)

H, W, D, K = 375, 1242, 128, 2
SPECKLE, MAX_DIFF = 100, 1.0
WARM_FRAMES = 4


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


def quality(sm, seq):
    """Raw and filtered maps of one sequence: temporal std, toggle rate and MAE (scored columns >= D)."""
    filt = cuda_depth.TemporalFilter(1, H, W)
    raw, filtered = [], []
    for left, right, _ in seq:
        lt, rt = torch.from_numpy(left[None]).cuda(), torch.from_numpy(right[None]).cuda()
        m = sm.compute_disparity_map_batch_lr(lt, rt)[0]
        m = cuda_depth.filter_speckles(m, max_speckle_size=SPECKLE, max_diff=MAX_DIFF)
        raw.append(m.cpu().numpy())
        filtered.append(filt.apply(m, lt[0]).cpu().numpy())
    truth = np.stack([t for _, _, t in seq])[WARM_FRAMES:]
    raw, filtered = np.stack(raw)[WARM_FRAMES:], np.stack(filtered)[WARM_FRAMES:]
    scored = np.zeros((H, W), bool)
    scored[:, D:] = True
    out = {}
    for name, maps in (("raw", raw), ("filtered", filtered)):
        valid = (maps != -1.0) & scored
        out[name] = {"temporal_std": round(temporal_ref.temporal_std(maps, scored=scored), 4),
                     "toggle_rate": round(temporal_ref.toggle_rate(maps, scored=scored), 5),
                     "mae": round(float(np.abs(maps - truth)[valid].mean()), 4),
                     "valid_fraction": round(float(valid.sum() / (scored.sum() * len(maps))), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=24)
    args = ap.parse_args()
    result = {"config": f"C2 {W}x{H}", "stream": "one caller stream", "motion_radius": 1, "repeats": args.repeats,
              "iters": args.iters, "gpu": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(0)
    n_max = 32
    disp = torch.from_numpy(rng.uniform(0, 100, (n_max, H, W)).astype(np.float32)).cuda()
    conf = torch.from_numpy(rng.uniform(0, 1, (n_max, H, W)).astype(np.float32)).cuda()
    guide = torch.from_numpy(rng.integers(0, 256, (n_max, H, W)).astype(np.float32)).cuda()
    out = torch.empty_like(disp)
    for n in (1, 32):
        filt = cuda_depth.TemporalFilter(n, H, W)
        for name, c in (("no_conf", None), ("conf", conf)):
            shape = (n, H, W)
            d, g, o = disp[:n].view(shape), guide[:n].view(shape), out[:n].view(shape)
            cc = None if c is None else c[:n].view(shape)
            iters = args.iters if n > 1 else 5 * args.iters
            t = time_calls(lambda: filt.apply(d, g, confidence=cc, out=o), iters, args.repeats, args.warmup)
            planes = 9 + (c is not None)
            nbytes = planes * 4 * n * H * W
            t["bytes"] = nbytes
            t["tb_per_s"] = round(nbytes / (t["us_median"] * 1e-6) / 1e12, 3)
            result[f"n{n}_{name}"] = t
    cfg = cuda_depth.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=0,
                                                 max_disparity=D - 1)
    sm = cuda_depth.StereoMatching(cfg, max_batch=2)
    result["quality_static"] = quality(sm, seqs.static_sequence(args.frames, H, W, D, K, index=0, seed=1))
    result["quality_moving"] = quality(sm, seqs.moving_sequence(args.frames, H, W, D, K, index=0, seed=1, step=3))
    torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
