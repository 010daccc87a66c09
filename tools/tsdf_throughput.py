#!/usr/bin/env python3
"""Cost and quality of TSDF fusion at C2 (1242x375) with KITTI-like intrinsics (f = 721.5 px, B = 0.54 m), on one caller
stream:
    python tools/tsdf_throughput.py [--repeats 7] [--iters 10]
Throughput: a 512x256x512 volume of 0.1 m voxels (51.2 x 25.6 x 51.2 m, 67.1 M voxels, u8 RGB colour) with the camera
at the centre of its -z face looking along +z, and synthetic maps of depths uniform in 3..50 m with 10 % invalid
pixels and a u8 RGB left frame; the 8-map case drives 0.5 m forward per frame.  Times smx_tsdf_integrate of 1 map per
call, of 8 maps per call and 8 single-map calls (poses on the device), and smx_tsdf_extract_points (normals and
colours) of the volume those 8 maps filled.  Each timed step is captured `iters` times into one HIP graph (no host
overhead in the numbers), replayed after a warm-up, `repeats` times: the median and the spread (min, max) per step.
Bytes counted for integration: the pixel pass (the map and the colour planes read, 12 B per pixel written) and the
measured voxels' state read and written once (24 B each); for extraction: tsdf and weight read twice.  TB/s = those
bytes over the median time.
Quality: an analytic scene (a ground plane and three boxes, tests/tsdf_ref.py) seen from 12 poses at C2, disparities
with sigma = 0.5 px noise and 5 % outliers; the RMS and 95th-percentile distance to the true surface of the fused points
(0.05 m voxels) against the single-frame reproject_to_3d clouds cropped to the same volume.
The yardstick is the LR call of 32 pairs (f32 gray, 128 disparities, K = 2) timed the same way but eagerly.  Prints one
JSON line."""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch, cuda_depth   # noqa: E401,E402
from cuda_depth import _native           # noqa: E402
import tsdf_ref                          # noqa: E402

H, W, D, K = 375, 1242, 128, 2
FOCAL, BASELINE = 721.5, 0.54
DIMS, VS, ORIGIN = (512, 256, 512), 0.1, (-25.6, -12.8, 0.0)


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


class Integrator:
    """smx_tsdf_integrate of maps [n, H, W] with device poses [n, 3, 4] into vol, on the current stream."""

    def __init__(self, vol, disp, rgb, w2c, Q):
        self.vol, self.disp, self.rgb, self.w2c = vol, disp, rgb, w2c
        self.n = disp.shape[0]
        self.wsb = _native.LIB.smx_tsdf_integrate_workspace_bytes(self.n, H, W)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        self.q = (C.c_float * 16)(*Q.reshape(-1).tolist())
        self.p = (C.c_float * 16)(*cuda_depth.projection_matrix(Q).reshape(-1).tolist())
        self.o = (C.c_float * 3)(*vol.origin)

    def __call__(self):
        v = self.vol
        nx, ny, nz = v.dims
        cuda_depth.check(_native.LIB.smx_tsdf_integrate(
            0, nx, ny, nz, self.o, v.voxel_size, v.truncation, v.max_weight, v.tsdf.data_ptr(), v.weight.data_ptr(),
            v.color.data_ptr(), self.n, H, W, self.disp.data_ptr(), self.q, self.p, self.w2c.data_ptr(), None, 0.0,
            0.0, math.inf, -1.0, self.rgb.data_ptr(), 3, _native.DTYPE_U8, self.ws.data_ptr(), self.wsb,
            C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def quality(n_poses=12):
    scene = tsdf_ref.Scene(ground_y=1.65, boxes=[((-3.0, -0.2, 8.0), (-1.0, 1.65, 10.0)),
                                                 ((1.0, -0.5, 12.0), (3.5, 1.65, 14.0)),
                                                 ((-2.0, 0.2, 16.0), (1.0, 1.65, 18.0))])
    dims, vs, origin = (256, 96, 384), 0.05, (-6.4, -3.0, 3.0)
    lo = np.array(origin)
    hi = lo + vs * np.array(dims)
    Q = cuda_depth.reprojection_matrix(FOCAL, W / 2.0, H / 2.0, BASELINE)
    rng = np.random.default_rng(7)
    poses = np.stack([tsdf_ref.look_at((rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1), 0.25 * i),
                                       (rng.uniform(-0.5, 0.5), 0.5, 0.25 * i + 20.0)) for i in range(n_poses)])
    vol = cuda_depth.TSDFVolume(dims, vs, origin, color=False)
    single = []
    for pose in poses:
        d = scene.render(pose, H, W, FOCAL, W / 2.0, H / 2.0, BASELINE)
        ok = d > 0
        d[ok] += rng.normal(0.0, 0.5, int(ok.sum())).astype(np.float32)
        out = ok & (rng.random(d.shape) < 0.05)
        d[out] = rng.uniform(1.0, 96.0, int(out.sum())).astype(np.float32)
        td = torch.from_numpy(d).cuda()
        vol.integrate(td, Q, pose)
        pts = cuda_depth.reproject_to_3d(td, Q).points.cpu().numpy().astype(np.float64)
        pw = pts @ pose[:3, :3].T + pose[:3, 3]
        pw = pw[np.all((pw >= lo) & (pw < hi), axis=1)]
        single.append(scene.distance(pw))
    fused = scene.distance(vol.extract_point_cloud(min_weight=2.0, normals=False).points.cpu().numpy())
    single = np.concatenate(single)
    rms = lambda e: float(np.sqrt(np.mean(e ** 2)))  # noqa: E731
    res = {"poses": n_poses, "voxel_m": vs, "noise_px": 0.5, "outliers": 0.05, "fused_points": int(fused.size),
           "fused_rms_m": round(rms(fused), 4), "fused_p95_m": round(float(np.percentile(fused, 95)), 4),
           "single_rms_m": round(rms(single), 4), "single_p95_m": round(float(np.percentile(single, 95)), 4)}
    res["rms_ratio"] = round(res["fused_rms_m"] / res["single_rms_m"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    n = 8
    z = rng.uniform(3.0, 50.0, (n, H, W))
    d = (FOCAL * BASELINE / z).astype(np.float32)
    d[rng.random((n, H, W)) < 0.10] = -1.0
    disp = torch.from_numpy(d).cuda()
    rgb = torch.from_numpy(rng.integers(0, 256, (n, 3, H, W)).astype(np.uint8)).cuda()
    Q = cuda_depth.reprojection_matrix(FOCAL, W / 2.0, H / 2.0, BASELINE)
    c2w = np.stack([np.eye(4)] * n)
    c2w[:, 2, 3] = 0.5 * np.arange(n)
    w2c = torch.from_numpy(cuda_depth.world_to_camera_poses(c2w)).cuda()
    vol = cuda_depth.TSDFVolume(DIMS, VS, ORIGIN, truncation=0.3)
    result = {"config": f"C2 {W}x{H}", "volume": "512x256x512 @ 0.1 m, u8 RGB", "stream": "one caller stream",
              "f": FOCAL, "baseline_m": BASELINE, "repeats": args.repeats, "iters": args.iters,
              "gpu": torch.cuda.get_device_name(0)}
    one = Integrator(vol, disp[:1], rgb[:1], w2c[:1], Q)
    eight = Integrator(vol, disp, rgb, w2c, Q)
    singles = [Integrator(vol, disp[f:f + 1], rgb[f:f + 1], w2c[f:f + 1], Q) for f in range(n)]
    nvox = DIMS[0] * DIMS[1] * DIMS[2]
    for name, fn, maps in (("integrate_n1", one, 1), ("integrate_n8", eight, n),
                           ("integrate_8x_n1", lambda: [s() for s in singles], n)):
        vol.reset()
        fn()
        torch.cuda.synchronize()
        measured = int(vol.weight.count_nonzero().item())
        t = time_graph(fn, args.iters, args.repeats, args.warmup)
        calls = 1 if name != "integrate_8x_n1" else n
        nbytes = maps * H * W * (4 + 3 + 12) + calls * 24 * measured
        t["measured_voxel_fraction"] = round(measured / nvox, 3)
        t["mbytes"] = round(nbytes / 1e6, 1)
        t["tb_per_s"] = round(nbytes / (t["us_median"] * 1e-6) / 1e12, 3)
        result[name] = t
    vol.reset()
    eight()
    cap = int(vol.extract_point_cloud_batched(1)[3].item())
    t = time_graph(lambda: vol.extract_point_cloud_batched(max(cap, 1)), args.iters, args.repeats, args.warmup)
    t["points"] = cap
    nbytes = 2 * 8 * nvox
    t["mbytes"] = round(nbytes / 1e6, 1)
    t["tb_per_s"] = round(nbytes / (t["us_median"] * 1e-6) / 1e12, 3)
    result["extract"] = t
    del vol
    torch.cuda.empty_cache()
    result["quality"] = quality()
    cfg = cuda_depth.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=0,
                                                 max_disparity=D - 1)
    sm = cuda_depth.StereoMatching(cfg, max_batch=64)
    gl = torch.from_numpy(rng.integers(0, 256, (32, H, W)).astype(np.float32)).cuda()
    gr = torch.roll(gl, -8, dims=2).contiguous()
    result["lr_n32"] = time_eager(lambda: sm.compute_disparity_map_batch_lr(gl, gr), max(2, args.iters // 2),
                                  args.repeats, args.warmup)
    result["integrate_n8_over_lr_n32"] = round(result["integrate_n8"]["us_median"] / result["lr_n32"]["us_median"], 3)
    torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
