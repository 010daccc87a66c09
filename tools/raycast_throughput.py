#!/usr/bin/env python3
"""Cost of ray casting a TSDF volume (smx_tsdf_raycast) at C2 (1242x375), on one caller stream:
    python tools/raycast_throughput.py [--repeats 7] [--iters 10]
The volume of tools/tsdf_throughput.py: 512x256x512 voxels of 0.1 m (67.1 M voxels, u8 RGB colour), the camera at the
centre of its -z face looking along +z, KITTI-like intrinsics; step = voxel_size and depth 0 .. the farthest corner
(58.7 m: 587 samples per ray), min_weight 1.  Times one view with all five outputs, one view with the disparity alone,
and 8 views in one call (the 8 poses of the filling maps, 0.5 m forward each), on three states of the volume:
    "maps"     filled by one call of the 8 synthetic C2 maps of tools/tsdf_throughput.py (depths uniform in 3..50 m: noise)
    "spheres"  the 32 analytic spheres of tools/mesh_throughput.py, every voxel measured
    "empty"    no voxel measured: every sample is skipped, the cost of the brick pass and of the jumps
and, in the same run on the same state, smx_tsdf_extract_points (normals and colours): the yardstick.  The aim is one
view in no more time than that full sweep of the volume.  Each timed step is captured `iters` times into one HIP graph
(no host overhead in the numbers), replayed after a warm-up, `repeats` times: the median and the spread (min, max) per
step.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np, torch, cuda_depth   # noqa: E401,E402
from cuda_depth import _native           # noqa: E402
import tsdf_throughput as tt             # noqa: E402


class Caster:
    """smx_tsdf_raycast of n views [n, 3, 4] (device) of vol into preallocated outputs, on the current stream."""

    def __init__(self, vol, Q, poses, z_max, all_outputs=True):
        self.vol, self.n, self.z_max = vol, poses.shape[0], z_max
        self.poses = torch.from_numpy(poses).cuda()
        n, H, W = self.n, tt.H, tt.W
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")  # noqa: E731
        self.disp = f(n, H, W)
        self.depth, self.normals, self.weight = (f(n, H, W), f(n, 3, H, W), f(n, H, W)) if all_outputs else (None,) * 3
        self.colors = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda") if all_outputs else None
        self.wsb = _native.LIB.smx_tsdf_raycast_workspace_bytes(*vol.dims)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        self.q = (C.c_float * 16)(*Q.reshape(-1).tolist())
        self.o = (C.c_float * 3)(*vol.origin)

    def __call__(self):
        v = self.vol
        nx, ny, nz = v.dims
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        cuda_depth.check(_native.LIB.smx_tsdf_raycast(
            0, nx, ny, nz, self.o, v.voxel_size, v.tsdf.data_ptr(), v.weight.data_ptr(), v.color.data_ptr(), 1.0, self.n,
            tt.H, tt.W, self.q, self.poses.data_ptr(), v.voxel_size, 0.0, self.z_max, -1.0, self.disp.data_ptr(),
            ptr(self.depth), ptr(self.normals), ptr(self.colors), ptr(self.weight), self.ws.data_ptr(), self.wsb,
            C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def measure(vol, Q, poses, z_max, args):
    probe = vol.extract_point_cloud_batched(1)
    points = max(int(probe[3].item()), 1)
    res = {"extract_points": tt.time_graph(lambda: vol.extract_point_cloud_batched(points), args.iters, args.repeats,
                                           args.warmup)}
    one = Caster(vol, Q, poses[:1], z_max)
    res["one_view"] = tt.time_graph(one, args.iters, args.repeats, args.warmup)
    res["one_view"]["hit_fraction"] = round(float((one.disp != -1.0).float().mean().item()), 3)
    res["one_view_disparity_only"] = tt.time_graph(Caster(vol, Q, poses[:1], z_max, False), args.iters, args.repeats,
                                                   args.warmup)
    res["eight_views"] = tt.time_graph(Caster(vol, Q, poses, z_max), args.iters, args.repeats, args.warmup)
    res["aim_us"] = res["extract_points"]["us_median"]
    res["aim_met"] = bool(res["one_view"]["us_median"] <= res["aim_us"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--states", default="empty,maps,spheres", help="the states of the volume to time, comma separated")
    args = ap.parse_args()
    H, W, n = tt.H, tt.W, 8
    rng = np.random.default_rng(0)
    z = rng.uniform(3.0, 50.0, (n, H, W))
    d = (tt.FOCAL * tt.BASELINE / z).astype(np.float32)
    d[rng.random((n, H, W)) < 0.10] = -1.0
    disp = torch.from_numpy(d).cuda()
    rgb = torch.from_numpy(rng.integers(0, 256, (n, 3, H, W)).astype(np.uint8)).cuda()
    Q = cuda_depth.reprojection_matrix(tt.FOCAL, W / 2.0, H / 2.0, tt.BASELINE)
    c2w = np.stack([np.eye(4)] * n)
    c2w[:, 2, 3] = 0.5 * np.arange(n)
    w2c = torch.from_numpy(cuda_depth.world_to_camera_poses(c2w)).cuda()
    poses = cuda_depth.camera_to_world_poses(c2w)
    vol = cuda_depth.TSDFVolume(tt.DIMS, tt.VS, tt.ORIGIN, truncation=0.3)
    nx, ny, nz = tt.DIMS
    *_, (_, z_max) = vol._check_render_args(Q, c2w, (H, W), 1.0, None, None, True, True, -1.0)
    result = {"volume": "512x256x512 @ 0.1 m, u8 RGB", "views": "C2 1242x375", "stream": "one caller stream",
              "samples_per_ray": int(np.floor(np.float32(z_max) / np.float32(tt.VS))) + 1, "repeats": args.repeats,
              "iters": args.iters, "gpu": torch.cuda.get_device_name(0)}
    states = args.states.split(",")
    if "empty" in states:
        result["empty"] = measure(vol, Q, poses, z_max, args)
    tt.Integrator(vol, disp, rgb, w2c, Q)()
    if "maps" in states:
        result["maps"] = measure(vol, Q, poses, z_max, args)
    if "spheres" not in states:
        print(json.dumps(result))
        return
    # a volume full of surface: 32 spheres of radius 40.3 voxels on a lattice of period 128, written into the state
    sq = [((torch.arange(m, device="cuda") % 128).float() - 63.5) ** 2 for m in (nz, ny, nx)]
    dist = torch.sqrt(sq[0][:, None, None] + sq[1][None, :, None] + sq[2][None, None, :]) - 40.3
    vol.tsdf.copy_(torch.clamp(dist / 3.0, -1.0, 1.0))
    vol.weight.fill_(1.0)
    del dist
    result["spheres"] = measure(vol, Q, poses, z_max, args)
    torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
