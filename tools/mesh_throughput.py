#!/usr/bin/env python3
"""Cost of the triangle-mesh extraction of a TSDF volume, on one caller stream:
    python tools/mesh_throughput.py [--repeats 7] [--iters 10]
The volume of tools/tsdf_throughput.py: 512x256x512 voxels of 0.1 m (67.1 M voxels, u8 RGB colour) filled by one call of
the same 8 synthetic C2 maps (depths uniform in 3..50 m, 10 % invalid pixels, 0.5 m forward per frame).  Times, in the
same run, smx_tsdf_extract_points alone (normals and colours: the yardstick), smx_tsdf_extract_triangles alone, and the
whole TSDFVolume.extract_triangle_mesh_batched (both, with its allocations).  The synthetic maps are noise in depth, so
that volume has many crossings but hardly a cell whose eight voxels all lie in a truncation band; "spheres" repeats the
three measurements on the same volume filled with 32 analytic spheres, where every crossing belongs to triangles.
Each timed step is captured `iters` times into one HIP graph (no host overhead in the numbers), replayed after a
warm-up, `repeats` times: the median and the spread (min, max) per step.
Bytes counted for the points: tsdf and weight read twice (16 B per voxel) and 27 B written per point; for the triangles:
tsdf and weight read once, the byte per voxel written once and read twice (11 B per voxel), the word per 64 voxels
written once and read once, and 12 B written per triangle.  The aim for the triangle pass is the measured time of the
point extraction times the ratio of those byte counts.  Prints one JSON line."""
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


def measure(vol, args):
    nx, ny, nz = vol.dims
    nvox = nx * ny * nz
    probe = vol.extract_triangle_mesh_batched(1, 1)
    points, triangles = int(probe[3].item()), int(probe[5].item())
    vcap, tcap = max(points, 1), max(triangles, 1)
    result = {"points": points, "triangles": triangles}

    t = tt.time_graph(lambda: vol.extract_point_cloud_batched(vcap), args.iters, args.repeats, args.warmup)
    pbytes = 16 * nvox + 27 * points
    t["mbytes"] = round(pbytes / 1e6, 1)
    t["tb_per_s"] = round(pbytes / (t["us_median"] * 1e-6) / 1e12, 3)
    result["extract_points"] = t

    tris = torch.empty((tcap, 3), dtype=torch.int32, device="cuda")
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    wsb = _native.LIB.smx_tsdf_extract_triangles_workspace_bytes(nx, ny, nz)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")

    def triangles_only():
        cuda_depth.check(_native.LIB.smx_tsdf_extract_triangles(
            0, nx, ny, nz, vol.tsdf.data_ptr(), vol.weight.data_ptr(), 1.0, tcap, tris.data_ptr(), count.data_ptr(),
            ws.data_ptr(), wsb, C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    t = tt.time_graph(triangles_only, args.iters, args.repeats, args.warmup)
    tbytes = 11 * nvox + 8 * (nvox // 64) + 12 * triangles
    t["mbytes"] = round(tbytes / 1e6, 1)
    t["tb_per_s"] = round(tbytes / (t["us_median"] * 1e-6) / 1e12, 3)
    t["workspace_mbytes"] = round(wsb / 1e6, 1)
    result["extract_triangles"] = t
    assert int(count.item()) == triangles

    result["extract_triangle_mesh_batched"] = tt.time_graph(lambda: vol.extract_triangle_mesh_batched(vcap, tcap),
                                                            args.iters, args.repeats, args.warmup)
    ratio = tbytes / pbytes
    aim = ratio * result["extract_points"]["us_median"]
    result["traffic_ratio"] = round(ratio, 3)
    result["aim_us"] = round(aim, 1)
    result["aim_met"] = bool(result["extract_triangles"]["us_median"] <= aim)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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
    vol = cuda_depth.TSDFVolume(tt.DIMS, tt.VS, tt.ORIGIN, truncation=0.3)
    tt.Integrator(vol, disp, rgb, w2c, Q)()
    nx, ny, nz = tt.DIMS
    result = {"volume": "512x256x512 @ 0.1 m, u8 RGB, 8 C2 maps", "stream": "one caller stream",
              "repeats": args.repeats, "iters": args.iters, "gpu": torch.cuda.get_device_name(0)}
    result.update(measure(vol, args))
    # a volume full of surface: 32 spheres of radius 40.3 voxels on a lattice of period 128, written into the state
    sq = [((torch.arange(m, device="cuda") % 128).float() - 63.5) ** 2 for m in (nz, ny, nx)]
    dist = torch.sqrt(sq[0][:, None, None] + sq[1][None, :, None] + sq[2][None, None, :]) - 40.3
    vol.tsdf.copy_(torch.clamp(dist / 3.0, -1.0, 1.0))
    vol.weight.fill_(1.0)
    del dist
    result["spheres"] = measure(vol, args)
    torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
