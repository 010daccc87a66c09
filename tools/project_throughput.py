#!/usr/bin/env python3
"""Cost of projecting point clouds back into camera views at C2 (1242x375) with KITTI-like intrinsics (f = 721.5 px,
B = 0.54 m), on one caller stream:
    python tools/project_throughput.py [--repeats 7] [--iters 20]
Synthetic maps as in tools/points_throughput.py: disparities uniform in 1..96 px with 10 % invalid pixels.  The 32 maps
become 32 clouds (smx_reproject_points, timed here as the yardstick, without colour), which smx_project_points
(cuda_depth.project_points_batched, index plane on, depth plane off) takes back into 32 views
  - at the identity pose and at a pose 0.33 m forward, the rows in pixel order as reprojection leaves them: consecutive
    lanes hit consecutive keys;
  - at the forward pose with every cloud's rows randomly permuted: the scattered-atomic case, reported without an aim;
  - at the forward pose with radius 0, 1 and 2.
Each timed call is captured `iters` times into one HIP graph and replayed `repeats` times after a warm-up (the scheme of
tools/points_throughput.py): the median and the spread of the time per call.  The aim for the two pixel-order cases is
the reprojection's time multiplied by the ratio of counted traffic, computed from the actual counts: per point the
projection reads 12 B, sends its 8 B key and, for a winner, gathers 12 B in the resolve; per pixel it clears an 8 B key,
reads it in the resolve and writes 8 B (disparity and index).  The reprojection reads 4 B per pixel twice (its count
and scatter passes) and writes 12 B per point.  aim_met is printed either way.  One LiDAR-like scan of 120 000 returns
in sensor order (64 rings x 1875 azimuths) is projected with the KITTI calibration, and
helpers.kitti_calibration.velodyne_depth_map is timed on the host beside it, in this process.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd"), os.path.join(ROOT, "tools")]
import numpy as np, torch, cuda_depth   # noqa: E401,E402
from points_throughput import FOCAL, BASELINE, H, W, stats, time_graph   # noqa: E402

CAM2CAM = """R_rect_00: 9.999239e-01 9.837760e-03 -7.445048e-03 -9.869795e-03 9.999421e-01 -4.278459e-03 7.402527e-03 4.351614e-03 9.999631e-01
P_rect_02: 7.215377e+02 0.000000e+00 6.095593e+02 4.485728e+01 0.000000e+00 7.215377e+02 1.728540e+02 2.163791e-01 0.000000e+00 0.000000e+00 1.000000e+00 2.745884e-03
P_rect_03: 7.215377e+02 0.000000e+00 6.095593e+02 -3.395242e+02 0.000000e+00 7.215377e+02 1.728540e+02 2.199936e+00 0.000000e+00 0.000000e+00 1.000000e+00 2.729905e-03
"""
VELO2CAM = """R: 7.533745e-03 -9.999714e-01 -6.166020e-04 1.480249e-02 7.280733e-04 -9.998902e-01 9.998621e-01 7.523790e-03 1.480755e-02
T: -4.069766e-03 -7.631618e-02 -2.717806e-01
"""


def lidar_scan(rng, rings=64, azimuths=1875):
    """[rings * azimuths, 4] float32 in sensor order (azimuth by azimuth, ring by ring inside): ranges of a ground plane
    1.7 m below the sensor and walls 5..60 m away, elevation +2..-24.8 degrees, the full turn."""
    az = np.repeat(np.linspace(-np.pi, np.pi, azimuths, endpoint=False), rings)
    el = np.tile(np.deg2rad(np.linspace(2.0, -24.8, rings)), azimuths)
    wall = np.repeat(rng.uniform(5.0, 60.0, azimuths), rings)
    with np.errstate(divide="ignore"):
        ground = np.where(el < 0, 1.7 / np.maximum(np.sin(-el), 1e-6), np.inf)
    r = np.minimum(wall, ground) + rng.normal(0, 0.02, az.size)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el),
                     rng.uniform(0, 1, az.size)], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    n = 32
    d = rng.uniform(1.0, 96.0, (n, H, W)).astype(np.float32)
    d[rng.random((n, H, W)) < 0.10] = -1.0
    disp = torch.from_numpy(d).cuda()
    Q = cuda_depth.reprojection_matrix(FOCAL, W / 2.0, H / 2.0, BASELINE)
    result = {"config": f"C2 {W}x{H}", "stream": "one caller stream", "f": FOCAL, "baseline_m": BASELINE, "clouds": n,
              "invalid_fraction": 0.1, "repeats": args.repeats, "iters": args.iters, "gpu": torch.cuda.get_device_name(0)}
    points, _, _, offsets, _ = cuda_depth.reproject_to_3d_batched(disp, Q, indices=False)
    off = offsets.cpu().numpy()
    pts, px = int(off[-1]), n * H * W
    result["points"], result["pixels"] = pts, px
    result["reproject_n32_no_colour"] = time_graph(
        lambda: cuda_depth.reproject_to_3d_batched(disp, Q, indices=False), args.iters, args.repeats, args.warmup)
    project_bytes = pts * (12 + 8 + 12) + px * (8 + 8 + 8)
    reproject_bytes = px * 2 * 4 + pts * 12
    ratio = project_bytes / reproject_bytes
    result["traffic"] = {"project_mbytes": round(project_bytes / 1e6, 1), "reproject_mbytes": round(reproject_bytes / 1e6, 1),
                         "ratio": round(ratio, 3)}
    aim = result["reproject_n32_no_colour"]["us_median"] * ratio
    result["aim_us"] = round(aim, 2)

    def pose(forward):
        m = np.tile(np.eye(4), (n, 1, 1))
        m[:, 2, 3] = forward
        return torch.from_numpy(cuda_depth.world_to_camera_poses(m)).cuda()

    identity, forward = pose(0.0), pose(0.33)
    perm = np.concatenate([off[f] + rng.permutation(off[f + 1] - off[f]) for f in range(n)] + [np.arange(pts, px)])
    shuffled = points[torch.from_numpy(perm).cuda()].contiguous()

    def timed(cloud, poses, radius=0):
        t = time_graph(lambda: cuda_depth.project_points_batched(cloud, offsets, Q, None, (H, W), radius=radius,
                                                                 world_to_camera=poses), args.iters, args.repeats, args.warmup)
        disp_out, index, _ = cuda_depth.project_points_batched(cloud, offsets, Q, None, (H, W), radius=radius,
                                                               world_to_camera=poses)
        t["pixels_hit"] = int((index >= 0).sum().item())
        return t

    for name, poses in (("identity", identity), ("forward_0.33m", forward)):
        t = timed(points, poses)
        t["over_aim"] = round(t["us_median"] / aim, 3)
        t["aim_met"] = bool(t["us_median"] <= aim)
        result[f"project_n32_{name}"] = t
    result["project_n32_forward_0.33m_permuted_rows"] = timed(shuffled, forward)
    for radius in (1, 2):
        result[f"project_n32_forward_0.33m_radius{radius}"] = timed(points, forward, radius)

    # one LiDAR-like scan in sensor order, device against host
    from helpers.kitti_calibration import velodyne_depth_map, velodyne_disparity_map_device, velodyne_projection
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "calib_cam_to_cam.txt"), "w").write(CAM2CAM)
        open(os.path.join(tmp, "calib_velo_to_cam.txt"), "w").write(VELO2CAM)
        velo = os.path.join(tmp, "scan.bin")
        scan = lidar_scan(rng)
        scan.tofile(velo)
        M, P = velodyne_projection(tmp)
        front = scan[scan[:, 0] >= 0]
        cloud = torch.from_numpy(np.ascontiguousarray(front[:, :3])).cuda()
        one = torch.tensor([0, len(front)], dtype=torch.int32).cuda()
        m_dev = torch.from_numpy(M[None]).cuda()
        t = time_graph(lambda: cuda_depth.project_points_batched(cloud, one, None, None, (H, W), P=P, world_to_camera=m_dev,
                                                                 invalid_disparity=0.0), args.iters, args.repeats, args.warmup)
        t["returns"], t["returns_in_front"] = len(scan), len(front)
        gt = velodyne_disparity_map_device(tmp, velo, (H, W), "cuda")
        t["pixels_hit"] = int((gt > 0).sum().item())
        result["lidar_scan_sensor_order"] = t
        whole, host = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            velodyne_disparity_map_device(tmp, velo, (H, W), "cuda")
            torch.cuda.synchronize()
            whole.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter()
            velodyne_depth_map(tmp, velo, (H, W), vel_depth=True)
            host.append((time.perf_counter() - t0) * 1e6)
        result["lidar_ground_truth_device_with_file_read_and_upload"] = stats(whole)
        result["lidar_ground_truth_host_velodyne_depth_map"] = stats(host)
    torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
