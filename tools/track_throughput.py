#!/usr/bin/env python3
"""Cost and quality of camera tracking (smx_track_camera) at C2 (1242x375), on one caller stream:
    python tools/track_throughput.py [--repeats 7] [--iters 10]
Cost: the volume of tools/raycast_throughput.py's "spheres" state (512x256x512 voxels of 0.1 m, 32 analytic spheres,
every voxel measured), the model view rendered from the camera at the centre of its -z face, the frame the library's
rendering from a pose 0.12 m and 0.6 degrees away; max_distance 0.5 m, depth 0 .. 60 m, no tolerance (every iteration of
a schedule runs).  Times, in the same run: the render of that one model view (disparity, depth and normals: what the track
reads) -- the yardstick: the aim is a default-schedule track in no more time than it; the default schedule
((4, 4), (2, 5), (1, 10)); ten iterations at stride 1; and one iteration split by difference: a call of zero iterations
(the launch that takes the poses in), an iteration at stride 32768 (one selected pixel: the floor of the two launches of
an iteration, with the solve) and an iteration at stride 1 (its accumulate launch is the rest).  Each timed step is
captured `iters` times into one HIP graph (no host overhead in the numbers), replayed after a warm-up, `repeats` times:
the median and the spread (min, max) per step.
Quality: the analytic sequence of tools/tsdf_throughput.py (a ground plane and three boxes from 12 poses at C2,
disparities with sigma = 0.5 px noise and 5 % outliers) fused into 0.1 m voxels at the true poses; every frame after the
first is tracked, before it is fused, against the volume so far from the previous frame's true pose; the error of the
tracked pose against the true one.  A reported figure, not a pass condition.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stereo-depth_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np, torch, cuda_depth   # noqa: E401,E402
from cuda_depth import _native           # noqa: E402
import track_ref                         # noqa: E402
import tsdf_ref                          # noqa: E402
import tsdf_throughput as tt             # noqa: E402

MAX_DISTANCE, DEPTH_RANGE = 0.5, (0.0, 60.0)


class Renderer:
    """smx_tsdf_raycast of one view (disparity, depth, normals) of vol into preallocated outputs, on the current stream."""

    def __init__(self, vol, Q, pose, z_max):
        self.vol, self.z_max = vol, z_max
        self.pose = torch.from_numpy(cuda_depth.camera_to_world_poses(pose)).cuda()
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")  # noqa: E731
        self.disp, self.depth, self.normals = f(1, tt.H, tt.W), f(1, tt.H, tt.W), f(1, 3, tt.H, tt.W)
        self.wsb = _native.LIB.smx_tsdf_raycast_workspace_bytes(*vol.dims)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        self.q = (C.c_float * 16)(*Q.reshape(-1).tolist())
        self.o = (C.c_float * 3)(*vol.origin)

    def __call__(self):
        v = self.vol
        nx, ny, nz = v.dims
        cuda_depth.check(_native.LIB.smx_tsdf_raycast(
            0, nx, ny, nz, self.o, v.voxel_size, v.tsdf.data_ptr(), v.weight.data_ptr(), None, 1.0, 1, tt.H, tt.W, self.q,
            self.pose.data_ptr(), v.voxel_size, 0.0, self.z_max, -1.0, self.disp.data_ptr(), self.depth.data_ptr(),
            self.normals.data_ptr(), None, None, self.ws.data_ptr(), self.wsb,
            C.c_void_p(torch.cuda.current_stream().cuda_stream)))


class Tracker:
    """smx_track_camera of one frame against a Renderer's view, from the view's pose, into preallocated outputs."""

    def __init__(self, frame, Q, view, model_pose, schedule):
        self.frame, self.view = frame, view
        self.q = (C.c_float * 16)(*Q.reshape(-1).tolist())
        self.pm = (C.c_float * 16)(*cuda_depth.projection_matrix(Q).reshape(-1).tolist())
        self.c2w = torch.from_numpy(cuda_depth.camera_to_world_poses(model_pose)).cuda()
        self.w2c = torch.from_numpy(cuda_depth.world_to_camera_poses(model_pose)).cuda()
        self.pose_out = torch.empty((1, 3, 4), dtype=torch.float32, device="cuda")
        self.info = torch.empty((1, 4), dtype=torch.int32, device="cuda")
        self.rms = torch.empty((1,), dtype=torch.float32, device="cuda")
        self.sums = torch.empty((1, 30), dtype=torch.float64, device="cuda")
        self.wsb = _native.LIB.smx_track_camera_workspace_bytes(1, tt.H, tt.W)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        flat = [int(v) for pair in schedule for v in pair]
        self.pairs, self.schedule = len(flat) // 2, (C.c_int32 * max(len(flat), 1))(*flat)

    def __call__(self):
        cuda_depth.check(_native.LIB.smx_track_camera(
            0, 1, tt.H, tt.W, self.frame.data_ptr(), None, self.q, 0.0, DEPTH_RANGE[0], DEPTH_RANGE[1], -1.0, tt.H, tt.W,
            self.view.depth.data_ptr(), self.view.normals.data_ptr(), self.q, self.pm, self.c2w.data_ptr(),
            self.w2c.data_ptr(), self.c2w.data_ptr(), self.pairs, self.schedule, MAX_DISTANCE, 100, 1e-3, 0.0, 0.0,
            self.pose_out.data_ptr(), self.info.data_ptr(), self.rms.data_ptr(), self.sums.data_ptr(), self.ws.data_ptr(),
            self.wsb, C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def outcome(self, true_pose):
        torch.cuda.synchronize()
        lost, iterations, inliers, accepted = (int(v) for v in self.info[0].tolist())
        m, deg = track_ref.pose_error(self.pose_out[0].cpu().numpy(), true_pose)
        return {"lost": lost, "iterations": iterations, "inliers": inliers, "accepted": accepted,
                "error_m": round(m, 5), "error_deg": round(deg, 4)}


def cost(args):
    H, W = tt.H, tt.W
    Q = cuda_depth.reprojection_matrix(tt.FOCAL, W / 2.0, H / 2.0, tt.BASELINE)
    vol = cuda_depth.TSDFVolume(tt.DIMS, tt.VS, tt.ORIGIN, truncation=0.3, color=False)
    nx, ny, nz = tt.DIMS
    sq = [((torch.arange(m, device="cuda") % 128).float() - 63.5) ** 2 for m in (nz, ny, nx)]
    dist = torch.sqrt(sq[0][:, None, None] + sq[1][None, :, None] + sq[2][None, None, :]) - 40.3
    vol.tsdf.copy_(torch.clamp(dist / 3.0, -1.0, 1.0))
    vol.weight.fill_(1.0)
    del dist
    model_pose = np.eye(4)
    ang = np.radians(0.6)
    true_pose = np.eye(4)
    true_pose[:3, :3] = [[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]
    true_pose[:3, 3] = [0.08, -0.04, 0.08]
    *_, (_, z_max) = vol._check_render_args(Q, np.stack([model_pose, true_pose]), (H, W), 1.0, None, None, True, False, -1.0)
    seen = Renderer(vol, Q, true_pose, z_max)
    seen()
    frame = seen.disp.clone()
    view = Renderer(vol, Q, model_pose, z_max)
    res = {"render_model_view": tt.time_graph(view, args.iters, args.repeats, args.warmup)}
    res["render_model_view"]["hit_fraction"] = round(float((view.disp != -1.0).float().mean().item()), 3)
    start_m, start_deg = track_ref.pose_error(model_pose, true_pose)
    res["start_error_m"], res["start_error_deg"] = round(start_m, 5), round(start_deg, 4)
    for name, schedule in (("default_schedule", track_ref.DEFAULT_SCHEDULE), ("ten_at_stride_1", ((1, 10),)),
                           ("zero_iterations", ()), ("one_at_stride_32768", ((32768, 1),)), ("one_at_stride_1", ((1, 1),)),
                           ("one_at_stride_2", ((2, 1),)), ("one_at_stride_4", ((4, 1),))):
        tracker = Tracker(frame, Q, view, model_pose, schedule)
        res[name] = tt.time_graph(tracker, args.iters, args.repeats, args.warmup)
        res[name].update(tracker.outcome(true_pose))
    res["aim_us"] = res["render_model_view"]["us_median"]
    res["aim_met"] = bool(res["default_schedule"]["us_median"] <= res["aim_us"])
    return res


def quality(n_poses=12):
    scene = tsdf_ref.Scene(ground_y=1.65, boxes=[((-3.0, -0.2, 8.0), (-1.0, 1.65, 10.0)),
                                                 ((1.0, -0.5, 12.0), (3.5, 1.65, 14.0)),
                                                 ((-2.0, 0.2, 16.0), (1.0, 1.65, 18.0))])
    H, W = tt.H, tt.W
    dims, vs, origin = (128, 48, 192), 0.1, (-6.4, -3.0, 3.0)
    Q = cuda_depth.reprojection_matrix(tt.FOCAL, W / 2.0, H / 2.0, tt.BASELINE)
    rng = np.random.default_rng(7)
    poses = np.stack([tsdf_ref.look_at((rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1), 0.25 * i),
                                       (rng.uniform(-0.5, 0.5), 0.5, 0.25 * i + 20.0)) for i in range(n_poses)])
    vol = cuda_depth.TSDFVolume(dims, vs, origin, color=False)
    frames = []
    for i, pose in enumerate(poses):
        d = scene.render(pose, H, W, tt.FOCAL, W / 2.0, H / 2.0, tt.BASELINE)
        ok = d > 0
        d[ok] += rng.normal(0.0, 0.5, int(ok.sum())).astype(np.float32)
        out = ok & (rng.random(d.shape) < 0.05)
        d[out] = rng.uniform(1.0, 96.0, int(out.sum())).astype(np.float32)
        td = torch.from_numpy(d).cuda()
        if i > 0:
            found = vol.track(td, Q, poses[i - 1], max_distance=1.0, depth_range=(0.0, 40.0))
            m, deg = track_ref.pose_error(found.pose.cpu().numpy(), pose)
            m0, deg0 = track_ref.pose_error(poses[i - 1], pose)
            frames.append({"lost": int(found.lost), "inliers": int(found.inliers), "start_m": round(m0, 4),
                           "start_deg": round(deg0, 3), "error_m": round(m, 4), "error_deg": round(deg, 3)})
        vol.integrate(td, Q, pose)
    good = [f for f in frames if not f["lost"]]
    res = {"poses": n_poses, "voxel_m": vs, "noise_px": 0.5, "outliers": 0.05, "tracked": len(good),
           "lost": len(frames) - len(good), "frames": frames}
    if good:
        res["error_m_median"] = round(float(np.median([f["error_m"] for f in good])), 4)
        res["error_m_max"] = round(max(f["error_m"] for f in good), 4)
        res["error_deg_median"] = round(float(np.median([f["error_deg"] for f in good])), 3)
        res["error_deg_max"] = round(max(f["error_deg"] for f in good), 3)
        res["start_m_median"] = round(float(np.median([f["start_m"] for f in good])), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-quality", action="store_true")
    args = ap.parse_args()
    result = {"volume": "512x256x512 @ 0.1 m, spheres", "frames": "C2 1242x375", "stream": "one caller stream",
              "repeats": args.repeats, "iters": args.iters, "gpu": torch.cuda.get_device_name(0)}
    result.update(cost(args))
    torch.cuda.empty_cache()
    if not args.skip_quality:
        result["quality"] = quality()
    torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
