#!/usr/bin/env python3
"""Cost and quality of camera tracking with the photometric term (smx_track_camera_photometric) at C2 (1242x375), on one
caller stream:
    python tools/track_photo_throughput.py [--repeats 7] [--iters 10]
Cost: tools/track_throughput.py's set-up -- the "spheres" volume (512x256x512 voxels of 0.1 m), its model view, the frame
rendered 0.12 m and 0.6 degrees away -- with intensity planes that are one smooth function of the pixel for the frame and
for the model, so that every geometric inlier with its four taps inside the view is a photometric inlier and pays for the
whole term.  Times, in the same run and each captured `iters` times into one HIP graph: the geometric default-schedule
track (smx_track_camera), the joint one, and one iteration at stride 1 of each.  The aim is the geometric time times the
ratio of the two rules' loads per inlier pixel from memory that differs from lane to lane (LOADS below, counted from the
rules in include/stereo_mi355x.h); the geometric tracker is bound by a latency chain per lane rather than by its loads
(DESIGN.md), so the ratio may be pessimistic.  A reported figure, met or missed.
Quality: tools/track_throughput.py's analytic sequence (a ground plane and three boxes from 12 poses, noisy disparities)
with a texture painted on the scene -- a smooth function of the world point, the frames' gray images -- fused into a colour
volume; every frame after the first is tracked, before it is fused, with and without the term.  Then a textured wall: one
plane facing the camera, which the geometric tracker loses.  Reported figures, not pass conditions.  Prints one JSON line."""
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
import track_throughput as base          # noqa: E402
import tsdf_ref                          # noqa: E402
import tsdf_throughput as tt             # noqa: E402

# loads per inlier pixel whose address differs from lane to lane (the matrices and poses are the same for a wave)
LOADS = {"geometric": {"disp": 1, "model_depth": 1, "model_normals": 3},
         "photometric": {"frame_intensity": 1, "model_depth taps": 4, "model_intensity taps": 4}}
WEIGHT, MAX_DIFFERENCE = 0.01, 30.0


class PhotoTracker(base.Tracker):
    """smx_track_camera_photometric on a Tracker's operands and two intensity planes."""

    def __init__(self, frame, Q, view, model_pose, schedule, frame_int, model_int):
        super().__init__(frame, Q, view, model_pose, schedule)
        self.frame_int, self.model_int = frame_int, model_int
        self.sums = torch.empty((1, 33), dtype=torch.float64, device="cuda")
        self.pinfo = torch.empty((1, 2), dtype=torch.int32, device="cuda")
        self.prms = torch.empty((1,), dtype=torch.float32, device="cuda")
        self.wsb = _native.LIB.smx_track_camera_photometric_workspace_bytes(1, tt.H, tt.W)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")

    def __call__(self):
        cuda_depth.check(_native.LIB.smx_track_camera_photometric(
            0, 1, tt.H, tt.W, self.frame.data_ptr(), None, self.q, 0.0, base.DEPTH_RANGE[0], base.DEPTH_RANGE[1], -1.0,
            tt.H, tt.W, self.view.depth.data_ptr(), self.view.normals.data_ptr(), self.q, self.pm, self.c2w.data_ptr(),
            self.w2c.data_ptr(), self.c2w.data_ptr(), self.pairs, self.schedule, base.MAX_DISTANCE, 100, 1e-3, 0.0, 0.0,
            self.frame_int.data_ptr(), self.model_int.data_ptr(), WEIGHT, MAX_DIFFERENCE, self.pose_out.data_ptr(),
            self.info.data_ptr(), self.rms.data_ptr(), self.sums.data_ptr(), self.pinfo.data_ptr(), self.prms.data_ptr(),
            self.ws.data_ptr(), self.wsb, C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def outcome(self, true_pose):
        out = super().outcome(true_pose)
        out["photometric_inliers"] = int(self.pinfo[0, 0])
        return out


def cost_operands():
    """(Q, frame, view, model_pose, true_pose, plane [1, H, W]): the C2 frame, the spheres volume's model view and the
    smooth intensity plane that the cost runs read."""
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
    seen = base.Renderer(vol, Q, true_pose, z_max)
    seen()
    frame = seen.disp.clone()
    view = base.Renderer(vol, Q, model_pose, z_max)
    view()
    v, u = torch.meshgrid(torch.arange(H, device="cuda").float(), torch.arange(W, device="cuda").float(), indexing="ij")
    plane = (128.0 + 40.0 * torch.sin(0.021 * u) + 30.0 * torch.cos(0.017 * v))[None].contiguous()
    return Q, frame, view, model_pose, true_pose, plane


def cost(args):
    Q, frame, view, model_pose, true_pose, plane = cost_operands()
    res = {}
    for name, schedule in (("default_schedule", track_ref.DEFAULT_SCHEDULE), ("one_at_stride_1", ((1, 1),))):
        geo = base.Tracker(frame, Q, view, model_pose, schedule)
        res["geometric_" + name] = tt.time_graph(geo, args.iters, args.repeats, args.warmup)
        res["geometric_" + name].update(geo.outcome(true_pose))
        joint = PhotoTracker(frame, Q, view, model_pose, schedule, plane, plane.clone())
        res["joint_" + name] = tt.time_graph(joint, args.iters, args.repeats, args.warmup)
        res["joint_" + name].update(joint.outcome(true_pose))
    g, p = sum(LOADS["geometric"].values()), sum(LOADS["photometric"].values())
    res["loads_per_inlier"] = {"geometric": g, "joint": g + p}
    res["aim_us"] = round(res["geometric_default_schedule"]["us_median"] * (g + p) / g, 2)
    res["aim_met"] = bool(res["joint_default_schedule"]["us_median"] <= res["aim_us"])
    res["joint_over_geometric"] = round(res["joint_default_schedule"]["us_median"] /
                                        res["geometric_default_schedule"]["us_median"], 3)
    return res


def texture(p):
    """The paint of a world point [..., 3]: smooth at the scale of the 0.1 m voxels."""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return 128.0 + 50.0 * np.sin(1.3 * x + 0.7 * y) * np.cos(0.9 * z + 0.4 * y) + 40.0 * np.sin(0.8 * x - 1.1 * z + 2.0 * y)


def painted(scene, pose, rng, noise_px, outliers):
    """(noisy disparity [H, W] f32, gray image [H, W] u8) of the scene from pose; the image is painted at the exact hit."""
    H, W = tt.H, tt.W
    d = scene.render(pose, H, W, tt.FOCAL, W / 2.0, H / 2.0, tt.BASELINE)
    ok = d > 0
    with np.errstate(divide="ignore"):
        z = np.where(ok, tt.FOCAL * tt.BASELINE / d.astype(np.float64), 0.0)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cam = np.stack([(u - W / 2.0) / tt.FOCAL * z, (v - H / 2.0) / tt.FOCAL * z, z], -1)
    m = np.asarray(pose, np.float64)
    gray = np.where(ok, np.clip(np.rint(texture(cam @ m[:3, :3].T + m[:3, 3])), 0, 255), 0).astype(np.uint8)
    d[ok] += rng.normal(0.0, noise_px, int(ok.sum())).astype(np.float32)
    out = ok & (rng.random(d.shape) < outliers)
    d[out] = rng.uniform(1.0, 96.0, int(out.sum())).astype(np.float32)
    return d, gray


def sequence(scene, poses, dims, vs, origin, variants=None, **track_args):
    """Tracks every frame after the first against the colour volume so far from the previous true pose, with and without
    the term (or once per entry of variants: name -> track arguments on top of the term's), then fuses it at its true
    pose."""
    Q = cuda_depth.reprojection_matrix(tt.FOCAL, tt.W / 2.0, tt.H / 2.0, tt.BASELINE)
    rng = np.random.default_rng(7)
    vol = cuda_depth.TSDFVolume(dims, vs, origin)
    variants = {"joint": {}} if variants is None else variants
    rows = {name: [] for name in ("geometric",) + tuple(variants)}
    for i, pose in enumerate(poses):
        d, gray = painted(scene, pose, rng, 0.5, 0.05)
        td, tg = torch.from_numpy(d).cuda(), torch.from_numpy(gray).cuda()
        if i > 0:
            term = dict(image=tg, photometric_weight=WEIGHT, max_intensity_difference=MAX_DIFFERENCE)
            for name, extra in [("geometric", {})] + [(k, dict(term, **v)) for k, v in variants.items()]:
                found = vol.track(td, Q, poses[i - 1], **track_args, **extra)
                m, deg = track_ref.pose_error(found.pose.cpu().numpy(), pose)
                rows[name].append({"lost": int(found.lost), "error_m": round(m, 4), "error_deg": round(deg, 3)})
        vol.integrate(td, Q, pose, image=tg[None].expand(3, -1, -1).contiguous())
    res = {}
    for name, frames in rows.items():
        good = [f for f in frames if not f["lost"]]
        res[name] = {"tracked": len(good), "lost": len(frames) - len(good)}
        if good:
            res[name].update(error_m_median=round(float(np.median([f["error_m"] for f in good])), 4),
                             error_m_max=round(max(f["error_m"] for f in good), 4),
                             error_deg_median=round(float(np.median([f["error_deg"] for f in good])), 3),
                             error_deg_max=round(max(f["error_deg"] for f in good), 3))
    starts = [track_ref.pose_error(a, b) for a, b in zip(poses[:-1], poses[1:])]
    res["start_m_median"] = round(float(np.median([s[0] for s in starts])), 4)
    res["start_deg_median"] = round(float(np.median([s[1] for s in starts])), 3)
    return res


def analytic_sequence(n_poses=12):
    """sequence()'s arguments for the ground plane and three boxes seen from n_poses poses."""
    rng = np.random.default_rng(7)
    scene = tsdf_ref.Scene(ground_y=1.65, boxes=[((-3.0, -0.2, 8.0), (-1.0, 1.65, 10.0)),
                                                 ((1.0, -0.5, 12.0), (3.5, 1.65, 14.0)),
                                                 ((-2.0, 0.2, 16.0), (1.0, 1.65, 18.0))])
    poses = np.stack([tsdf_ref.look_at((rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1), 0.25 * i),
                                       (rng.uniform(-0.5, 0.5), 0.5, 0.25 * i + 20.0)) for i in range(n_poses)])
    return scene, poses, (128, 48, 192), 0.1, (-6.4, -3.0, 3.0)


def textured_wall():
    """sequence()'s arguments for a wall 8 m ahead that fills the view; the camera drifts sideways, 5 cm and a fifth of a
    degree a frame."""
    wall = tsdf_ref.Scene(ground_y=1000.0, boxes=[((-40.0, -40.0, 8.0), (40.0, 40.0, 9.0))])
    steps = np.stack([tsdf_ref.look_at((0.05 * i, -0.02 * i, 0.01 * i), (0.05 * i + 0.03 * i, -0.02 * i, 8.0))
                      for i in range(6)])
    return wall, steps, (192, 64, 32), 0.1, (-9.6, -3.2, 6.5)


def quality(n_poses=12, variants=None):
    return {"analytic_sequence": sequence(*analytic_sequence(n_poses), variants=variants, max_distance=1.0, depth_range=(0.0, 40.0)),
            "textured_wall": sequence(*textured_wall(), variants=variants, max_distance=1.0, depth_range=(0.0, 40.0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-quality", action="store_true")
    args = ap.parse_args()
    result = {"volume": "512x256x512 @ 0.1 m, spheres", "frames": "C2 1242x375", "stream": "one caller stream",
              "repeats": args.repeats, "iters": args.iters, "weight": WEIGHT, "max_intensity_difference": MAX_DIFFERENCE,
              "gpu": torch.cuda.get_device_name(0)}
    result.update(cost(args))
    torch.cuda.empty_cache()
    if not args.skip_quality:
        result["quality"] = quality()
    torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
