"""KITTI raw-drive calibration files and velodyne ground truth ("next" row f4).

Behavioural restatement of /root/reference/src/python/helpers/velodyne_points_helpers.py:9-96
(itself the monodepth evaluation utility): `calib_*.txt` parsing, focal length / baseline of the
colour pair (cameras 2 and 3) and the sparse depth map obtained by projecting a velodyne scan
into an image.  Vectorised (sort + segmented minimum) instead of the reference's per-duplicate
Python loop.  The reference's own function does not run on this image's numpy (it uses the
`np.int` alias removed in numpy 1.24), so this module is checked against an independent
loop restatement in tests/test_kitti_camera.py: parity unpinned by the reference.
"""
from __future__ import annotations

import os
from typing import Dict, Tuple, Union

import numpy as np

_NUMERIC = set("0123456789.e+- ")


def read_calibration(path: str) -> Dict[str, Union[str, np.ndarray]]:
    """`key: v0 v1 ...` lines -> float arrays; lines that are not purely numeric stay strings
    (velodyne_points_helpers.py:31-47)."""
    out: Dict[str, Union[str, np.ndarray]] = {}
    with open(path, "r") as f:
        for line in f:
            if ":" not in line:
                continue
            key, text = line.split(":", 1)
            text = text.strip()
            out[key] = text
            if text and _NUMERIC.issuperset(text):
                try:
                    out[key] = np.array([float(tok) for tok in text.split(" ")])
                except ValueError:
                    pass
    return out


def focal_length_and_baseline(calib_dir: str) -> Tuple[float, float]:
    """Focal length of camera 2 and the distance between cameras 2 and 3
    (velodyne_points_helpers.py:9-21: t_x / -f of each rectified projection matrix)."""
    cam = read_calibration(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    p2 = np.asarray(cam["P_rect_02"]).reshape(3, 4)
    p3 = np.asarray(cam["P_rect_03"]).reshape(3, 4)
    offset2 = p2[0, 3] / -p2[0, 0]
    offset3 = p3[0, 3] / -p3[0, 0]
    return float(p2[0, 0]), float(offset3 - offset2)


def stereo_rectification(calib_dir: str, cams: Tuple[int, int] = (2, 3), **kwargs):
    """cuda_depth.StereoRectification of a raw ("extract") drive's camera pair from calib_cam_to_cam.txt: for camera x,
    the map of K_0x, D_0x (k1 k2 p1 p2 k3), R_rect_0x and P_rect_0x, from the raw size S_0x to the rectified size
    S_rect_0x (both stored as width height).  kwargs: border_mode, border_value, device."""
    import cuda_depth
    cal = read_calibration(os.path.join(calib_dir, "calib_cam_to_cam.txt"))

    def size(key: str) -> Tuple[int, int]:
        w, h = (int(round(float(v))) for v in np.asarray(cal[key]).reshape(2))
        return h, w

    in_shapes = {size(f"S_0{c}") for c in cams}
    out_shapes = {size(f"S_rect_0{c}") for c in cams}
    if len(in_shapes) != 1 or len(out_shapes) != 1:
        raise ValueError(f"cameras {cams} differ in raw or rectified size: {sorted(in_shapes)} / {sorted(out_shapes)}")
    in_shape, out_shape = in_shapes.pop(), out_shapes.pop()
    geometry = [(np.asarray(cal[f"K_0{c}"]).reshape(3, 3), np.asarray(cal[f"D_0{c}"]).reshape(5),
                 np.asarray(cal[f"R_rect_0{c}"]).reshape(3, 3), np.asarray(cal[f"P_rect_0{c}"]).reshape(3, 4))
                for c in cams]
    return cuda_depth.StereoRectification.from_calibration(geometry[0], geometry[1], in_shape, out_shape, **kwargs)


def velodyne_to_image_projection(calib_dir: str, cam: int = 2) -> np.ndarray:
    """3x4 matrix taking homogeneous velodyne points to pixels of rectified camera `cam`
    (velodyne_points_helpers.py:58-68)."""
    cam2cam = read_calibration(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    velo2cam = read_calibration(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
    rigid = np.eye(4)
    rigid[:3, :3] = np.asarray(velo2cam["R"]).reshape(3, 3)
    rigid[:3, 3] = np.asarray(velo2cam["T"])
    rectify = np.eye(4)
    rectify[:3, :3] = np.asarray(cam2cam["R_rect_00"]).reshape(3, 3)
    project = np.asarray(cam2cam["P_rect_0" + str(cam)]).reshape(3, 4)
    return project @ rectify @ rigid


def load_velodyne_scan(path: str) -> np.ndarray:
    """[N, 4] float32 (forward, left, up, 1): reflectance replaced by the homogeneous 1
    (velodyne_points_helpers.py:24-28)."""
    pts = np.fromfile(path, dtype=np.float32).reshape(-1, 4)
    pts[:, 3] = 1.0
    return pts


def velodyne_depth_map(calib_dir: str, velo_file_name: str, im_shape: Tuple[int, int], cam: int = 2,
                       vel_depth: bool = False) -> np.ndarray:
    """Sparse [H, W] float64 depth image of one scan (velodyne_points_helpers.py:55-96).

    Points behind the sensor are dropped, the rest projected, rounded to the pixel grid with the
    KITTI devkit's "-1" (Matlab indexing) and written in scan order, so that a later point
    overwrites an earlier one.  Then points are grouped by the reference's linear index
    `row * (W - 1) + col - 1` (NOT a bijection: it is the reference's `sub2ind`, kept as is);
    every group with more than one point stores the group's smallest depth at the pixel of the
    group's first point.  vel_depth: depth is the velodyne forward coordinate instead of the
    camera z."""
    H, W = int(im_shape[0]), int(im_shape[1])
    P = velodyne_to_image_projection(calib_dir, cam)
    scan = load_velodyne_scan(velo_file_name)
    scan = scan[scan[:, 0] >= 0, :]
    proj = (P @ scan.T).T                                   # float64 [N, 3]
    proj[:, :2] = proj[:, :2] / proj[:, 2][:, None]
    if vel_depth:
        proj[:, 2] = scan[:, 0]
    col = np.round(proj[:, 0]) - 1
    row = np.round(proj[:, 1]) - 1
    keep = (col >= 0) & (row >= 0) & (col < W) & (row < H)
    col, row, z = col[keep].astype(np.int64), row[keep].astype(np.int64), proj[keep, 2]

    depth = np.zeros((H, W))
    # scan order, last write wins (explicit: fancy assignment leaves the winner unspecified)
    flat = row * W + col
    last = np.full(H * W, -1, dtype=np.int64)
    np.maximum.at(last, flat, np.arange(flat.size))
    hit = last >= 0
    depth.reshape(-1)[hit] = z[last[hit]]

    if z.size:
        key = row * (W - 1) + col - 1                       # the reference's (aliasing) sub2ind
        order = np.argsort(key, kind="stable")              # groups keep scan order inside
        sk = key[order]
        starts = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
        counts = np.diff(np.r_[starts, sk.size])
        zmin = np.minimum.reduceat(z[order], starts)
        multi = counts > 1
        first = order[starts[multi]]                        # first point (scan order) of each group
        depth[row[first], col[first]] = zmin[multi]
    depth[depth < 0] = 0
    return depth


def velodyne_projection(calib_dir: str, cam: int = 2) -> Tuple[np.ndarray, np.ndarray]:
    """velodyne_to_image_projection in the two factors cuda_depth.project_points_batched takes: (M [3, 4] float32, the top
    rows of rectify @ rigid, velodyne -> rectified camera 0 frame; P [4, 4] float32 with [u' v' d' w'] = P [X Y Z 1]), both
    computed in float64 and rounded once.  With Pr = P_rect_0<cam>: rows 0 and 1 of P are Pr[0] - Pr[2] and Pr[1] - Pr[2],
    so that u'/w' and v'/w' are the projected column and row minus the devkit's 1; row 3 is Pr[2]; row 2 is
    [0, 0, 0, focal * baseline] of focal_length_and_baseline, a disparity over the projective depth."""
    cam2cam = read_calibration(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    velo2cam = read_calibration(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
    rigid = np.eye(4)
    rigid[:3, :3] = np.asarray(velo2cam["R"]).reshape(3, 3)
    rigid[:3, 3] = np.asarray(velo2cam["T"])
    rectify = np.eye(4)
    rectify[:3, :3] = np.asarray(cam2cam["R_rect_00"]).reshape(3, 3)
    pr = np.asarray(cam2cam["P_rect_0" + str(cam)], dtype=np.float64).reshape(3, 4)
    focal, baseline = focal_length_and_baseline(calib_dir)
    P = np.stack([pr[0] - pr[2], pr[1] - pr[2], np.array([0.0, 0.0, 0.0, focal * baseline]), pr[2]])
    return (rectify @ rigid)[:3].astype(np.float32), P.astype(np.float32)


def velodyne_disparity_map_device(calib_dir: str, velo_file_name: str, im_shape: Tuple[int, int], device, cam: int = 2):
    """The ground-truth disparity of one scan, [H, W] float64 on `device`, 0 where no return lands: what
    KittiSingleViewCamera derives from velodyne_depth_map(..., vel_depth=True), with the projection and the choice among
    the returns of a pixel on the GPU (cuda_depth.project_points_batched with velodyne_projection's matrices).  The scan is
    loaded and its returns behind the sensor (x < 0) dropped on the host, as the reference does; the value of a pixel is
    baseline * focal / x of the return that won it, in float64 and in the camera's own torch expression.

    It differs from the host path on purpose in two places.  Where several returns land on one pixel, the nearest by
    camera depth is kept; the host path keeps what the reference's aliasing `sub2ind` grouping produces (the last return
    in scan order, or the smallest depth of an aliased group written at the group's first pixel).  And the projection is
    float32: a return that projects exactly onto a half-pixel boundary may round to the other pixel.  On pixels hit by
    exactly one return away from such boundaries the two paths agree bit for bit.  (A return at or behind the camera's
    plane, which the host path would still project, is dropped.)"""
    import cuda_depth
    import torch
    H, W = int(im_shape[0]), int(im_shape[1])
    device = torch.device(device)
    M, P = velodyne_projection(calib_dir, cam)
    focal, baseline = focal_length_and_baseline(calib_dir)
    scan = load_velodyne_scan(velo_file_name)
    scan = scan[scan[:, 0] >= 0, :]
    count = scan.shape[0]
    if count == 0:
        return torch.zeros((H, W), dtype=torch.float64, device=device)
    points = torch.from_numpy(np.ascontiguousarray(scan[:, :3])).to(device)
    offsets = torch.tensor([0, count], dtype=torch.int32).to(device)
    _, index, _ = cuda_depth.project_points_batched(points, offsets, None, None, (H, W), P=P, world_to_camera=M[None],
                                                    invalid_disparity=0.0)
    index = index[0]
    forward = points[:, 0].to(torch.float64)[index.clamp(min=0).long()]
    disparity = baseline * focal / forward                              # x = 0 -> inf -> 0, as the host path
    zero = torch.zeros((), dtype=torch.float64, device=device)
    return torch.where((index >= 0) & ~torch.isinf(disparity), disparity, zero)


def reprojection_matrix(calib_dir: str, cams: Tuple[int, int] = (2, 3)) -> np.ndarray:
    """The float32 4x4 reprojection matrix Q (cuda_depth.reprojection_matrix) of a rectified camera pair from
    calib_cam_to_cam.txt: fx, fy, cx, cy of P_rect_0<left>, cx_right of P_rect_0<right>, and the baseline
    t_x / -f (right) - t_x / -f (left) in metres, so that the points are in the left rectified camera's frame."""
    cal = read_calibration(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    pl = np.asarray(cal[f"P_rect_0{cams[0]}"], dtype=np.float64).reshape(3, 4)
    pr = np.asarray(cal[f"P_rect_0{cams[1]}"], dtype=np.float64).reshape(3, 4)
    baseline = pr[0, 3] / -pr[0, 0] - pl[0, 3] / -pl[0, 0]
    import cuda_depth
    return cuda_depth.reprojection_matrix(float(pl[0, 0]), float(pl[0, 2]), float(pl[1, 2]), float(baseline),
                                          fy=float(pl[1, 1]), cx_right=float(pr[0, 2]))
