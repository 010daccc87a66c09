"""Inputs shared by tests/test_project_cpu.py and tests/test_project_gpu.py: the round-trip maps, the collision-free KITTI
scan and the ground truth the device rule gives when the NumPy twin (tests/project_ref.py) drives it."""
from __future__ import annotations

import os

import numpy as np

import points3d_ref
import project_ref

KITTI_SHAPE = (375, 1242)

# (H, W, fx, cx, cy, baseline, doffs, (d_lo, d_hi)): a KITTI frame, a 1080p rig, an odd small map with Middlebury's doffs
ROUND_TRIPS = {
    "kitti": (375, 1242, 721.5, 609.6, 172.9, 0.537, 0.0, (4.0, 64.0)),
    "1080p": (1080, 1920, 1733.7, 960.0, 540.0, 0.12, 0.0, (75.0, 262.0)),
    "doffs": (33, 257, 400.0, 128.0, 16.0, 0.2, 3.5, (2.0, 40.0)),
}


def round_trip_case(name, cd, seed=0):
    """(Q, P, disp [1, H, W] with 10 % holes at -1)."""
    H, W, fx, cx, cy, B, doffs, (lo, hi) = ROUND_TRIPS[name]
    rng = np.random.default_rng(seed)
    disp = rng.uniform(lo, hi, (1, H, W)).astype(np.float32)
    disp[rng.random((1, H, W)) < 0.1] = np.float32(-1.0)
    Q = cd.reprojection_matrix(fx, cx, cy, B, cx_right=cx + doffs)
    return Q, cd.projection_matrix(Q), disp


IDENTITY = np.eye(4, dtype=np.float32)[None, :3, :]


def round_trip_twin(Q, P, disp):
    """The twin's round trip: (points, indices, disp_back, index_back, relative error of disp_back on the valid pixels)."""
    _, H, W = disp.shape
    points, _, indices, offsets, _ = points3d_ref.reproject_ref(disp, Q)
    back, index, _ = project_ref.project_ref(points, offsets, IDENTITY, P, (H, W))
    valid = disp[0] != np.float32(-1.0)
    err = float(np.max(np.abs(back[0][valid].astype(np.float64) - disp[0][valid]) / np.abs(disp[0][valid])))
    return points, indices, back[0], index[0], err


def collision_free_scan(calib_dir, count=40000, seed=5):
    """A random scan [N, 4] float32 (x 3..60, y -25..25, z -2.5..1.5) reduced to the returns whose float64 projection is
    more than 1e-3 px from a rounding boundary and, of those that land in the image, to the ones whose pixel and whose
    reference `sub2ind` key are both unique: on it the host path has nothing to choose between."""
    from helpers.kitti_calibration import velodyne_to_image_projection
    H, W = KITTI_SHAPE
    rng = np.random.default_rng(seed)
    scan = np.stack([rng.uniform(3, 60, count), rng.uniform(-25, 25, count), rng.uniform(-2.5, 1.5, count),
                     np.ones(count)], 1).astype(np.float32)
    proj = (velodyne_to_image_projection(calib_dir) @ scan.astype(np.float64).T).T
    u, v = proj[:, 0] / proj[:, 2], proj[:, 1] / proj[:, 2]
    away = (np.abs(u - np.floor(u) - 0.5) > 1e-3) & (np.abs(v - np.floor(v) - 0.5) > 1e-3)
    scan, u, v = scan[away], u[away], v[away]
    col, row = (np.round(u) - 1).astype(np.int64), (np.round(v) - 1).astype(np.int64)
    inside = (col >= 0) & (row >= 0) & (col < W) & (row < H)
    keep = np.ones(len(scan), dtype=bool)
    for key in (row * W + col, row * (W - 1) + col - 1):
        _, inverse, counts = np.unique(key[inside], return_inverse=True, return_counts=True)
        keep[np.flatnonzero(inside)[counts[inverse] > 1]] = False
    return scan[keep]


def write_scan(path, scan):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    scan.astype(np.float32).tofile(path)


def host_ground_truth(calib_dir, velo_file):
    """What KittiSingleViewCamera yields before padding: baseline * focal / depth, 0 where there is no return."""
    from helpers.kitti_calibration import focal_length_and_baseline, velodyne_depth_map
    focal, baseline = focal_length_and_baseline(calib_dir)
    import torch
    depth = torch.from_numpy(velodyne_depth_map(calib_dir, velo_file, KITTI_SHAPE, vel_depth=True))
    disparity = baseline * focal / depth            # the camera's expression, which torch evaluates as reciprocal * scalar
    disparity[torch.isinf(disparity)] = 0
    return disparity.numpy()


def twin_ground_truth(calib_dir, velo_file):
    """helpers.kitti_calibration.velodyne_disparity_map_device with the twin in the device call's place."""
    from helpers.kitti_calibration import focal_length_and_baseline, load_velodyne_scan, velodyne_projection
    M, P = velodyne_projection(calib_dir)
    focal, baseline = focal_length_and_baseline(calib_dir)
    scan = load_velodyne_scan(velo_file)
    scan = scan[scan[:, 0] >= 0, :]
    _, index, _ = project_ref.project_one(scan[:, :3], M, P, KITTI_SHAPE, invalid_disparity=0.0)
    import torch
    forward = torch.from_numpy(scan[:, 0].astype(np.float64)[np.maximum(index, 0)])
    disparity = (baseline * focal / forward).numpy()                           # in torch, as the device path and the camera
    return np.where((index >= 0) & ~np.isinf(disparity), disparity, 0.0)


def tiny_clouds(seed, n, most, H, W, Q, margin=1.5):
    """A batch of n clouds of 0..most points each (points [total + 1, 3] float32 with one spare row, offsets [n + 1] int32,
    the index of a cloud that follows a run of empty ones): the first two and the last three clouds are empty, and so are
    40 in a row from n // 3 on, more than one thread's share of the offsets at any n; the cloud after them has `most`
    points.  The points land in or within `margin` pixels of an H x W view of Q from near the identity, at depths on a
    0.1 m grid so that equal depths meet."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, most + 1, n)
    after = n // 3 + 40
    counts[:2], counts[-3:], counts[n // 3:after], counts[after] = 0, 0, 0, most
    total = int(counts.sum())
    u = rng.uniform(-margin, W - 1 + margin, total)
    v = rng.uniform(-margin, H - 1 + margin, total)
    z = np.round(rng.uniform(0.4, 6.0, total), 1)
    z[rng.random(total) < 0.03] *= -1
    fx, fy, cx, cy = float(Q[2, 3]), float(Q[2, 3] / Q[1, 1]), -float(Q[0, 3]), -float(Q[1, 3] / Q[1, 1])
    pts = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1).astype(np.float32)
    pts = np.concatenate([pts, np.zeros((1, 3), np.float32)])
    return pts, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), after


def near_identity_views(seed, n):
    """n world-to-camera matrices [n, 3, 4] float32: the identity moved by a few centimetres."""
    rng = np.random.default_rng(seed)
    w2c = np.tile(np.eye(4, dtype=np.float32)[:3], (n, 1, 1))
    w2c[:, :, 3] = rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32)
    return w2c


def unruly_offsets(off, cap):
    """The offsets of a batch with entries that the device has to clamp (points3d_ref.clamp_offsets), for a batch whose
    n + 1 offsets give a thread of the clamping workgroup `per` = 3 entries (513 <= n + 1 <= 768): negative entries, a
    large entry at the middle, the end and the start of a thread's share, each of which raises every later entry up to
    where the true offsets pass it, and an entry above the capacity near the end."""
    n1 = len(off)
    per = (n1 + 255) // 256
    assert per == 3 and n1 > 660, n1
    raw = np.array(off, dtype=np.int64)
    raw[0], raw[10], raw[31] = -3, -5, -2 ** 31
    raw[50 * per + 1] = off[50 * per + 61]               # thread 50's middle entry: clouds up to 60 further on are emptied
    raw[110 * per + 2] = off[110 * per + 80]             # the last entry of thread 110's share
    raw[170 * per] = off[170 * per + 47]                 # the first entry of thread 170's
    raw[650] = cap + 7                                   # everything from here on is clamped to the capacity
    raw[655] = 2 ** 31 - 1
    return raw.astype(np.int32)
