"""NumPy reference of smx_project_points (include/stereo_mi355x.h), in the header's float32 operation order: every
arithmetic step below is one float32 NumPy operation on float32 operands (NumPy neither fuses nor reorders them), and the
depth test is np.minimum.at on the 64-bit keys (bits(c_2) << 32) | j, so the GPU must match it bit for bit."""
from __future__ import annotations

import numpy as np

from points3d_ref import clamp_offsets

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def project_candidates(pts, M, P, shape, radius=0, depth_range=(0.0, np.inf), invalid_disparity=-1.0):
    """The points of one cloud [N, 3] that become candidates: (j [K] int64, fu [K] int64, fv [K] int64, c_2 [K] f32,
    d [K] f32), in input order.  M: [3, 4], P: [4, 4]."""
    H, W = shape
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    M = np.asarray(M, dtype=np.float32).reshape(3, 4)
    P = np.asarray(P, dtype=np.float32).reshape(4, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    R = np.float32(radius)
    with np.errstate(all="ignore"):
        c = [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)]
        ok = np.isfinite(c[2]) & (c[2] > 0) & (c[2] >= np.float32(depth_range[0])) & (c[2] <= np.float32(depth_range[1]))
        p = [((P[r, 0] * c[0] + P[r, 1] * c[1]) + P[r, 2] * c[2]) + P[r, 3] for r in range(4)]
        ok &= p[3] > 0
        fu = np.floor(p[0] / p[3] + np.float32(0.5))
        fv = np.floor(p[1] / p[3] + np.float32(0.5))
        ok &= (fu >= -R) & (fu <= np.float32(W - 1) + R) & (fv >= -R) & (fv <= np.float32(H - 1) + R)   # NaN fails
        d = p[2] / p[3]
        ok &= np.isfinite(d) & (d != np.float32(invalid_disparity))
    j = np.flatnonzero(ok)
    return j, fu[j].astype(np.int64), fv[j].astype(np.int64), c[2][j].astype(np.float32), d[j].astype(np.float32)


def project_one(pts, M, P, shape, radius=0, depth_range=(0.0, np.inf), invalid_disparity=-1.0):
    """One cloud into one view: (disp [H, W] f32, index [H, W] int32, depth [H, W] f32)."""
    H, W = shape
    j, fu, fv, c2, d = project_candidates(pts, M, P, shape, radius, depth_range, invalid_disparity)
    keys = np.full(H * W, EMPTY, dtype=np.uint64)
    key = (c2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            u, v = fu + dx, fv + dy
            inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
            np.minimum.at(keys, (v * W + u)[inside], key[inside])
    hit = keys != EMPTY
    win = (keys[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    disp = np.full(H * W, np.float32(invalid_disparity), dtype=np.float32)
    index = np.full(H * W, -1, dtype=np.int32)
    depth = np.full(H * W, np.nan, dtype=np.float32)
    d_all = np.zeros(max(len(np.asarray(pts).reshape(-1, 3)), 1), dtype=np.float32)
    d_all[j] = d
    disp[hit] = d_all[win]
    index[hit] = win.astype(np.int32)
    depth[hit] = (keys[hit] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return disp.reshape(H, W), index.reshape(H, W), depth.reshape(H, W)


def project_ref(points, offsets, world_to_camera, P, shape, radius=0, depth_range=(0.0, np.inf), invalid_disparity=-1.0):
    """points [cap, 3] f32, offsets [n + 1] (used clamped, as the device does), world_to_camera [n, 3, 4].  Returns
    (disp, index, depth), each [n, H, W]."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    off = clamp_offsets(offsets, points.shape[0])
    w2c = np.asarray(world_to_camera, dtype=np.float32).reshape(-1, 3, 4)
    outs = [project_one(points[off[f]:off[f + 1]], w2c[f], P, shape, radius, depth_range, invalid_disparity)
            for f in range(len(off) - 1)]
    return tuple(np.stack([o[k] for o in outs]) for k in range(3))


def project_loop(pts, M, P, shape, radius=0, depth_range=(0.0, np.inf), invalid_disparity=-1.0):
    """project_one as a plain double loop over points and footprint pixels, with an explicit (c_2, j) comparison instead
    of keys: what the twin is checked against.  For a few hundred points."""
    H, W = shape
    f32 = np.float32
    pts = np.asarray(pts, dtype=f32).reshape(-1, 3)
    M = np.asarray(M, dtype=f32).reshape(3, 4)
    P = np.asarray(P, dtype=f32).reshape(4, 4)
    R = f32(radius)
    disp = np.full((H, W), f32(invalid_disparity), dtype=f32)
    index = np.full((H, W), -1, dtype=np.int32)
    depth = np.full((H, W), np.nan, dtype=f32)
    with np.errstate(all="ignore"):
        for j, (x, y, z) in enumerate(pts):
            c = [f32(f32(f32(f32(M[r, 0] * x) + f32(M[r, 1] * y)) + f32(M[r, 2] * z)) + M[r, 3]) for r in range(3)]
            if not (np.isfinite(c[2]) and c[2] > 0 and f32(depth_range[0]) <= c[2] <= f32(depth_range[1])):
                continue
            p = [f32(f32(f32(f32(P[r, 0] * c[0]) + f32(P[r, 1] * c[1])) + f32(P[r, 2] * c[2])) + P[r, 3]) for r in range(4)]
            if not p[3] > 0:
                continue
            fu = np.floor(f32(f32(p[0] / p[3]) + f32(0.5)))
            fv = np.floor(f32(f32(p[1] / p[3]) + f32(0.5)))
            if not (-R <= fu <= f32(W - 1) + R and -R <= fv <= f32(H - 1) + R):
                continue
            d = f32(p[2] / p[3])
            if not (np.isfinite(d) and d != f32(invalid_disparity)):
                continue
            for v in range(int(fv) - radius, int(fv) + radius + 1):
                for u in range(int(fu) - radius, int(fu) + radius + 1):
                    if 0 <= u < W and 0 <= v < H:
                        if index[v, u] < 0 or c[2] < depth[v, u]:          # a later j wins only when strictly nearer
                            disp[v, u], index[v, u], depth[v, u] = d, j, c[2]
    return disp, index, depth
