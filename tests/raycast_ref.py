"""NumPy reference of smx_tsdf_raycast (include/stereo_mi355x.h), in the header's float32 operation order: every
arithmetic step is one float32 NumPy operation on float32 operands, vectorised over the rays of a view, looping over the
samples m = 0 .. M-1.  It is the dense rule: every sample of every ray that has not ended is evaluated, nothing is
skipped."""
from __future__ import annotations

import numpy as np

f32 = np.float32


def sample_count(z_min, z_max, step) -> int:
    """M = (int)floorf((z_max - z_min)/step) + 1 in float32."""
    return int(np.floor((f32(z_max) - f32(z_min)) / f32(step))) + 1


def _cell(p, origin, s, dims):
    """(g, f, in_bounds) of the points p = [px, py, pz]."""
    g = [(p[a] - origin[a]) / s - f32(0.5) for a in range(3)]
    f = [np.floor(x) for x in g]
    inb = np.ones(g[0].shape, bool)
    for a in range(3):
        inb &= (f[a] >= 0) & (f[a] <= f32(dims[a] - 2))                # NaN fails
    return g, f, inb


def _lerp(a, b, t):
    return a + (b - a) * t


def _corners(vol, f, idx, dims):
    """The eight corner values [8, len(idx)] (cx fastest) of the cells f at the rays idx, from the flat volume."""
    nx, ny, _ = dims
    i0 = [f[a][idx].astype(np.int64) for a in range(3)]
    base = (i0[2] * ny + i0[1]) * nx + i0[0]
    return np.stack([vol[base + cx + cy * nx + cz * nx * ny] for cz in (0, 1) for cy in (0, 1) for cx in (0, 1)])


def _trilinear(c, g, f, idx):
    tx, ty, tz = (g[a][idx] - f[a][idx] for a in range(3))
    c00, c10 = _lerp(c[0], c[1], tx), _lerp(c[2], c[3], tx)
    c01, c11 = _lerp(c[4], c[5], tx), _lerp(c[6], c[7], tx)
    return _lerp(_lerp(c00, c10, ty), _lerp(c01, c11, ty), tz)


def _view(state, dims, o, s, q, M, H, W, min_weight, step, z_min, n_samples, invalid):
    nx, ny, nz = dims
    T = state["tsdf"].reshape(-1)
    Wt = state["weight"].reshape(-1)
    v, u = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    xp = (q[0, 0] * u + q[0, 1] * v) + q[0, 3]
    yp = (q[1, 0] * u + q[1, 1] * v) + q[1, 3]
    zp = (q[2, 0] * u + q[2, 1] * v) + q[2, 3]
    has_ray = zp > 0
    rx, ry = xp / zp, yp / zp
    dw = [(M[r, 0] * rx + M[r, 1] * ry) + M[r, 2] for r in range(3)]
    e = [M[r, 3] for r in range(3)]
    N = u.size
    done = ~has_ray
    hit = np.zeros(N, bool)
    lam_hit = np.zeros(N, f32)
    pv = np.zeros(N, bool)
    pT = np.zeros(N, f32)
    for m in range(n_samples):
        if done.all():
            break
        lam = z_min + f32(m) * step
        p = [e[a] + dw[a] * lam for a in range(3)]
        g, f, inb = _cell(p, o, s, dims)
        idx = np.flatnonzero(inb & ~done)
        ok = (_corners(Wt, f, idx, dims) >= min_weight).all(axis=0)
        val = _trilinear(_corners(T, f, idx, dims), g, f, idx)
        valid = np.zeros(N, bool)
        valid[idx] = ok
        Tm = np.zeros(N, f32)
        Tm[idx] = val
        ends = valid & (Tm < 0) & ~done
        h = ends & pv & (pT >= 0) & (pT < 1)
        lam_prev = z_min + f32(m - 1) * step
        lh = lam_prev + step * (pT / (pT - Tm))
        lam_hit[h] = lh[h]
        hit |= h
        done |= ends
        upd = ~done
        pv[upd] = valid[upd]
        pT[upd] = Tm[upd]
    out = {"disparity": np.where(hit, (zp / lam_hit - q[3, 3]) / q[3, 2], invalid).astype(f32).reshape(H, W),
           "depth": np.where(hit, lam_hit, f32(np.nan)).astype(f32).reshape(H, W)}
    # the hit point, its normal, colour and weight
    hi = np.flatnonzero(hit)
    ps = [(e[a] + dw[a] * lam_hit)[hi] for a in range(3)]
    d, ok = [], np.ones(hi.size, bool)
    for a in range(3):
        side = []
        for sign in (1, -1):
            pp = list(ps)
            pp[a] = ps[a] + s if sign > 0 else ps[a] - s
            g, f, inb = _cell(pp, o, s, dims)
            ok &= inb
            idx = np.flatnonzero(inb)
            t = np.zeros(hi.size, f32)
            t[idx] = _trilinear(_corners(T, f, idx, dims), g, f, idx)
            side.append(t)
        d.append(side[0] - side[1])
    ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    ok &= ln != 0
    nrm = np.zeros((3, N), f32)
    for a in range(3):
        nrm[a, hi] = np.where(ok, d[a] / ln, f32(0))
    out["normals"] = nrm.reshape(3, H, W)
    g, _, _ = _cell(ps, o, s, dims)
    iv = [np.fmin(np.fmax(np.floor(g[a] + f32(0.5)), f32(0)), f32(dims[a] - 1)).astype(np.int64) for a in range(3)]
    vox = (iv[2] * ny + iv[1]) * nx + iv[0]
    wgt = np.zeros(N, f32)
    wgt[hi] = Wt[vox]
    out["weight"] = wgt.reshape(H, W)
    out["colors"] = None
    if state["color"] is not None:
        col = np.zeros((3, N), np.uint8)
        col[:, hi] = state["color"].reshape(-1, 4)[vox, :3].T
        out["colors"] = col.reshape(3, H, W)
    return out


def raycast_ref(state, dims, origin, voxel_size, Q, camera_to_world, shape, *, min_weight=1.0, step=None,
                depth_range=(0.0, 10.0), invalid_disparity=-1.0):
    """The five outputs of smx_tsdf_raycast for poses camera_to_world [n, 3 or 4, 4] (taken as float32, not inverted):
    a dict of disparity, depth, weight [n, H, W] f32, normals [n, 3, H, W] f32 and colors [n, 3, H, W] u8 (None without
    a colour volume).  state: tsdf_ref.empty_state's dict; step defaults to voxel_size."""
    H, W = shape
    q = np.asarray(Q, f32).reshape(4, 4)
    poses = np.asarray(camera_to_world, f32)
    if poses.ndim == 2:
        poses = poses[None]
    s = f32(voxel_size)
    step = s if step is None else f32(step)
    o = [f32(v) for v in origin]
    z_min, z_max = f32(depth_range[0]), f32(depth_range[1])
    n_samples = sample_count(z_min, z_max, step)
    views = []
    with np.errstate(all="ignore"):
        for M in poses:
            views.append(_view(state, dims, o, s, q, M[:3, :], H, W, f32(min_weight), step, z_min, n_samples,
                               f32(invalid_disparity)))
    return {k: None if views[0][k] is None else np.stack([v[k] for v in views]) for k in views[0]}


def view_pose(camera_to_world) -> np.ndarray:
    """[n, 3, 4] float32: the top rows of camera-to-world poses, rounded once from float64 (as TSDFVolume.render does)."""
    m = np.asarray(camera_to_world, np.float64)
    if m.ndim == 2:
        m = m[None]
    return np.ascontiguousarray(m[:, :3, :].astype(np.float32))
