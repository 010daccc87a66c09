"""NumPy reference of smx_reproject_points and smx_voxel_downsample (include/stereo_mi355x.h), in the header's float32
operation order: every arithmetic step below is one float32 NumPy operation on float32 operands (NumPy neither fuses
nor reorders them), so the GPU must match it bit for bit."""
from __future__ import annotations

import numpy as np

VOX_LIMIT = np.float32(2 ** 20)
CHUNK = 64


def colour_u8(v: np.ndarray) -> np.ndarray:
    """f32 -> u8: clamp(floorf(v + 0.5f), 0, 255), NaN -> 0."""
    if v.dtype == np.uint8:
        return v
    r = np.floor(v.astype(np.float32) + np.float32(0.5))
    return np.fmin(np.fmax(r, np.float32(0)), np.float32(255)).astype(np.uint8)


def reproject_ref(disp, Q, image=None, confidence=None, min_confidence=0.0, depth_range=(0.0, np.inf),
                  invalid_disparity=-1.0):
    """disp [n, H, W] f32; image None, [n, H, W] / [n, 1, H, W] (gray) or [n, 3, H, W], u8 or f32; confidence [n, H, W] or
    None.  Returns (points [N, 3] f32, colors [N, 3] u8 or None, indices [N] int32, offsets [n + 1], xyz_map)."""
    disp = np.asarray(disp, dtype=np.float32)
    n, H, W = disp.shape
    q = np.asarray(Q, dtype=np.float32).reshape(4, 4)
    v, u = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    d = disp
    with np.errstate(all="ignore"):
        rows = [((q[r, 0] * u + q[r, 1] * v) + q[r, 2] * d) + q[r, 3] for r in range(4)]
        xw, yw, zw, ww = rows
        X, Y, Z = xw / ww, yw / ww, zw / ww
        ok = np.isfinite(d) & (d != np.float32(invalid_disparity)) & (ww > 0)
        ok &= np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
        ok &= (Z >= np.float32(depth_range[0])) & (Z <= np.float32(depth_range[1]))
        if confidence is not None:
            ok &= np.asarray(confidence, dtype=np.float32) >= np.float32(min_confidence)
    xyz = np.stack([X, Y, Z], axis=-1).astype(np.float32)
    xyz_map = np.where(ok[..., None], xyz, np.float32(np.nan)).astype(np.float32)
    points = xyz[ok]
    counts = ok.reshape(n, -1).sum(axis=1)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pix = np.broadcast_to(np.arange(H * W, dtype=np.int32).reshape(H, W), (n, H, W))
    indices = pix[ok].astype(np.int32)
    colors = None
    if image is not None:
        img = np.asarray(image)
        if img.ndim == 3:
            img = img[:, None]
        c = colour_u8(img)                                            # [n, C, H, W]
        if c.shape[1] == 1:
            c = np.repeat(c, 3, axis=1)
        colors = np.moveaxis(c, 1, -1)[ok]
    return points, colors, indices, offsets, xyz_map


def _voxel_index(pts: np.ndarray, voxel_size: float):
    with np.errstate(all="ignore"):
        f = np.floor(pts / np.float32(voxel_size))
    ok = np.all((f >= -VOX_LIMIT) & (f < VOX_LIMIT), axis=1)
    idx = np.zeros(f.shape, dtype=np.int64)
    idx[ok] = f[ok].astype(np.int64)
    return idx, ok


def two_level_sum(P: np.ndarray, starts: np.ndarray, cnt: np.ndarray) -> np.ndarray:
    """Per segment [starts[v], starts[v] + cnt[v]) of P [M, 3] f32: sequential sums within chunks of 64 (from the first
    point), then sequential over the chunk sums.  Vectorised across segments; loops over the position only."""
    V = starts.size
    if V == 0:
        return np.zeros((0, 3), dtype=np.float32)
    nch = (cnt + CHUNK - 1) // CHUNK
    first = np.concatenate([[0], np.cumsum(nch)[:-1]])
    seg = np.repeat(np.arange(V), nch)
    k = np.arange(nch.sum()) - first[seg]
    c_start = starts[seg] + CHUNK * k
    c_len = np.minimum(CHUNK, cnt[seg] - CHUNK * k)
    cs = P[c_start].astype(np.float32).copy()
    for j in range(1, CHUNK):
        m = c_len > j
        if not m.any():
            break
        cs[m] = cs[m] + P[c_start[m] + j]
    S = cs[first].copy()
    for kk in range(1, int(nch.max())):
        m = nch > kk
        S[m] = S[m] + cs[first[m] + kk]
    return S


def clamp_offsets(offsets, capacity):
    """The caller's offsets as smx_voxel_downsample reads them: "clamped to a non-decreasing sequence in [0, capacity]",
    each entry raised to the one before it (the first to 0), then lowered to the capacity."""
    out, prev = [], 0
    for o in offsets:
        prev = min(max(int(o), prev), int(capacity))
        out.append(prev)
    return np.asarray(out, dtype=np.int64)


def voxel_ref(points, colors, offsets, voxel_size, min_points=1):
    """points [cap, 3] f32, colors [cap, 3] u8 or None, offsets [n + 1].  Returns (points [V, 3] f32, colors [V, 3] u8 or
    None, counts [V] int32, offsets [n + 1] int64, dropped [n] int64)."""
    points = np.asarray(points, dtype=np.float32)
    offsets = [int(o) for o in offsets]
    n = len(offsets) - 1
    outs_p, outs_c, outs_n, dropped, out_off = [], [], [], [], [0]
    for m in range(n):
        P = points[offsets[m]:offsets[m + 1]]
        Cc = None if colors is None else np.asarray(colors)[offsets[m]:offsets[m + 1]]
        idx, ok = _voxel_index(P, voxel_size)
        drop = int((~ok).sum())
        sel = np.flatnonzero(ok)
        order = sel[np.lexsort((idx[sel, 2], idx[sel, 1], idx[sel, 0]))]      # stable: pixel order within a voxel
        keys = idx[order]
        if order.size:
            head = np.r_[True, np.any(keys[1:] != keys[:-1], axis=1)]
            starts = np.flatnonzero(head)
            cnt = np.diff(np.r_[starts, order.size])
        else:
            starts = cnt = np.zeros(0, dtype=np.int64)
        keep = cnt >= min_points
        drop += int(cnt[~keep].sum())
        if Cc is not None:                                        # integer sums over every voxel, then the kept ones
            Cs = Cc[order].astype(np.int64)
            sums = (np.stack([np.add.reduceat(Cs[:, ch], starts) for ch in range(3)], axis=1) if starts.size
                    else np.zeros((0, 3), np.int64))[keep]
        starts, cnt = starts[keep], cnt[keep]
        Ps = P[order]
        S = two_level_sum(Ps, starts, cnt)
        outs_p.append((S / cnt.astype(np.float32)[:, None]).astype(np.float32))
        if Cc is not None:
            outs_c.append(((sums + (cnt // 2)[:, None]) // cnt[:, None]).astype(np.uint8))
        outs_n.append(cnt.astype(np.int32))
        dropped.append(drop)
        out_off.append(out_off[-1] + int(cnt.size))
    cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dt)  # noqa: E731
    return (cat(outs_p, (0, 3), np.float32), None if colors is None else cat(outs_c, (0, 3), np.uint8),
            cat(outs_n, (0,), np.int32), np.asarray(out_off, dtype=np.int64), np.asarray(dropped, dtype=np.int64))
