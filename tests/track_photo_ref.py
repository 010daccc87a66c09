"""NumPy reference of smx_track_camera_photometric (include/stereo_mi355x.h), written from the header's text on top of
tests/track_ref.py: the geometric terms are track_ref.pixel_terms's as they are; the photometric terms of the geometric
inliers are one NumPy operation on float32 operands per float32 step; per tile column and row the geometric term is added
first and the photometric one second; the trees, the solve and the update are track_ref's."""
from __future__ import annotations

import numpy as np

import track_ref as tr

f32 = np.float32
TERMS = 33                                                           # the header's sums: 30 joint, then (w e) e, w, 1
SLOTS = 34                                                           # 0..29, 30 the accepted pixels, 31..33 the photometric sums
DEFAULT_MAX_DIFFERENCE = 30.0


def intensity_planes_ref(image, channels):
    """smx_intensity_planes: uint8 [n, channels, H, W] to float32 [n, H, W]."""
    a = np.asarray(image)
    assert a.dtype == np.uint8 and a.ndim == 4 and a.shape[1] == channels and channels in (1, 3)
    if channels == 1:
        return a[:, 0].astype(f32)
    v = 77 * a[:, 0].astype(np.int32) + 150 * a[:, 1].astype(np.int32) + 29 * a[:, 2].astype(np.int32)
    return v.astype(f32) * f32(0.00390625)


def photo_terms(points, T, model, stride, frame_intensity, weight, max_difference, inlier):
    """[SLOTS, Hs, Ws] float64: the photometric terms of every selected pixel (+0.0 where it has none), in the slots they
    are added to.  inlier: [Hs, Ws] bool, the geometric inliers."""
    X, Y, Z, w, _ = (a[::stride, ::stride] for a in points)
    F = np.asarray(frame_intensity, f32)[::stride, ::stride]
    T = np.asarray(T, f32)
    Mw, Pm = model["w2c"], model["Pm"]
    depth, Imod = model["depth"], np.asarray(model["intensity"], f32)
    Hm, Wm = depth.shape
    lam = f32(weight)
    with np.errstate(all="ignore"):
        p = [((T[r, 0] * X + T[r, 1] * Y) + T[r, 2] * Z) + T[r, 3] for r in range(3)]
        c = [((Mw[r, 0] * p[0] + Mw[r, 1] * p[1]) + Mw[r, 2] * p[2]) + Mw[r, 3] for r in range(3)]
        u = {r: ((Pm[r, 0] * c[0] + Pm[r, 1] * c[1]) + Pm[r, 2] * c[2]) + Pm[r, 3] for r in (0, 1, 3)}
        x, y = u[0] / u[3], u[1] / u[3]
        x0, y0 = np.floor(x), np.floor(y)
        m = inlier & (x0 >= 0) & (x0 <= f32(Wm - 2)) & (y0 >= 0) & (y0 <= f32(Hm - 2))
        ix = np.where(m, x0, 0).astype(np.int64)
        iy = np.where(m, y0, 0).astype(np.int64)
        if Wm < 2 or Hm < 2:
            m = np.zeros_like(m)
            ix1, iy1 = ix, iy
        else:
            ix1, iy1 = ix + 1, iy + 1
        taps = [(iy, ix), (iy, ix1), (iy1, ix), (iy1, ix1)]
        for t in taps:
            z = depth[t]
            m &= np.isfinite(z) & (z > 0) & np.isfinite(Imod[t])
        I00, I10, I01, I11 = (Imod[t] for t in taps)
        ax, ay = x - x0, y - y0
        bx, by = f32(1.0) - ax, f32(1.0) - ay
        Im = by * (bx * I00 + ax * I10) + ay * (bx * I01 + ax * I11)
        gx = by * (I10 - I00) + ay * (I11 - I01)
        gy = bx * (I01 - I00) + ax * (I11 - I10)
        e = F - Im
        m &= np.isfinite(e) & (np.abs(e) <= f32(max_difference))
        h = [(gx * (Pm[0, j] - x * Pm[3, j]) + gy * (Pm[1, j] - y * Pm[3, j])) / u[3] for j in range(3)]
        gw = [(Mw[0, i] * h[0] + Mw[1, i] * h[1]) + Mw[2, i] * h[2] for i in range(3)]
        a = [lam * (p[1] * gw[2] - p[2] * gw[1]), lam * (p[2] * gw[0] - p[0] * gw[2]), lam * (p[0] * gw[1] - p[1] * gw[0]),
             lam * gw[0], lam * gw[1], lam * gw[2]]
        b = lam * e
        for v in a + [b]:
            m &= np.isfinite(v)
        wa = [w * a[i] for i in range(6)]
        planes = {k: wa[i] * a[j] for k, (i, j) in enumerate(tr.PAIRS)}
        planes.update({21 + i: wa[i] * b for i in range(6)})
        planes.update({31: (w * e) * e, 32: w, 33: np.ones_like(e)})
    out = np.zeros((SLOTS,) + X.shape, np.float64)
    for k, t in planes.items():
        assert t.dtype == np.float32, k
        out[k] = np.where(m, t.astype(np.float64), 0.0)
    return out


def pixel_terms(points, T, model, stride, max_distance, frame_intensity, weight, max_difference):
    """(G, P), each [SLOTS, Hs, Ws] float64: the geometric terms in slots 0..30 (track_ref.pixel_terms) and the
    photometric ones."""
    geo = tr.pixel_terms(points, T, model, stride, max_distance)
    G = np.zeros((SLOTS,) + geo.shape[1:], np.float64)
    G[:tr.TERMS + 1] = geo
    P = photo_terms(points, T, model, stride, frame_intensity, weight, max_difference, geo[29] == 1.0)
    return G, P


def tile_sums(G, P):
    """[SLOTS, ty * tx] float64: the sum of every 64 x 4 tile; down a tile column, per row, the geometric term is added
    first and the photometric one second."""
    K, Hs, Ws = G.shape
    tx, ty = -(-Ws // tr.COLS), -(-Hs // tr.ROWS)
    col = np.zeros((K, ty, tx, tr.COLS), np.float64)
    pads = []
    for terms in (G, P):
        pad = np.zeros((K, ty * tr.ROWS, tx * tr.COLS), np.float64)
        pad[:, :Hs, :Ws] = terms
        pads.append(pad.reshape(K, ty, tr.ROWS, tx, tr.COLS))
    for r in range(tr.ROWS):
        col = (col + pads[0][:, :, r]) + pads[1][:, :, r]
    return tr._pairs_tree(col.reshape(K, ty * tx, tr.COLS))


def track_photo_ref(disp, Q, pose_in, model, frame_intensity, weight, *, max_difference=DEFAULT_MAX_DIFFERENCE,
                    confidence=None, schedule=tr.DEFAULT_SCHEDULE, max_distance=0.3, depth_range=(0.0, np.inf),
                    min_confidence=0.0, invalid_disparity=-1.0, min_inliers=100, min_pivot=1e-6, rot_eps=0.0,
                    trans_eps=0.0, keep_tiles=False):
    """One triple, as track_ref.track_ref; model: model_view()'s dict with "intensity" [Hm, Wm] added.  Returns a dict of
    pose, info, rms, sums [33] f64, pinfo [2] int32 (photometric inliers, geometric inliers without the term) and prms;
    with keep_tiles also tiles [SLOTS, ty * tx] f64, the tile sums of the last iteration that ran (None if none did)."""
    pts = tr.frame_points(disp, Q, confidence, min_confidence, depth_range, invalid_disparity)
    T0 = np.ascontiguousarray(np.asarray(pose_in, f32)[:3])
    T = T0.copy()
    info, pinfo = np.zeros(4, np.int32), np.zeros(2, np.int32)
    rms = prms = f32(np.nan)
    sums = np.zeros(TERMS, np.float64)
    done, tiles = False, None
    with np.errstate(all="ignore"):
        for stride, iterations in schedule:
            for _ in range(iterations):
                if done:
                    break
                tiles = tile_sums(*pixel_terms(pts, T, model, stride, max_distance, frame_intensity, weight, max_difference))
                S = tr._pairs_tree(tiles)
                sums = np.concatenate([S[:30], S[31:34]])
                info[1] += 1
                info[2], info[3] = int(S[29]), int(S[30])
                pinfo[0], pinfo[1] = int(S[33]), int(S[29]) - int(S[33])
                rms = np.sqrt(f32(S[27] / S[28]))
                prms = np.sqrt(f32(S[31] / S[32]))
                x = tr.solve(S, float(min_pivot)) if info[2] >= min_inliers else None
                if x is None:
                    info[0], T, done = 1, T0.copy(), True
                    break
                T, ww, tt = tr.update(T, x)
                done = bool(ww <= f32(rot_eps) * f32(rot_eps) and tt <= f32(trans_eps) * f32(trans_eps))
    out = {"pose": T, "info": info, "rms": f32(rms), "sums": sums, "pinfo": pinfo, "prms": f32(prms)}
    if keep_tiles:
        out["tiles"] = tiles
    return out
