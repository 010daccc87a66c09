"""NumPy reference of smx_intensity_pyramid and smx_track_camera_pyramid (include/stereo_mi355x.h), written from the
header's text on top of tests/track_ref.py and tests/track_photo_ref.py: the reduce is one NumPy operation on float32
operands per float32 step with clamped indices; the geometric terms are track_ref.pixel_terms's as they are; the
photometric terms are track_photo_ref.photo_terms's with the level's coordinates, taps, gradient scaling and Huber's
weight; the tile sums, the trees, the solve and the update are theirs."""
from __future__ import annotations

import numpy as np

import track_photo_ref as tp
import track_ref as tr

f32 = np.float32
TERMS, SLOTS = tp.TERMS, tp.SLOTS


def level_dims(H, W, levels):
    dims = [(H, W)]
    for _ in range(levels - 1):
        dims.append(((dims[-1][0] + 1) // 2, (dims[-1][1] + 1) // 2))
    return dims


def _taps(m2, m1, c, p1, p2):
    return (((m2 + p2) + f32(4.0) * (m1 + p1)) + f32(6.0) * c) * f32(0.0625)


def reduce_ref(a):
    """One level from the one before it: a [..., H, W] float32 to [..., ceil(H / 2), ceil(W / 2)]."""
    a = np.asarray(a, f32)
    H, W = a.shape[-2:]
    with np.errstate(all="ignore"):
        x = 2 * np.arange((W + 1) // 2)
        col = [np.clip(x + k, 0, W - 1) for k in (-2, -1, 0, 1, 2)]
        h = _taps(*(a[..., :, c] for c in col))
        y = 2 * np.arange((H + 1) // 2)
        row = [np.clip(y + k, 0, H - 1) for k in (-2, -1, 0, 1, 2)]
        out = _taps(*(h[..., r, :] for r in row))
    assert out.dtype == np.float32
    return out


def intensity_pyramid_ref(planes, levels, mask_depth=None):
    """smx_intensity_pyramid: the list of `levels` float32 arrays [..., H_l, W_l] of planes [..., H, W]."""
    a = np.array(planes, f32)
    if mask_depth is not None:
        z = np.asarray(mask_depth, f32)
        with np.errstate(all="ignore"):
            a[~(np.isfinite(z) & (z > 0))] = np.nan
    out = [a]
    for _ in range(levels - 1):
        out.append(reduce_ref(out[-1]))
    return out


def flat(pyramid):
    """The pyramid as the entry's one buffer."""
    return np.concatenate([np.ascontiguousarray(p, f32).reshape(-1) for p in pyramid])


def default_levels(schedule, levels):
    """min(levels - 1, trailing zero bits of the stride) per pair."""
    return tuple(min(levels - 1, (int(s) & -int(s)).bit_length() - 1) for s, _ in schedule)


def photo_terms(points, T, model, stride, level, frame_level, weight, max_difference, huber_delta, inlier):
    """[SLOTS, Hs, Ws] float64, as track_photo_ref.photo_terms: the terms read from level `level`.  model["pyramid"]:
    the model view's levels [Hl, Wl]; frame_level: the frame pyramid's level [ceil(H / 2^level), ceil(W / 2^level)]."""
    assert stride % (1 << level) == 0
    X, Y, Z, w, _ = (a[::stride, ::stride] for a in points)
    H, W = points[0].shape
    F = np.asarray(frame_level, f32)[np.ix_(np.arange(0, H, stride) >> level, np.arange(0, W, stride) >> level)]
    T = np.asarray(T, f32)
    Mw, Pm = model["w2c"], model["Pm"]
    Imod = np.asarray(model["pyramid"][level], f32)
    Hl, Wl = Imod.shape
    lam, inv, delta = f32(weight), f32(1.0 / (1 << level)), f32(huber_delta)
    with np.errstate(all="ignore"):
        p = [((T[r, 0] * X + T[r, 1] * Y) + T[r, 2] * Z) + T[r, 3] for r in range(3)]
        c = [((Mw[r, 0] * p[0] + Mw[r, 1] * p[1]) + Mw[r, 2] * p[2]) + Mw[r, 3] for r in range(3)]
        u = {r: ((Pm[r, 0] * c[0] + Pm[r, 1] * c[1]) + Pm[r, 2] * c[2]) + Pm[r, 3] for r in (0, 1, 3)}
        x, y = u[0] / u[3], u[1] / u[3]
        xl, yl = x * inv, y * inv
        x0, y0 = np.floor(xl), np.floor(yl)
        m = inlier & (x0 >= 0) & (x0 <= f32(Wl - 2)) & (y0 >= 0) & (y0 <= f32(Hl - 2))
        ix = np.where(m, x0, 0).astype(np.int64)
        iy = np.where(m, y0, 0).astype(np.int64)
        if Wl < 2 or Hl < 2:
            m = np.zeros_like(m)
            ix1, iy1 = ix, iy
        else:
            ix1, iy1 = ix + 1, iy + 1
        taps = [(iy, ix), (iy, ix1), (iy1, ix), (iy1, ix1)]
        for t in taps:
            m &= np.isfinite(Imod[t])
        I00, I10, I01, I11 = (Imod[t] for t in taps)
        ax, ay = xl - x0, yl - y0
        bx, by = f32(1.0) - ax, f32(1.0) - ay
        Im = by * (bx * I00 + ax * I10) + ay * (bx * I01 + ax * I11)
        gx = (by * (I10 - I00) + ay * (I11 - I01)) * inv
        gy = (bx * (I01 - I00) + ax * (I11 - I10)) * inv
        e = F - Im
        m &= np.isfinite(e) & (np.abs(e) <= f32(max_difference))
        h = [(gx * (Pm[0, j] - x * Pm[3, j]) + gy * (Pm[1, j] - y * Pm[3, j])) / u[3] for j in range(3)]
        gw = [(Mw[0, i] * h[0] + Mw[1, i] * h[1]) + Mw[2, i] * h[2] for i in range(3)]
        a = [lam * (p[1] * gw[2] - p[2] * gw[1]), lam * (p[2] * gw[0] - p[0] * gw[2]), lam * (p[0] * gw[1] - p[1] * gw[0]),
             lam * gw[0], lam * gw[1], lam * gw[2]]
        b = lam * e
        for v in a + [b]:
            m &= np.isfinite(v)
        wh = np.where(np.abs(e) <= delta, f32(1.0), delta / np.abs(e)).astype(f32)
        wp = w * wh
        wa = [wp * a[i] for i in range(6)]
        planes = {k: wa[i] * a[j] for k, (i, j) in enumerate(tr.PAIRS)}
        planes.update({21 + i: wa[i] * b for i in range(6)})
        planes.update({31: (wp * e) * e, 32: wp, 33: np.ones_like(e)})
    out = np.zeros((SLOTS,) + X.shape, np.float64)
    for k, t in planes.items():
        assert t.dtype == np.float32, k
        out[k] = np.where(m, t.astype(np.float64), 0.0)
    return out


def pixel_terms(points, T, model, stride, max_distance, level, frame_level, weight, max_difference, huber_delta):
    """(G, P) as track_photo_ref.pixel_terms."""
    geo = tr.pixel_terms(points, T, model, stride, max_distance)
    G = np.zeros((SLOTS,) + geo.shape[1:], np.float64)
    G[:tr.TERMS + 1] = geo
    P = photo_terms(points, T, model, stride, level, frame_level, weight, max_difference, huber_delta, geo[29] == 1.0)
    return G, P


def track_pyramid_ref(disp, Q, pose_in, model, frame_pyramid, weight, *, schedule_levels=None, huber_delta=np.inf,
                      max_difference=tp.DEFAULT_MAX_DIFFERENCE, confidence=None, schedule=tr.DEFAULT_SCHEDULE,
                      max_distance=0.3, depth_range=(0.0, np.inf), min_confidence=0.0, invalid_disparity=-1.0,
                      min_inliers=100, min_pivot=1e-6, rot_eps=0.0, trans_eps=0.0, keep_tiles=False):
    """One triple, as track_photo_ref.track_photo_ref; model: model_view()'s dict with "pyramid" added, the list of the
    model view's levels (intensity_pyramid_ref with mask_depth = the model's depth); frame_pyramid: the frame's levels;
    schedule_levels: one level per pair (default default_levels for the pyramids' depth)."""
    if schedule_levels is None:
        schedule_levels = default_levels(schedule, len(frame_pyramid))
    assert len(schedule_levels) == len(schedule) and len(model["pyramid"]) == len(frame_pyramid)
    pts = tr.frame_points(disp, Q, confidence, min_confidence, depth_range, invalid_disparity)
    T0 = np.ascontiguousarray(np.asarray(pose_in, f32)[:3])
    T = T0.copy()
    info, pinfo = np.zeros(4, np.int32), np.zeros(2, np.int32)
    rms = prms = f32(np.nan)
    sums = np.zeros(TERMS, np.float64)
    done, tiles = False, None
    with np.errstate(all="ignore"):
        for (stride, iterations), level in zip(schedule, schedule_levels):
            for _ in range(iterations):
                if done:
                    break
                tiles = tp.tile_sums(*pixel_terms(pts, T, model, stride, max_distance, level, frame_pyramid[level], weight,
                                                  max_difference, huber_delta))
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
