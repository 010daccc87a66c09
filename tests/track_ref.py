"""NumPy reference of smx_track_camera (include/stereo_mi355x.h), written from the header's text: every float32 step is
one NumPy operation on float32 operands, vectorised over the selected pixels of an iteration; the thirty sums are float64
additions in the header's order (tile columns top to bottom, the 64 columns and then the tiles by adjacent-pairs trees);
the solve runs in Python floats (IEEE float64, no fused multiply-add) and the pose update in np.float32 scalars."""
from __future__ import annotations

import math

import numpy as np

f32 = np.float32
COLS, ROWS = 64, 4                                                   # a tile of the selected grid
DEFAULT_SCHEDULE = ((4, 4), (2, 5), (1, 10))
TERMS = 30
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]              # the order of the 21 terms (w a_i) a_j


def frame_points(disp, Q, confidence=None, min_confidence=0.0, depth_range=(0.0, np.inf), invalid_disparity=-1.0):
    """(X, Y, Z, w, accepted), each [H, W]: the camera points of smx_reproject_points under smx_tsdf_integrate's pixel
    acceptance rule (with X and Y finite as well)."""
    d = np.asarray(disp, f32)
    H, W = d.shape
    q = np.asarray(Q, f32).reshape(4, 4)
    v, u = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    with np.errstate(all="ignore"):
        r = [((q[k, 0] * u + q[k, 1] * v) + q[k, 2] * d) + q[k, 3] for k in range(4)]
        X, Y, Z = r[0] / r[3], r[1] / r[3], r[2] / r[3]
        ok = np.isfinite(d) & (d != f32(invalid_disparity)) & (r[3] > 0) & np.isfinite(Z)
        ok &= (Z >= f32(depth_range[0])) & (Z <= f32(depth_range[1]))
        w = np.ones_like(d)
        if confidence is not None:
            c = np.asarray(confidence, f32)
            ok &= (c >= f32(min_confidence)) & (c > 0)
            w = c.copy()
        ok &= np.isfinite(X) & np.isfinite(Y)
    return X, Y, Z, w, ok


def model_view(depth, normals, Qm, camera_to_world):
    """The model side of one triple: depth [Hm, Wm], normals [3, Hm, Wm], Qm, and the pose [4, 4] / [3, 4] (float64 or
    float32) rounded and inverted the way the Python layer does."""
    m = np.asarray(camera_to_world, np.float64)
    if m.shape[0] == 3:
        m = np.vstack([m, [0.0, 0.0, 0.0, 1.0]])
    return {"depth": np.asarray(depth, f32), "normals": np.asarray(normals, f32), "Qm": np.asarray(Qm, f32).reshape(4, 4),
            "Pm": np.linalg.inv(np.asarray(Qm, np.float64).reshape(4, 4)).astype(f32),
            "c2w": np.ascontiguousarray(m[:3].astype(f32)),
            "w2c": np.ascontiguousarray(np.linalg.inv(m)[:3].astype(f32))}


def pixel_terms(points, T, model, stride, max_distance):
    """[31, Hs, Ws] float64: the thirty terms of every selected pixel of an iteration of stride `stride` at the pose
    T [3, 4] float32 (+0.0 where the pixel is skipped), and, as a 31st plane, 1 where the pixel is accepted."""
    X, Y, Z, w, ok = (a[::stride, ::stride] for a in points)
    T = np.asarray(T, f32)
    Mw, Mc, Pm, Qm = model["w2c"], model["c2w"], model["Pm"], model["Qm"]
    depth, normals = model["depth"], model["normals"]
    Hm, Wm = depth.shape
    with np.errstate(all="ignore"):
        p = [((T[r, 0] * X + T[r, 1] * Y) + T[r, 2] * Z) + T[r, 3] for r in range(3)]
        c = [((Mw[r, 0] * p[0] + Mw[r, 1] * p[1]) + Mw[r, 2] * p[2]) + Mw[r, 3] for r in range(3)]
        pp = {r: ((Pm[r, 0] * c[0] + Pm[r, 1] * c[1]) + Pm[r, 2] * c[2]) + Pm[r, 3] for r in (0, 1, 3)}
        fu = np.floor(pp[0] / pp[3] + f32(0.5))
        fv = np.floor(pp[1] / pp[3] + f32(0.5))
        m = ok & (c[2] > 0) & (pp[3] > 0) & (fu >= 0) & (fu <= f32(Wm - 1)) & (fv >= 0) & (fv <= f32(Hm - 1))
        iu = np.where(m, fu, 0).astype(np.int64)
        iv = np.where(m, fv, 0).astype(np.int64)
        lam = depth[iv, iu]
        m &= np.isfinite(lam) & (lam > 0)
        n = [normals[a][iv, iu] for a in range(3)]
        m &= ~((n[0] == 0) & (n[1] == 0) & (n[2] == 0))
        xp = (Qm[0, 0] * fu + Qm[0, 1] * fv) + Qm[0, 3]
        yp = (Qm[1, 0] * fu + Qm[1, 1] * fv) + Qm[1, 3]
        zp = (Qm[2, 0] * fu + Qm[2, 1] * fv) + Qm[2, 3]
        rx, ry = xp / zp, yp / zp
        q = [Mc[r, 3] + ((Mc[r, 0] * rx + Mc[r, 1] * ry) + Mc[r, 2]) * lam for r in range(3)]
        dl = [q[r] - p[r] for r in range(3)]
        dist2 = (dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]
        m &= dist2 <= f32(max_distance) * f32(max_distance)
        b = (n[0] * dl[0] + n[1] * dl[1]) + n[2] * dl[2]
        a = [p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]]
        wa = [w * a[i] for i in range(6)]
        planes = [wa[i] * a[j] for i, j in PAIRS] + [wa[i] * b for i in range(6)] + [(w * b) * b, w, np.ones_like(w)]
    for k, t in enumerate(planes):
        assert t.dtype == np.float32, k
    out = np.zeros((TERMS + 1,) + X.shape, np.float64)
    for k, t in enumerate(planes):
        out[k] = np.where(m, t.astype(np.float64), 0.0)
    out[TERMS] = ok
    return out


def _pairs_tree(x):
    """Adjacent pairs first over the last axis, padded with +0.0 to a power of two."""
    n = x.shape[-1]
    p = 1
    while p < n:
        p *= 2
    if p != n:
        x = np.concatenate([x, np.zeros(x.shape[:-1] + (p - n,), x.dtype)], axis=-1)
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def tile_sums(terms):
    """[K, ty * tx] float64 from [K, Hs, Ws] float64: the sum of every 64 x 4 tile of the selected grid in the header's
    order, the tiles in row-major order."""
    K, Hs, Ws = terms.shape
    tx, ty = -(-Ws // COLS), -(-Hs // ROWS)
    pad = np.zeros((K, ty * ROWS, tx * COLS), np.float64)
    pad[:, :Hs, :Ws] = terms
    t = pad.reshape(K, ty, ROWS, tx, COLS)
    col = np.zeros((K, ty, tx, COLS), np.float64)
    for r in range(ROWS):                                             # a tile column, top to bottom, from +0.0
        col = col + t[:, :, r]
    return _pairs_tree(col.reshape(K, ty * tx, COLS))                 # the 64 columns of every tile


def reduce_terms(terms):
    """[K] float64 from [K, Hs, Ws] float64, in the header's order."""
    return _pairs_tree(tile_sums(terms))                              # the tiles in row-major order


def iteration_tile_sums(points, T, model, stride, max_distance, band_tile_rows=None):
    """[31, ty * tx] float64: tile_sums(pixel_terms(...)) of one iteration.  band_tile_rows: evaluate that many tile rows
    at a time (a tile's sum does not depend on the band it is evaluated in, so the bits are the same; the memory is the
    band's)."""
    if band_tile_rows is None:
        return tile_sums(pixel_terms(points, T, model, stride, max_distance))
    rows = int(band_tile_rows) * ROWS * stride                        # frame rows per band: whole tile rows
    assert rows > 0
    H = points[0].shape[0]
    return np.concatenate([tile_sums(pixel_terms(tuple(a[r:r + rows] for a in points), T, model, stride, max_distance))
                           for r in range(0, H, rows)], axis=1)


def solve(S, min_pivot):
    """x (six Python floats) of A x = g by LDL^T without pivoting in the header's order, or None when a pivot is not
    finite or <= min_pivot or a component of x is not finite."""
    A = [[0.0] * 6 for _ in range(6)]
    for k, (i, j) in enumerate(PAIRS):
        A[i][j] = A[j][i] = float(S[k])
    g = [float(S[21 + i]) for i in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    for j in range(6):
        v = [L[j][k] * d[k] for k in range(j)]
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * v[k]
        if not (math.isfinite(s) and s > min_pivot):
            return None
        d[j] = s
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * v[k]
            L[i][j] = s / d[j]
    y = [0.0] * 6
    for i in range(6):
        s = g[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i] / d[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s
    return x if all(math.isfinite(c) for c in x) else None


def cayley(om):
    """C [3, 3] float32 of the rotation vector om (three float32), in the header's operation order."""
    a = [f32(o) * f32(0.5) for o in om]
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    den, k = f32(1.0) + aa, f32(1.0) - aa
    t = [f32(2.0) * x for x in a]
    C = np.empty((3, 3), f32)
    C[0, 0], C[1, 1], C[2, 2] = (k + t[0] * a[0]) / den, (k + t[1] * a[1]) / den, (k + t[2] * a[2]) / den
    C[0, 1], C[0, 2] = (t[0] * a[1] - t[2]) / den, (t[0] * a[2] + t[1]) / den
    C[1, 0], C[1, 2] = (t[1] * a[0] + t[2]) / den, (t[1] * a[2] - t[0]) / den
    C[2, 0], C[2, 1] = (t[2] * a[0] - t[1]) / den, (t[2] * a[1] + t[0]) / den
    return C


def update(T, x):
    """(T' [3, 4] float32, omega.omega, tau.tau) after the twist x."""
    om, tau = [f32(c) for c in x[:3]], [f32(c) for c in x[3:]]
    C = cayley(om)
    out = np.empty((3, 4), f32)
    for r in range(3):
        for c in range(3):
            out[r, c] = (C[r, 0] * T[0, c] + C[r, 1] * T[1, c]) + C[r, 2] * T[2, c]
        out[r, 3] = ((C[r, 0] * T[0, 3] + C[r, 1] * T[1, 3]) + C[r, 2] * T[2, 3]) + tau[r]
    return out, (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2], (tau[0] * tau[0] + tau[1] * tau[1]) + tau[2] * tau[2]


def track_ref(disp, Q, pose_in, model, *, confidence=None, schedule=DEFAULT_SCHEDULE, max_distance=0.3,
              depth_range=(0.0, np.inf), min_confidence=0.0, invalid_disparity=-1.0, min_inliers=100, min_pivot=1e-6,
              rot_eps=0.0, trans_eps=0.0, band_tile_rows=None, keep_tiles=False):
    """One triple: disp [H, W], pose_in [3, 4] / [4, 4] (taken as float32), model: model_view()'s dict.  Returns a dict of
    pose [3, 4] f32, info [4] int32 (lost, iterations, inliers, accepted), rms f32 and sums [30] f64; with keep_tiles
    also tiles [31, ty * tx] f64, the tile sums of the last iteration that ran (None if none did).  band_tile_rows:
    iteration_tile_sums's."""
    pts = frame_points(disp, Q, confidence, min_confidence, depth_range, invalid_disparity)
    T0 = np.ascontiguousarray(np.asarray(pose_in, f32)[:3])
    T = T0.copy()
    info = np.zeros(4, np.int32)
    rms = f32(np.nan)
    sums = np.zeros(TERMS, np.float64)
    done, tiles = False, None
    with np.errstate(all="ignore"):
        for stride, iterations in schedule:
            for _ in range(iterations):
                if done:
                    break
                tiles = iteration_tile_sums(pts, T, model, stride, max_distance, band_tile_rows)
                S = _pairs_tree(tiles)
                sums = S[:TERMS].copy()
                info[1] += 1
                info[2], info[3] = int(S[29]), int(S[TERMS])
                rms = np.sqrt(f32(S[27] / S[28]))
                x = solve(S, float(min_pivot)) if info[2] >= min_inliers else None
                if x is None:
                    info[0], T, done = 1, T0.copy(), True
                    break
                T, ww, tt = update(T, x)
                done = bool(ww <= f32(rot_eps) * f32(rot_eps) and tt <= f32(trans_eps) * f32(trans_eps))
    out = {"pose": T, "info": info, "rms": f32(rms), "sums": sums}
    if keep_tiles:
        out["tiles"] = tiles
    return out


def information(sums):
    """The symmetric 6 x 6 information matrix from the thirty sums."""
    A = np.zeros((6, 6), np.float64)
    for k, (i, j) in enumerate(PAIRS):
        A[i, j] = A[j, i] = sums[k]
    return A


def pose_error(a, b):
    """(metres, degrees) between two poses [3 or 4, 4]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dR = a[:3, :3] @ b[:3, :3].T
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1.0) / 2.0))))
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3])), ang
