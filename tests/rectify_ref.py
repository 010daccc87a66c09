"""CPU reference of the rectification remap (include/stereo_mi355x.h: smx_remap_pairs), of the map builder and of the
map quantisation (cuda_depth.rectification_map / quantize_map), in numpy.

`remap` is vectorised over the output pixels: integer arithmetic for uint8, float32 arrays in the stated order for float32
(numpy does not fuse).  `remap_pixel` states the rule for one pixel in plain Python, straight from the header, and the CPU
tests check the two against each other.  Images are [n, C, H, W]; the map is int32 [H_out, W_out, 2] (x, y) in 1/32 pixel."""
import numpy as np

CONSTANT, REPLICATE = 0, 1
CANONICAL_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]   # every NaN result


def taps(qmap, Hi, Wi, border):
    """(rows [4, Ho, Wo], cols [4, Ho, Wo] clamped, inside [4, Ho, Wo], weights [4, Ho, Wo] int64), tap order 00 01 10 11."""
    q = np.asarray(qmap, np.int64)                          # 64 bits: x0 + 1 cannot overflow
    x0, y0 = q[..., 0] >> 5, q[..., 1] >> 5
    fx, fy = q[..., 0] & 31, q[..., 1] & 31
    ys = np.stack([y0, y0, y0 + 1, y0 + 1])
    xs = np.stack([x0, x0 + 1, x0, x0 + 1])
    inside = (ys >= 0) & (ys < Hi) & (xs >= 0) & (xs < Wi)
    w = np.stack([(32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy])
    return np.clip(ys, 0, Hi - 1), np.clip(xs, 0, Wi - 1), inside | (border == REPLICATE), w


def remap(img, qmap, border=CONSTANT, border_value=0):
    img = np.asarray(img)
    n, C, Hi, Wi = img.shape
    ys, xs, inside, w = taps(qmap, Hi, Wi, border)
    p = img[:, :, ys, xs]                                   # [n, C, 4, Ho, Wo]
    if img.dtype == np.uint8:
        p = np.where(inside, p.astype(np.int64), int(border_value))
        return ((np.sum(w * p, axis=2) + 512) >> 10).astype(np.uint8)
    assert img.dtype == np.float32
    p = np.where(inside, p, np.float32(border_value)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.where(w != 0, w.astype(np.float32) * p, np.float32(0.0)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (((a[:, :, 0] + a[:, :, 1]) + (a[:, :, 2] + a[:, :, 3])) * np.float32(0.0009765625)).astype(np.float32)
    return np.where(np.isnan(r), CANONICAL_NAN, r)


def remap_pixel(img, qmap, i, c, v, u, border=CONSTANT, border_value=0):
    """One output value, in plain Python ints (and numpy float32 scalars for float32)."""
    Hi, Wi = img.shape[-2:]
    qx, qy = int(qmap[v, u, 0]), int(qmap[v, u, 1])
    x0, y0, fx, fy = qx >> 5, qy >> 5, qx & 31, qy & 31
    weights = ((32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy)
    vals = []
    for (dy, dx), wk in zip(((0, 0), (0, 1), (1, 0), (1, 1)), weights):
        y, x = y0 + dy, x0 + dx
        if border == REPLICATE:
            y, x = min(max(y, 0), Hi - 1), min(max(x, 0), Wi - 1)
        inside = 0 <= y < Hi and 0 <= x < Wi
        vals.append((wk, img[i, c, y, x] if inside else border_value))
    if img.dtype == np.uint8:
        return (sum(wk * int(p) for wk, p in vals) + 512) >> 10
    f = np.float32
    a = [f(0.0) if wk == 0 else f(wk) * f(p) for wk, p in vals]
    with np.errstate(invalid="ignore", over="ignore"):
        r = f(f(f(a[0] + a[1]) + f(a[2] + a[3])) * f(0.0009765625))
    return CANONICAL_NAN if np.isnan(r) else r


def rectification_map(K, dist, R, P, out_shape):
    """float64 (map_x, map_y) of initUndistortRectifyMap's model; NaN where X2 <= 0 or the result is not finite."""
    Ho, Wo = out_shape
    K, R = np.asarray(K, float).reshape(3, 3), np.asarray(R, float).reshape(3, 3)
    P = np.asarray(P, float).reshape(3, -1)[:, :3]
    k1, k2, p1, p2, k3 = (list(np.asarray(dist, float).reshape(-1)) + [0.0] * 5)[:5]
    v, u = np.mgrid[0:Ho, 0:Wo].astype(float)
    X = np.einsum("ij,jhw->ihw", np.linalg.inv(P @ R), np.stack([u, v, np.ones_like(u)]))
    with np.errstate(all="ignore"):
        x, y = X[0] / X[2], X[1] / X[2]
        r2 = x * x + y * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * kr + p1 * (2 * x * y) + p2 * (r2 + 2 * x * x)
        yd = y * kr + p1 * (r2 + 2 * y * y) + p2 * (2 * x * y)
        mx = K[0, 0] * xd + K[0, 1] * yd + K[0, 2]
        my = K[1, 1] * yd + K[1, 2]
    bad = ~(X[2] > 0) | ~np.isfinite(mx) | ~np.isfinite(my)
    mx[bad] = np.nan
    my[bad] = np.nan
    return mx, my


def quantize_map(map_x, map_y, in_shape):
    Hi, Wi = in_shape
    out = []
    for m, hi in ((map_x, (Wi + 1) * 32), (map_y, (Hi + 1) * 32)):
        with np.errstate(all="ignore"):
            f = np.floor(np.asarray(m, float) * 32.0 + 0.5)
        out.append(np.where(np.isfinite(f), np.clip(f, -64, hi), -64).astype(np.int32))
    return np.stack(out, axis=-1)


def valid_mask(qmap, in_shape):
    """Output pixels whose taps of non-zero weight all lie inside the input."""
    Hi, Wi = in_shape
    ys, xs, inside, w = taps(qmap, Hi, Wi, CONSTANT)
    return np.all(inside | (w == 0), axis=0)
