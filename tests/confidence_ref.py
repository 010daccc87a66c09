"""CPU reference of the per-pixel confidence (include/stereo_mi355x.h: smx_confidence_map), in numpy.

`confidence_map` is vectorised: the LR term gathers D_R along each row, the texture term takes the window's max and min
as a separable sliding max / min over the edge-padded guide (NaN entering the max as -inf and the min as +inf), every
arithmetic step a float32 numpy operation (one round-to-nearest, no fused operation, denormals kept).
`confidence_map_loop` restates the rule with np.float32 scalars, one pixel and one window value at a time, and the CPU
tests check the two against each other.  Maps are [H, W] or [n, H, W] float32; the n maps are independent."""
import numpy as np

from median_ref import valid_mask

F = np.float32
ONE, ZERO, HALF = F(1.0), F(0.0), F(0.5)


def check_params(radius, lr_scale, texture_scale, invalid_disparity, has_guide):
    assert np.isfinite(lr_scale) and lr_scale > 0
    assert np.isfinite(texture_scale) and texture_scale > 0
    assert np.isfinite(invalid_disparity)
    assert not has_guide or 1 <= radius <= 15


def lr_term(d, right, lr_scale, invalid_disparity):
    """(ok, c_lr) of step 2 on [n, H, W] maps: ok is False where the pixel points outside the row or at a non-valid
    right-view value."""
    n, H, W = d.shape
    Y = np.arange(W)[None, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((d + HALF).astype(np.float32))
        inb = (t >= 0) & (t <= Y)
        idx = np.where(inb, Y - np.where(inb, t, 0).astype(np.int64), 0)
        r = np.take_along_axis(right, idx, axis=2)
        ok = inb & valid_mask(r, invalid_disparity)
        e = np.abs((d - r).astype(np.float32))
        c = np.maximum(ZERO, (ONE - (e / F(lr_scale)).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return ok, c


def _slide(a, radius, axis, op):
    """op (np.maximum or np.minimum) over the 2 radius + 1 values along `axis` of an array padded by radius on it."""
    m = a.shape[axis] - 2 * radius
    out = np.take(a, range(0, m), axis=axis)
    for j in range(1, 2 * radius + 1):
        out = op(out, np.take(a, range(j, j + m), axis=axis))
    return out


def texture_term(guide, radius, texture_scale):
    """c_tex of step 3 on [n, H, W] guides."""
    g = np.pad(np.asarray(guide, np.float32), ((0, 0), (radius, radius), (radius, radius)), mode="edge")
    nan = np.isnan(g)
    gmax = np.where(nan, F(-np.inf), g).astype(np.float32)
    gmin = np.where(nan, F(np.inf), g).astype(np.float32)
    mx = _slide(_slide(gmax, radius, 2, np.maximum), radius, 1, np.maximum)
    mn = _slide(_slide(gmin, radius, 2, np.minimum), radius, 1, np.minimum)
    with np.errstate(invalid="ignore", over="ignore"):
        rng = (mx - mn).astype(np.float32)
        bad = ~(mx >= mn) | np.isnan(rng)
        rng = np.where(rng == 0, ZERO, rng).astype(np.float32)          # -0.0 and +0.0 count as equal
        c = np.minimum(ONE, (rng / F(texture_scale)).astype(np.float32)).astype(np.float32)
    return np.where(bad, ZERO, c).astype(np.float32)


def confidence_map(d, right=None, guide=None, radius=2, lr_scale=1.0, texture_scale=10.0, invalid_disparity=-1.0):
    """The rule on [H, W] or [n, H, W] maps; right and guide may each be None."""
    check_params(radius, lr_scale, texture_scale, invalid_disparity, guide is not None)
    d = np.asarray(d, np.float32)
    two = d.ndim == 2
    if two:
        d = d[None]
        right = None if right is None else np.asarray(right, np.float32)[None]
        guide = None if guide is None else np.asarray(guide, np.float32)[None]
    ok = valid_mask(d, invalid_disparity)
    c_lr = np.ones(d.shape, np.float32)
    if right is not None:
        ok_lr, c_lr = lr_term(d, np.asarray(right, np.float32), lr_scale, invalid_disparity)
        ok &= ok_lr
    c_tex = np.ones(d.shape, np.float32) if guide is None else texture_term(guide, radius, texture_scale)
    out = np.where(ok, (c_lr * c_tex).astype(np.float32), ZERO).astype(np.float32)
    return out[0] if two else out


def confidence_map_loop(d, right=None, guide=None, radius=2, lr_scale=1.0, texture_scale=10.0,
                        invalid_disparity=-1.0):
    """The rule on one [H, W] map, one pixel at a time, straight from the header (slow: small maps only)."""
    check_params(radius, lr_scale, texture_scale, invalid_disparity, guide is not None)
    d = np.asarray(d, np.float32)
    H, W = d.shape
    inv = F(invalid_disparity)

    def valid(v):
        return bool(np.isfinite(v)) and v != inv

    out = np.zeros((H, W), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for X in range(H):
            for Y in range(W):
                v = F(d[X, Y])
                if not valid(v):
                    continue
                c_lr = ONE
                if right is not None:
                    t = F(np.floor(F(v + HALF)))
                    if not (t >= 0 and t <= Y):
                        continue
                    r = F(right[X, Y - int(t)])
                    if not valid(r):
                        continue
                    e = F(abs(F(v - r)))
                    c_lr = F(max(ZERO, F(ONE - F(e / F(lr_scale)))))
                c_tex = ONE
                if guide is not None:
                    vals = [F(guide[min(max(X + i, 0), H - 1), min(max(Y + j, 0), W - 1)])
                            for i in range(-radius, radius + 1) for j in range(-radius, radius + 1)]
                    vals = [g for g in vals if not np.isnan(g)]
                    if not vals:
                        continue
                    rng = F(F(max(vals)) - F(min(vals)))
                    if np.isnan(rng):
                        continue
                    if rng == 0:
                        rng = ZERO
                    c_tex = F(min(ONE, F(rng / F(texture_scale))))
                out[X, Y] = F(c_lr * c_tex)
    return out
