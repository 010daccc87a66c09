"""CPU reference of the motion-gated temporal filter (include/stereo_mi355x.h: smx_temporal_filter), in numpy.

`temporal_step` is vectorised: |g - G| over the edge-padded planes (padding is the rule's clamping), the window sum as
row sums in dx order then column sums in dy order, and the per-pixel cases as masks, every arithmetic step a float32
numpy operation (one round-to-nearest, no fused operation, denormals kept).  `temporal_step_loop` restates the rule
with np.float32 scalars, one pixel and one window value at a time, and the CPU tests check the two against each other.
`TemporalRef` carries the state and the previous guide across calls, as cuda_depth.TemporalFilter does.
Maps are [H, W] or [n, H, W] float32; the n maps are independent streams."""
import numpy as np

from median_ref import valid_mask

F = np.float32
ZERO, ONE = F(0.0), F(1.0)
DEFAULTS = dict(motion_radius=1, motion_threshold=4.0, decay=0.8, max_diff=1.0, max_weight=8.0, min_weight=0.25,
                invalid_disparity=-1.0)


def check_params(motion_radius, motion_threshold, decay, max_diff, max_weight, min_weight, invalid_disparity):
    assert 0 <= motion_radius <= 7
    assert np.isfinite(motion_threshold) and motion_threshold >= 0
    assert 0 < F(decay) <= 1
    assert np.isfinite(max_diff) and max_diff >= 0
    assert np.isfinite(max_weight) and max_weight > 0
    assert np.isfinite(min_weight) and min_weight >= 0
    assert np.isfinite(invalid_disparity)


def threshold(motion_radius, motion_threshold):
    """T = motion_threshold * (float)(2R+1)^2, one float32 product."""
    with np.errstate(over="ignore"):
        return F(F(motion_threshold) * F((2 * motion_radius + 1) ** 2))


def motion_sum(guide, prev_guide, motion_radius):
    """S of step 1 on [n, H, W] planes: row sums in dx order, then their sum in dy order."""
    R = motion_radius
    n, H, W = guide.shape
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs((np.asarray(guide, F) - np.asarray(prev_guide, F)).astype(F)).astype(F)
        ep = np.pad(e, ((0, 0), (R, R), (R, R)), mode="edge")
        r = ep[:, :, 0:W]
        for j in range(1, 2 * R + 1):
            r = (r + ep[:, :, j:j + W]).astype(F)
        s = r[:, 0:H, :]
        for j in range(1, 2 * R + 1):
            s = (s + r[:, j:j + H, :]).astype(F)
    return s


def static_mask(guide, prev_guide, motion_radius=1, motion_threshold=4.0):
    """STATIC of step 1 on [H, W] or [n, H, W] planes."""
    g, G = np.asarray(guide, F), np.asarray(prev_guide, F)
    two = g.ndim == 2
    s = motion_sum(g[None] if two else g, G[None] if two else G, motion_radius)
    with np.errstate(invalid="ignore"):
        m = s <= threshold(motion_radius, motion_threshold)
    return m[0] if two else m


def temporal_step(d, c, g, G, D, A, motion_radius=1, motion_threshold=4.0, decay=0.8, max_diff=1.0, max_weight=8.0,
                  min_weight=0.25, invalid_disparity=-1.0):
    """One call of the rule: (out, D', A') from the map d, the confidence c (or None), the guides g and G and the state
    (D, A), all [H, W] or [n, H, W].  guide_out is g itself."""
    check_params(motion_radius, motion_threshold, decay, max_diff, max_weight, min_weight, invalid_disparity)
    d, g, G, D, A = (np.asarray(x, F) for x in (d, g, G, D, A))
    inv = F(invalid_disparity)
    still = static_mask(g, G, motion_radius, motion_threshold)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dv = valid_mask(d, inv)
        if c is None:
            w = np.where(dv, ONE, ZERO).astype(F)
        else:
            c = np.asarray(c, F)
            w = np.where(dv & (c > 0), np.minimum(c, ONE), ZERO).astype(F)
        a = (A * F(decay)).astype(F)
        hist = (a > 0) & still & valid_mask(D, inv)
        agree = dv & hist & (np.abs((d - D).astype(F)) <= F(max_diff))
        hold = ~dv & hist & (a >= F(min_weight))
        sw = (a + w).astype(F)
        blend = (((a * D).astype(F) + (w * d).astype(F)).astype(F) / sw).astype(F)
        out = np.select([agree, dv, hold], [blend, d, D], inv).astype(F)
        new_a = np.select([agree, dv, hold], [np.minimum(sw, F(max_weight)), w, a], ZERO).astype(F)
    return out, out.copy(), new_a


def temporal_step_loop(d, c, g, G, D, A, motion_radius=1, motion_threshold=4.0, decay=0.8, max_diff=1.0,
                       max_weight=8.0, min_weight=0.25, invalid_disparity=-1.0):
    """The rule on one [H, W] map, one pixel at a time, straight from the header (slow: small maps only)."""
    check_params(motion_radius, motion_threshold, decay, max_diff, max_weight, min_weight, invalid_disparity)
    d, g, G, D, A = (np.asarray(x, F) for x in (d, g, G, D, A))
    H, W = d.shape
    R = motion_radius
    inv = F(invalid_disparity)
    T = threshold(R, motion_threshold)

    def valid(v):
        return bool(np.isfinite(v)) and v != inv

    def e(x, y):
        x, y = min(max(x, 0), H - 1), min(max(y, 0), W - 1)
        return F(abs(F(g[x, y] - G[x, y])))

    out = np.empty((H, W), F)
    new_a = np.empty((H, W), F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for X in range(H):
            for Y in range(W):
                S = None
                for dy in range(-R, R + 1):
                    r = e(X + dy, Y - R)
                    for dx in range(-R + 1, R + 1):
                        r = F(r + e(X + dy, Y + dx))
                    S = r if S is None else F(S + r)
                still = bool(S <= T)
                dd, DD, AA = F(d[X, Y]), F(D[X, Y]), F(A[X, Y])
                w = ZERO
                if valid(dd):
                    if c is None:
                        w = ONE
                    else:
                        cc = F(c[X, Y])
                        w = F(min(cc, ONE)) if cc > 0 else ZERO
                a = F(AA * F(decay))
                hist = bool(a > 0) and still and valid(DD)
                if valid(dd) and hist and F(abs(F(dd - DD))) <= F(max_diff):
                    o = F(F(F(a * DD) + F(w * dd)) / F(a + w))
                    na = F(min(F(a + w), F(max_weight)))
                elif valid(dd):
                    o, na = dd, w
                elif hist and a >= F(min_weight):
                    o, na = DD, a
                else:
                    o, na = inv, ZERO
                out[X, Y], new_a[X, Y] = o, na
    return out, out.copy(), new_a


class TemporalRef:
    """The filter's state across calls, as cuda_depth.TemporalFilter keeps it: D starts at invalid_disparity, A at 0 and
    the previous guide at 0."""

    def __init__(self, shape, **params):
        self.params = dict(DEFAULTS, **params)
        self.D = np.full(shape, F(self.params["invalid_disparity"]), F)
        self.A = np.zeros(shape, F)
        self.G = np.zeros(shape, F)

    def reset(self, streams=None):
        if streams is None:
            self.A[...] = 0
            self.D[...] = F(self.params["invalid_disparity"])
        else:
            for i in streams:
                self.A[i] = 0
                self.D[i] = F(self.params["invalid_disparity"])

    def apply(self, d, g, c=None, step=temporal_step):
        out, self.D, self.A = step(d, c, g, self.G, self.D, self.A, **self.params)
        self.G = np.array(g, F)
        return out


def temporal_std(maps, invalid_disparity=-1.0, scored=None):
    """Mean over pixels valid in every frame (and in `scored`) of the per-pixel standard deviation across frames."""
    maps = np.asarray(maps, np.float64)
    keep = np.all(valid_mask(maps.astype(F), invalid_disparity), axis=0)
    if scored is not None:
        keep &= scored
    return float(maps.std(axis=0)[keep].mean())


def toggle_rate(maps, invalid_disparity=-1.0, scored=None):
    """Fraction of (pixel, consecutive frame pair) where the pixel changes between valid and not valid."""
    v = valid_mask(np.asarray(maps, F), invalid_disparity)
    t = v[1:] != v[:-1]
    if scored is not None:
        t = t[:, scored]
    return float(t.mean())
