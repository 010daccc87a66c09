"""CPU reference of the image-guided weighted least squares filter (include/stereo_mi355x.h: smx_wls_filter), in numpy.

`wls_filter` is vectorised across the lines of a pass and loops over the positions along them, every operation a
float32 numpy operation (one round-to-nearest, no fused operation, denormals kept).  `wls_filter_loop` states the rule
once more with np.float32 scalars, one line and one element at a time, and the CPU tests check the two against each
other.  Maps are [H, W] or [n, H, W] float32; the n maps are independent."""
import numpy as np

from median_ref import range_index, valid_mask

F = np.float32
ONE, ZERO = F(1.0), F(0.0)
CANONICAL_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def check_tables(lambdas, range_weight):
    lam = np.asarray(lambdas, np.float32)
    rw = np.asarray(range_weight, np.float32)
    assert lam.ndim == 1 and 1 <= lam.size <= 8 and rw.shape == (256,)
    assert np.all(np.isfinite(lam)) and lam.min() >= 0 and lam.max() <= 2.0 ** 20
    assert np.all(np.isfinite(rw)) and rw.min() >= 0 and rw.max() <= 1
    return lam, rw


def planes(d, confidence, invalid_disparity):
    """(U, V) of the rule's steps 1 and 2."""
    d = np.asarray(d, np.float32)
    valid = valid_mask(d, invalid_disparity)
    if confidence is None:
        c = np.where(valid, ONE, ZERO).astype(np.float32)
    else:
        k = np.asarray(confidence, np.float32)
        with np.errstate(invalid="ignore"):
            c = np.where(valid & (k > 0), np.minimum(k, ONE), ZERO).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.where(valid, d * c, ZERO).astype(np.float32)
    return u, c


def solve_lines(f, g, lam, rw):
    """The Thomas solve of step 5 along the last axis of f (any leading shape), guide g of the same shape; f32 in and
    out.  Returns (x, e) for a list of right-hand sides f (they share r and e)."""
    N = g.shape[-1]
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        s = (lam * rw[range_index(g[..., :-1], g[..., 1:])]).astype(np.float32)     # [..., N-1]
        zeros = np.zeros(g.shape[:-1] + (1,), np.float32)
        Lr = np.concatenate([zeros, s], axis=-1)
        Rr = np.concatenate([s, zeros], axis=-1)
        e = np.empty(g.shape, np.float32)
        ys = [np.empty(g.shape, np.float32) for _ in f]
        for j in range(N):
            L, R = Lr[..., j], Rr[..., j]
            b = ((ONE + L) + R).astype(np.float32)
            if j == 0:
                r = (ONE / b).astype(np.float32)
                for y, ff in zip(ys, f):
                    y[..., 0] = ff[..., 0] * r
            else:
                r = (ONE / (b - L * e[..., j - 1])).astype(np.float32)
                for y, ff in zip(ys, f):
                    y[..., j] = (ff[..., j] + L * y[..., j - 1]) * r
            e[..., j] = R * r
        xs = []
        for y in ys:
            x = np.empty(g.shape, np.float32)
            x[..., N - 1] = y[..., N - 1]
            for j in range(N - 2, -1, -1):
                x[..., j] = y[..., j] + e[..., j] * x[..., j + 1]
            xs.append(x)
    return xs


def output(u, v, min_weight, invalid_disparity):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = (u / v).astype(np.float32)
        q = np.where(np.isnan(q), CANONICAL_NAN, q)
        return np.where(v > F(min_weight), q, F(invalid_disparity)).astype(np.float32)


def wls_filter(d, guide, lambdas, range_weight, confidence=None, min_weight=1e-3, invalid_disparity=-1.0):
    """The rule on [H, W] or [n, H, W] maps."""
    lam_t, rw = check_tables(lambdas, range_weight)
    d = np.asarray(d, np.float32)
    g = np.asarray(guide, np.float32)
    two = d.ndim == 2
    if two:
        d, g = d[None], g[None]
        confidence = None if confidence is None else np.asarray(confidence, np.float32)[None]
    u, v = planes(d, confidence, invalid_disparity)
    gt = np.ascontiguousarray(np.swapaxes(g, -1, -2))
    for lam in lam_t:
        u, v = solve_lines([u, v], g, lam, rw)                                     # rows
        ut, vt = solve_lines([np.swapaxes(u, -1, -2), np.swapaxes(v, -1, -2)], gt, lam, rw)   # columns
        u, v = np.swapaxes(ut, -1, -2), np.swapaxes(vt, -1, -2)
    out = output(u, v, min_weight, invalid_disparity)
    return out[0] if two else out


def _solve_line_loop(f, g, lam, rw):
    """Step 5 on one line, np.float32 scalars, straight from the header."""
    N = len(f)
    s = [F(lam * rw[int(range_index(g[j], g[j + 1]))]) for j in range(N - 1)]
    L = [ZERO] + s
    R = s + [ZERO]
    e, y = [ZERO] * N, [ZERO] * N
    for j in range(N):
        b = F(F(ONE + L[j]) + R[j])
        r = F(ONE / b) if j == 0 else F(ONE / F(b - F(L[j] * e[j - 1])))
        e[j] = F(R[j] * r)
        y[j] = F(f[j] * r) if j == 0 else F(F(f[j] + F(L[j] * y[j - 1])) * r)
    x = [ZERO] * N
    x[N - 1] = y[N - 1]
    for j in range(N - 2, -1, -1):
        x[j] = F(y[j] + F(e[j] * x[j + 1]))
    return x


def wls_filter_loop(d, guide, lambdas, range_weight, confidence=None, min_weight=1e-3, invalid_disparity=-1.0):
    """The rule on one [H, W] map, one element at a time (slow: small maps only)."""
    lam_t, rw = check_tables(lambdas, range_weight)
    d = np.asarray(d, np.float32)
    g = np.asarray(guide, np.float32)
    H, W = d.shape
    inv = F(invalid_disparity)
    U = np.zeros((H, W), np.float32)
    V = np.zeros((H, W), np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for i in range(H):
            for j in range(W):
                v = d[i, j]
                if not (np.isfinite(v) and v != inv):
                    continue
                if confidence is None:
                    c = ONE
                else:
                    k = F(confidence[i, j])
                    c = F(min(k, ONE)) if k > 0 else ZERO
                U[i, j] = F(v * c)
                V[i, j] = c
        for lam in lam_t:
            for P in (U, V):
                for i in range(H):
                    P[i, :] = _solve_line_loop(list(P[i, :]), g[i, :], lam, rw)
            for P in (U, V):
                for j in range(W):
                    P[:, j] = _solve_line_loop(list(P[:, j]), g[:, j], lam, rw)
        out = np.empty((H, W), np.float32)
        for i in range(H):
            for j in range(W):
                if V[i, j] > F(min_weight):
                    q = F(U[i, j] / V[i, j])
                    out[i, j] = CANONICAL_NAN if np.isnan(q) else q
                else:
                    out[i, j] = inv
    return out
