"""CPU reference of the image-guided weighted median (include/stereo_mi355x.h: smx_weighted_median), in numpy.

`weighted_median` is vectorised over the window offsets, a chunk of filtered pixels at a time (row-major, so a chunk
is a run of rows): for every pixel it gathers the (2r+1)^2 samples into one row of an array, sorts them by key and takes
the first sample at which twice the running weight reaches the total.  `weighted_median_pixel` states the rule for one
pixel in plain Python, straight from the header, and the CPU tests check the two against each other.  Maps are [H, W] or [n, H, W] float32; the n maps are
independent."""
import numpy as np

SIGN = np.uint32(0x80000000)


def valid_mask(d: np.ndarray, invalid_disparity: float) -> np.ndarray:
    d = np.asarray(d, np.float32)
    return np.isfinite(d) & (d != np.float32(invalid_disparity))


def key(d) -> np.ndarray:
    """uint32 keys of the rule's total order: negative values reversed below the positive ones, -0.0 < +0.0."""
    u = np.asarray(d, np.float32).view(np.uint32)
    return np.where((u & SIGN) != 0, ~u, u | SIGN).astype(np.uint32)


def range_index(gp, gq) -> np.ndarray:
    """k = fabsf(guide[p] - guide[q]) in float32, 255 for NaN or >= 255, else truncated."""
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(np.asarray(gp, np.float32) - np.asarray(gq, np.float32)).astype(np.float32)
        big = ~(a < np.float32(255.0))
        return np.where(big, 255, np.where(big, 0, a).astype(np.int64))


def _check_tables(radius, range_weight, spatial_weight):
    rw = np.asarray(range_weight, np.int64)
    sw = np.asarray(spatial_weight, np.int64)
    assert 1 <= radius <= 15 and rw.shape == (256,) and sw.shape == ((radius + 1) ** 2,)
    assert rw.min() >= 0 and rw.max() <= 1023 and sw.min() >= 0 and sw.max() <= 1023
    return rw, sw


def _filter_set(d, holes, invalid_disparity):
    return valid_mask(d, invalid_disparity) if holes is None else ~valid_mask(holes, invalid_disparity)


def _one_map(d, holes, guide, radius, rw, sw, invalid_disparity):
    d = np.ascontiguousarray(d, np.float32)
    guide = np.asarray(guide, np.float32)
    H, W = d.shape
    out = d.copy()
    valid = valid_mask(d, invalid_disparity)
    fx, fy = np.nonzero(_filter_set(d, holes, invalid_disparity))     # the filtered pixels, row-major
    offsets = [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)
               if sw[abs(dy) * (radius + 1) + abs(dx)] > 0]
    if not offsets or fx.size == 0:
        return out
    S = len(offsets)
    chunk = max(1, (1 << 22) // S)
    for c0 in range(0, fx.size, chunk):
        xs, ys = fx[c0:c0 + chunk], fy[c0:c0 + chunk]
        vals = np.zeros((xs.size, S), np.float32)                     # [pixel, sample]
        wts = np.zeros((xs.size, S), np.int64)
        gp = guide[xs, ys]
        for s, (dy, dx) in enumerate(offsets):
            qx, qy = xs + dy, ys + dx
            inside = (qx >= 0) & (qx < H) & (qy >= 0) & (qy < W)
            cx, cy = np.clip(qx, 0, H - 1), np.clip(qy, 0, W - 1)
            w = sw[abs(dy) * (radius + 1) + abs(dx)] * rw[range_index(gp, guide[cx, cy])]
            wts[:, s] = np.where(inside & valid[cx, cy], w, 0)
            vals[:, s] = d[cx, cy]
        T = wts.sum(axis=1)
        assert T.max() < 2 ** 30
        # 0xFFFFFFFF is the key of a NaN, never a sample's: it sorts the non-samples last
        keys = np.where(wts > 0, key(vals), np.uint32(0xFFFFFFFF))
        order = np.argsort(keys, axis=1, kind="stable")
        cum = np.cumsum(np.take_along_axis(wts, order, axis=1), axis=1)
        first = np.argmax(2 * cum >= T[:, None], axis=1)               # the first sample where 2 * running >= T
        med = np.take_along_axis(vals, np.take_along_axis(order, first[:, None], axis=1), axis=1)[:, 0]
        pick = T > 0
        out[xs[pick], ys[pick]] = med[pick]
    return out


def weighted_median(d, guide, radius, range_weight, spatial_weight, holes=None, invalid_disparity=-1.0):
    """The whole rule on [H, W] or [n, H, W] maps: returns the output map (a new array)."""
    rw, sw = _check_tables(radius, range_weight, spatial_weight)
    d = np.asarray(d, np.float32)
    if d.ndim == 2:
        return _one_map(d, holes, guide, radius, rw, sw, invalid_disparity)
    return np.stack([_one_map(d[i], None if holes is None else holes[i], guide[i], radius, rw, sw, invalid_disparity)
                     for i in range(d.shape[0])])


def weighted_median_pixel(d, guide, x, y, radius, range_weight, spatial_weight, holes=None, invalid_disparity=-1.0):
    """out[x, y] of one [H, W] map by the rule, in plain Python: the filtered set, the samples, T, then the smallest
    key K with 2 * (weight of the samples with key <= K) >= T."""
    rw, sw = _check_tables(radius, range_weight, spatial_weight)
    d = np.asarray(d, np.float32)
    guide = np.asarray(guide, np.float32)
    H, W = d.shape
    in_f = bool(valid_mask(d[x, y], invalid_disparity)) if holes is None else \
        not bool(valid_mask(np.asarray(holes, np.float32)[x, y], invalid_disparity))
    if not in_f:
        return d[x, y]
    samples = []                                                        # (key, weight, value)
    for qx in range(max(0, x - radius), min(H, x + radius + 1)):
        for qy in range(max(0, y - radius), min(W, y + radius + 1)):
            if not valid_mask(d[qx, qy], invalid_disparity):
                continue
            k = int(range_index(guide[x, y], guide[qx, qy]))
            w = int(sw[abs(qx - x) * (radius + 1) + abs(qy - y)]) * int(rw[k])
            if w > 0:
                samples.append((int(key(d[qx, qy])), w, d[qx, qy]))
    T = sum(w for _, w, _ in samples)
    if T == 0:
        return d[x, y]
    for K, _, v in sorted(samples, key=lambda s: s[0]):
        if 2 * sum(w for k, w, _ in samples if k <= K) >= T:
            return v
    raise AssertionError("unreachable: the largest key always qualifies")
