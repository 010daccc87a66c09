"""CPU reference of the speckle filter and the hole fill (include/stereo_mi355x.h: smx_filter_speckles,
smx_fill_invalid), in numpy and the standard library.  Written to be obviously correct rather than fast: an explicit
breadth-first search over the 4-neighbour links, and plain per-pixel loops for the fill.  Maps are [H, W] or [n, H, W]
float32; the n maps are independent."""
from collections import deque

import numpy as np


def valid_mask(d: np.ndarray, invalid_disparity: float) -> np.ndarray:
    d = np.asarray(d, np.float32)
    return np.isfinite(d) & (d != np.float32(invalid_disparity))


def _per_map(fn, d, *args):
    d = np.asarray(d, np.float32)
    if d.ndim == 2:
        return fn(d, *args)
    return np.stack([fn(m, *args) for m in d])


def region_sizes(d: np.ndarray, max_diff: float, invalid_disparity: float) -> np.ndarray:
    """[H, W] int64: the size of each valid pixel's region (0 for non-valid pixels)."""
    d = np.asarray(d, np.float32)
    H, W = d.shape
    valid = valid_mask(d, invalid_disparity)
    md = np.float32(max_diff)
    with np.errstate(over="ignore", invalid="ignore"):
        right = valid[:, :-1] & valid[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= md)    # (x, y) -- (x, y + 1)
        down = valid[:-1, :] & valid[1:, :] & (np.abs(d[:-1, :] - d[1:, :]) <= md)     # (x, y) -- (x + 1, y)
    sizes = np.zeros((H, W), np.int64)
    seen = np.zeros((H, W), bool)
    for x0 in range(H):
        for y0 in range(W):
            if not valid[x0, y0] or seen[x0, y0]:
                continue
            region = [(x0, y0)]
            seen[x0, y0] = True
            queue = deque(region)
            while queue:
                x, y = queue.popleft()
                for nx, ny, linked in ((x, y + 1, y + 1 < W and right[x, y]), (x, y - 1, y > 0 and right[x, y - 1]),
                                       (x + 1, y, x + 1 < H and down[x, y]), (x - 1, y, x > 0 and down[x - 1, y])):
                    if linked and not seen[nx, ny]:
                        seen[nx, ny] = True
                        region.append((nx, ny))
                        queue.append((nx, ny))
            for x, y in region:
                sizes[x, y] = len(region)
    return sizes


def _speckles_one(d, max_speckle_size, max_diff, invalid_disparity):
    out = d.copy()
    if max_speckle_size == 0:
        return out
    sizes = region_sizes(d, max_diff, invalid_disparity)
    out[(sizes > 0) & (sizes <= max_speckle_size)] = np.float32(invalid_disparity)
    return out


def filter_speckles(d, max_speckle_size: int, max_diff: float = 1.0, invalid_disparity: float = -1.0) -> np.ndarray:
    return _per_map(_speckles_one, d, max_speckle_size, max_diff, invalid_disparity)


def _fill_one(d, invalid_disparity):
    H, W = d.shape
    valid = valid_mask(d, invalid_disparity)
    out = d.copy()
    # row pass, on the input: nearest valid column on each side, by one sweep in each direction
    for x in range(H):
        if not valid[x].any():
            continue
        left = [-1] * W                                  # nearest valid column < y
        right = [W] * W                                  # nearest valid column > y
        for y in range(1, W):
            left[y] = y - 1 if valid[x, y - 1] else left[y - 1]
        for y in range(W - 2, -1, -1):
            right[y] = y + 1 if valid[x, y + 1] else right[y + 1]
        for y in range(W):
            if valid[x, y]:
                continue
            a, b = left[y], right[y]
            if a >= 0 and b < W:
                va, vb = d[x, a], d[x, b]
                out[x, y] = va if va <= vb else vb
            else:
                out[x, y] = d[x, a] if a >= 0 else d[x, b]
    # column pass, on the result of the row pass
    full = [x for x in range(H) if valid[x].any()]
    if not full:
        return out
    rows = out.copy()
    for x in range(H):
        if valid[x].any():
            continue
        above = [r for r in full if r < x]
        below = [r for r in full if r > x]
        if above and below:
            a, b = rows[above[-1]], rows[below[0]]
            out[x] = np.where(a <= b, a, b)
        else:
            out[x] = rows[above[-1]] if above else rows[below[0]]
    return out


def fill_invalid(d, invalid_disparity: float = -1.0) -> np.ndarray:
    return _per_map(_fill_one, d, invalid_disparity)
