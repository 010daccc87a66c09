"""NumPy twin of smx_tsdf_window (include/stereo_mi355x.h) and of the host arithmetic around it: a window of a volume's
state is a slice copied into a zero array; the spill boxes of a shift and the shift that follows a camera are restated
here independently of cuda_depth (the rounding in exact rational arithmetic)."""
import math
from fractions import Fraction

import numpy as np


def window_ref(src: np.ndarray, start, dims) -> np.ndarray:
    """src: [nz, ny, nx] or [nz, ny, nx, 4] of any dtype; start = (x0, y0, z0), dims = (bx, by, bz).  Destination voxel
    (i, j, k) is source voxel (x0 + i, y0 + j, z0 + k) where that exists, zero bits elsewhere."""
    (x0, y0, z0), (bx, by, bz) = start, dims
    nz, ny, nx = src.shape[:3]
    out = np.zeros((bz, by, bx) + src.shape[3:], src.dtype)
    lo = [max(0, -s) for s in (x0, y0, z0)]                          # destination range with a source, per axis
    hi = [min(b, n - s) for b, n, s in zip((bx, by, bz), (nx, ny, nz), (x0, y0, z0))]
    if all(l < h for l, h in zip(lo, hi)):
        out[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = src[z0 + lo[2]:z0 + hi[2], y0 + lo[1]:y0 + hi[1],
                                                         x0 + lo[0]:x0 + hi[0]]
    return out


def window_state(state: dict, start, dims) -> dict:
    """window_ref of every array of {"tsdf", "weight", "color" (or None)}."""
    return {k: None if v is None else window_ref(v, start, dims) for k, v in state.items()}


def origin_ref(origin, offset, voxel_size):
    """origin + offset * voxel_size per axis in float64."""
    return tuple(float(np.float64(o) + np.float64(k) * np.float64(voxel_size)) for o, k in zip(origin, offset))


def spill_boxes_ref(dims, d, margin):
    """[(start, dims)] of the boxes that leave a volume of `dims` shifted by d, axis by axis: the layers whose index i
    has no place i - d_a in [0, n), grown by `margin` layers toward the staying side, inside the volume."""
    boxes = []
    for a in range(3):
        n = dims[a]
        if d[a] == 0:
            continue
        leaving = [i for i in range(n) if not 0 <= i - d[a] < n]
        first, last = leaving[0], leaving[-1]
        if d[a] > 0:
            last = min(n - 1, last + margin)
        else:
            first = max(0, first - margin)
        start = tuple(first if b == a else 0 for b in range(3))
        size = tuple(last - first + 1 if b == a else dims[b] for b in range(3))
        boxes.append((start, size))
    return boxes


def round_half_away(x: float) -> int:
    """The integer nearest to the float x, halves away from zero, in exact arithmetic."""
    f = Fraction(x)
    r = math.floor(abs(f) + Fraction(1, 2))
    return r if f >= 0 else -r


def follow_shift_ref(position, origin, dims, voxel_size, anchor=(0.5, 0.5, 0.5)):
    """Per axis (position - (origin + anchor * dims * voxel_size)) / voxel_size, each operation in float64, then rounded."""
    out = []
    for p, o, n, a in zip(position, origin, dims, anchor):
        point = np.float64(o) + np.float64(a) * np.float64(n) * np.float64(voxel_size)
        out.append(round_half_away(float((np.float64(p) - point) / np.float64(voxel_size))))
    return tuple(out)


def follow_ref(position, origin, dims, voxel_size, threshold=None, anchor=(0.5, 0.5, 0.5)):
    """The shift TSDFVolume.follow makes: follow_shift_ref once a component reaches the threshold, else (0, 0, 0)."""
    threshold = max(1, min(dims) // 8) if threshold is None else threshold
    d = follow_shift_ref(position, origin, dims, voxel_size, anchor)
    return d if max(abs(c) for c in d) >= threshold else (0, 0, 0)


def random_words(rng, shape) -> np.ndarray:
    """uint32 patterns for a state array: random bits with NaNs (quiet and signalling payloads), infinities, -0.0 and
    denormals planted."""
    w = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = w.reshape(-1)
    special = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFBFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001,
                        0x807FFFFF, 0x00000000], np.uint32)
    at = rng.choice(flat.size, size=min(flat.size, 3 * special.size), replace=False)
    flat[at] = np.resize(special, at.size)
    return w
