"""NumPy twin of smx_tsdf_merge (include/stereo_mi355x.h): the rule restated operation by operation in float32 -- for one
pair with scalars (merge_pair), and for whole volumes with one array operation per step of the rule (merge_ref) -- on the
{"tsdf", "weight", "color"} uint32 word arrays of tests/tsdf_window_ref.py; and NumpyVolume, a host volume with
TSDFVolume's shift and merge built on the two twins, with which cuda_depth.TSDFSpillStore runs without a GPU."""
import numpy as np

import tsdf_window_ref as wref

FILL, AVERAGE = 0, 1
MODES = {"fill": FILL, "average": AVERAGE}


def _f32(word) -> np.float32:
    return np.array([word], np.uint32).view(np.float32)[0]


def _word(value) -> np.uint32:
    return np.array([value], np.float32).view(np.uint32)[0]


def _u8(c: np.float32) -> int:
    """(uint8)floorf(C + 0.5f); NaN stores 0.  The clamp is idle for finite weights."""
    v = np.floor(np.float32(c + np.float32(0.5)))
    if np.isnan(v):
        return 0
    return int(min(max(v, np.float32(0.0)), np.float32(255.0)))


def merge_pair(t0, w0, c0, t1, w1, c1, mode, max_weight):
    """The rule for one pair of words (colour words None without colour): the destination's three words afterwards."""
    W1 = _f32(w1)
    if not W1 > np.float32(0.0):                                      # NaN fails
        return t0, w0, c0
    W0 = _f32(w0)
    if not W0 > np.float32(0.0):
        return t1, w1, c1
    if mode == FILL:
        return t0, w0, c0
    with np.errstate(all="ignore"):
        T0, T1 = _f32(t0), _f32(t1)
        den = np.float32(W0 + W1)
        T = np.float32(np.float32(np.float32(T0 * W0) + np.float32(T1 * W1)) / den)
        W = np.fmin(den, np.float32(max_weight))
        c = None
        if c0 is not None:
            c = 0
            for ch in range(3):
                C0 = np.float32((int(c0) >> (8 * ch)) & 255)
                C1 = np.float32((int(c1) >> (8 * ch)) & 255)
                C = np.float32(np.float32(np.float32(C0 * W0) + np.float32(C1 * W1)) / den)
                c |= _u8(C) << (8 * ch)
            c = np.uint32(c)
    return _word(T), _word(W), c


def merge_ref(dst_state, src_state, placement, region, mode, max_weight):
    """dst_state / src_state: {"tsdf", "weight", "color" (or None)} of uint32 words [nz, ny, nx].  placement = (x0, y0, z0):
    source voxel (0, 0, 0) in destination voxels; region = ((rx, ry, rz), (cx, cy, cz)) in source voxels, or None for the
    whole source.  Returns the destination's new state (new arrays); the inputs are not modified."""
    mode = MODES.get(mode, mode)
    out = {k: None if v is None else v.copy() for k, v in dst_state.items()}
    sz, sy, sx = src_state["weight"].shape
    nz, ny, nx = out["weight"].shape
    (rx, ry, rz), (cx, cy, cz) = ((0, 0, 0), (sx, sy, sz)) if region is None else region
    assert rx >= 0 and ry >= 0 and rz >= 0 and cx >= 1 and cy >= 1 and cz >= 1
    assert rx + cx <= sx and ry + cy <= sy and rz + cz <= sz
    colour = out["color"] is not None
    # the pairs: the region in destination voxels, clipped to the destination grid
    lo = [max(0, o + r) for o, r in zip(placement, (rx, ry, rz))]
    hi = [min(n, o + r + c) for n, o, r, c in zip((nx, ny, nz), placement, (rx, ry, rz), (cx, cy, cz))]
    if any(h <= l for l, h in zip(lo, hi)):
        return out
    dsel = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    ssel = tuple(slice(l - o, h - o) for l, h, o in zip(lo[::-1], hi[::-1], placement[::-1]))
    t0, w0, t1, w1 = out["tsdf"][dsel], out["weight"][dsel], src_state["tsdf"][ssel], src_state["weight"][ssel]
    T0, W0, T1, W1 = (a.view(np.float32) for a in (t0, w0, t1, w1))
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):                                   # every line below is one float32 operation per pair
        measured = W1 > zero                                          # NaN fails
        take = measured & ~(W0 > zero)
        both = measured & ~take if mode == AVERAGE else np.zeros_like(take)
        den = W0 + W1
        a, b = T0 * W0, T1 * W1
        T = (a + b) / den
        W = np.fmin(den, np.float32(max_weight))
        new_t = np.where(take, t1, np.where(both, T.view(np.uint32), t0))
        new_w = np.where(take, w1, np.where(both, W.view(np.uint32), w0))
        if colour:
            c0, c1 = out["color"][dsel], src_state["color"][ssel]
            word = np.zeros(c0.shape, np.uint32)
            for ch in range(3):
                C0 = ((c0 >> np.uint32(8 * ch)) & np.uint32(255)).astype(np.float32)
                C1 = ((c1 >> np.uint32(8 * ch)) & np.uint32(255)).astype(np.float32)
                a, b = C0 * W0, C1 * W1
                C = (a + b) / den
                v = np.floor(C + np.float32(0.5))
                v = np.where(np.isnan(v), zero, np.clip(v, zero, np.float32(255.0)))    # NaN stores 0
                word |= v.astype(np.uint32) << np.uint32(8 * ch)
            out["color"][dsel] = np.where(take, c1, np.where(both, word, c0))
    out["tsdf"][dsel], out["weight"][dsel] = new_t, new_w
    return out


def plausible_state(rng, dims, colour=True, measured=0.6):
    """A state as fusion leaves it: weights finite and >= 0, all-zero words where the weight is 0."""
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    on = rng.random(shape) < measured
    weight = np.where(on, rng.choice(np.array([0.5, 1.0, 2.5, 7.0, 64.0], np.float32), shape), np.float32(0)).astype(np.float32)
    tsdf = np.where(on, rng.uniform(-1, 1, shape), 0).astype(np.float32)
    col = np.where(on, rng.integers(0, 2 ** 24, shape), 0).astype(np.uint32)
    return {"tsdf": tsdf.view(np.uint32).copy(), "weight": weight.view(np.uint32).copy(), "color": col if colour else None}


# a volume moved out and back through a TSDFSpillStore: the steps out; full_path adds the way home
OUT_AND_BACK = [[(3, 0, 0)], [(0, -2, 0)], [(0, 0, 4)], [(-5, 2, -1)], [(70, 0, 0)],
                [(4, 0, 0), (0, 3, 0), (-4, -3, 0)], [(6, 0, 0), (-2, 0, 0), (-4, 0, 0)]]


def full_path(steps):
    """The steps, then the way home in one step if they do not end there."""
    total = tuple(sum(s[a] for s in steps) for a in range(3))
    return steps if total == (0, 0, 0) else steps + [tuple(-c for c in total)]


class NumpyVolume:
    """TSDFVolume's shift, window and merge on host word arrays: what TSDFSpillStore needs of a volume."""

    def __init__(self, state, voxel_size=0.125, origin=(0.0, 0.0, 0.0), *, offset=(0, 0, 0), truncation=0.5,
                 max_weight=64.0, device="host"):
        self.state = {k: None if v is None else np.array(v, np.uint32) for k, v in state.items()}
        nz, ny, nx = self.state["weight"].shape
        self.dims, self.voxel_size, self._origin0, self.offset = (nx, ny, nz), voxel_size, tuple(origin), tuple(offset)
        self.truncation, self.max_weight, self.device = truncation, max_weight, device
        self.merges = 0

    @property
    def _offset(self):
        return self.offset

    @property
    def origin(self):
        return wref.origin_ref(self._origin0, self.offset, self.voxel_size)

    @property
    def color(self):
        return self.state["color"]

    @property
    def tsdf(self):
        return self.state["tsdf"]

    @property
    def weight(self):
        return self.state["weight"]

    def window(self, start, dims):
        return NumpyVolume(wref.window_state(self.state, start, dims), self.voxel_size, self._origin0,
                           offset=tuple(a + b for a, b in zip(self.offset, start)), truncation=self.truncation,
                           max_weight=self.max_weight, device=self.device)

    def shift(self, voxels, *, spill=False, margin=1):
        d = tuple(int(c) for c in voxels)
        if d == (0, 0, 0):
            return []
        boxes = [self.window(s, n) for s, n in wref.spill_boxes_ref(self.dims, d, margin)] if spill else []
        self.state = wref.window_state(self.state, d, self.dims)
        self.offset = tuple(a + b for a, b in zip(self.offset, d))
        return boxes

    def merge(self, other, *, mode="average", region=None):
        assert other._origin0 == self._origin0
        placement = tuple(b - a for a, b in zip(self.offset, other.offset))
        self.state = merge_ref(self.state, other.state, placement, region, mode, self.max_weight)
        self.merges += 1
