"""NumPy reference of smx_sgm, semi-global matching (include/stereo_mi355x.h).

The rule is integer up to one float32 division, so this reference and the kernels give the same bits.  Every step is
vectorised over one image axis; each path is marched with a plain loop along its direction."""
from __future__ import annotations

import numpy as np

F = np.float32
CENSUS_RY, CENSUS_RX = 3, 4                       # 7 rows x 9 columns
CENSUS_OFFSETS = [(dy, dx) for dy in range(-CENSUS_RY, CENSUS_RY + 1) for dx in range(-CENSUS_RX, CENSUS_RX + 1)
                  if (dy, dx) != (0, 0)]          # bit k of the census <-> CENSUS_OFFSETS[k], 62 bits
OUT_OF_IMAGE_COST = 64
DIRECTIONS4 = ((0, 1), (0, -1), (1, 0), (-1, 0))
DIRECTIONS8 = DIRECTIONS4 + ((1, 1), (-1, -1), (1, -1), (-1, 1))
_BIG = 1 << 20                                    # stands for "left out of the min"


def gray(frames) -> np.ndarray:
    """[C,H,W] (C in {1, 3}) uint8 or float32 -> float32 [H,W]: (0.2989 r + 0.5870 g) + 0.1140 b, every operation a
    float32 round-to-nearest, or the single channel as it is."""
    a = np.asarray(frames)
    if a.ndim != 3 or a.shape[0] not in (1, 3):
        raise ValueError(f"frames must be [C,H,W] with C in (1, 3), got {a.shape}")
    a = a.astype(F)
    if a.shape[0] == 1:
        return a[0].copy()
    with np.errstate(all="ignore"):
        return (F(0.2989) * a[0] + F(0.5870) * a[1]) + F(0.1140) * a[2]


def census(g: np.ndarray) -> np.ndarray:
    """float32 [H,W] -> uint64 [H,W]: bit k set when the neighbour at CENSUS_OFFSETS[k], its coordinates clamped into
    the image, is < the centre (IEEE: a NaN on either side gives 0)."""
    H, W = g.shape
    ys, xs = np.arange(H), np.arange(W)
    out = np.zeros((H, W), np.uint64)
    with np.errstate(invalid="ignore"):
        for k, (dy, dx) in enumerate(CENSUS_OFFSETS):
            nb = g[np.clip(ys + dy, 0, H - 1)][:, np.clip(xs + dx, 0, W - 1)]
            out |= (nb < g).astype(np.uint64) << np.uint64(k)
    return out


def _popcount64(a: np.ndarray) -> np.ndarray:
    b = a.view(np.uint8).reshape(a.shape + (8,))
    return np.unpackbits(b, axis=-1).sum(axis=-1, dtype=np.int32)


def cost_volume(cl: np.ndarray, cr: np.ndarray, min_disparity: int, D: int) -> np.ndarray:
    """int32 [H,W,D]: C(y,x,i) = popcount(cl(y,x) ^ cr(y, x - dmin - i)), or 64 when that column is < 0."""
    H, W = cl.shape
    C = np.full((H, W, D), OUT_OF_IMAGE_COST, np.int32)
    for i in range(D):
        s = min_disparity + i
        if s < W:
            C[:, s:, i] = _popcount64(np.bitwise_xor(cl[:, s:], cr[:, :W - s]))
    return C


def _step(Cp: np.ndarray, Lq: np.ndarray, P1: int, P2: int) -> np.ndarray:
    """One recurrence step over [..., D]: Lq is the predecessor's L."""
    M = Lq.min(axis=-1, keepdims=True)
    best = np.minimum(Lq, M + P2)
    best[..., 1:] = np.minimum(best[..., 1:], Lq[..., :-1] + P1)
    best[..., :-1] = np.minimum(best[..., :-1], Lq[..., 1:] + P1)
    return Cp + best - M


def path_cost(C: np.ndarray, direction, P1: int, P2: int) -> np.ndarray:
    """L_r over the whole image for r = direction = (dy, dx): int32 [H,W,D]."""
    H, W, D = C.shape
    dy, dx = direction
    L = np.empty_like(C)
    if dy == 0:                                   # march along x, all rows at once
        order = range(W) if dx > 0 else range(W - 1, -1, -1)
        for k, x in enumerate(order):
            L[:, x] = C[:, x] if k == 0 else _step(C[:, x], L[:, x - dx], P1, P2)
        return L
    order = range(H) if dy > 0 else range(H - 1, -1, -1)
    for k, y in enumerate(order):
        L[y] = C[y]
        if k == 0:
            continue
        xs = np.arange(W)
        xq = xs - dx
        has = (xq >= 0) & (xq < W)
        L[y, has] = _step(C[y, has], L[y - dy, xq[has]], P1, P2)
    return L


def aggregate(C: np.ndarray, paths: int, P1: int, P2: int) -> np.ndarray:
    """S = sum of L_r over the 4 or 8 directions: int32 [H,W,D]."""
    if paths not in (4, 8):
        raise ValueError(f"paths must be 4 or 8, got {paths}")
    S = np.zeros_like(C)
    for r in (DIRECTIONS4 if paths == 4 else DIRECTIONS8):
        L = path_cost(C, r, P1, P2)
        assert L.max() <= 255, "L_r above 255 with 0 <= P1 <= P2 <= 191"
        S += L
    return S


def right_wta(S: np.ndarray, min_disparity: int) -> np.ndarray:
    """iR(y, x'): the smallest i that minimises S(y, x' + dmin + i, i) over the i with x' + dmin + i <= W - 1, or -1
    when there is none.  int32 [H,W]."""
    H, W, D = S.shape
    Sr = np.full((H, W, D), _BIG, np.int64)
    for i in range(D):
        s = min_disparity + i
        if s < W:
            Sr[:, :W - s, i] = S[:, s:, i]
    iR = Sr.argmin(axis=-1).astype(np.int32)
    iR[Sr.min(axis=-1) >= _BIG] = -1
    return iR


def select(S: np.ndarray, min_disparity: int, uniqueness: int = 0, lr_max_diff: float = -1.0, subpixel: bool = True,
           invalid_disparity: float = -1.0) -> np.ndarray:
    """Winner, invalid pixels and value of the rule: float32 [H,W]."""
    H, W, D = S.shape
    S = S.astype(np.int64)
    ist = S.argmin(axis=-1)                                       # first minimum: the smallest i
    s0 = np.take_along_axis(S, ist[..., None], -1)[..., 0]
    d = min_disparity + ist
    xs = np.broadcast_to(np.arange(W)[None, :], (H, W))
    bad = xs - d < 0                                              # (a)
    if uniqueness:
        far = np.abs(np.arange(D)[None, None, :] - ist[..., None]) > 1
        m2 = np.where(far, S, _BIG).min(axis=-1)
        bad |= m2 * (100 - uniqueness) < s0 * 100                 # (b)
    if lr_max_diff >= 0:
        iR = right_wta(S, min_disparity)
        ys = np.broadcast_to(np.arange(H)[:, None], (H, W))
        xr = np.clip(xs - d, 0, W - 1)
        diff = np.abs(min_disparity + iR[ys, xr] - d).astype(F)
        bad |= (xs - d >= 0) & (diff > F(lr_max_diff))            # (c)
    out = d.astype(F)
    if subpixel and D >= 3:
        inner = (ist > 0) & (ist < D - 1)
        im, ip = np.clip(ist - 1, 0, D - 1), np.clip(ist + 1, 0, D - 1)
        sm = np.take_along_axis(S, im[..., None], -1)[..., 0]
        sp = np.take_along_axis(S, ip[..., None], -1)[..., 0]
        den = sm + sp - 2 * s0
        use = inner & (den > 0)
        with np.errstate(all="ignore"):
            frac = (sm - sp).astype(F) / (2 * np.maximum(den, 1)).astype(F)
        out = np.where(use, out + frac, out).astype(F)
    return np.where(bad, F(invalid_disparity), out).astype(F)


def sgm_pair(left, right, min_disparity: int, num_disparities: int, *, paths: int = 8, P1: int = 10, P2: int = 120,
             uniqueness: int = 0, lr_max_diff: float = -1.0, subpixel: bool = True, invalid_disparity: float = -1.0):
    """One pair of [C,H,W] frames -> (float32 [H,W] disparity, float32 [H,W] left gray plane)."""
    if not 0 <= P1 <= P2 <= 191:
        raise ValueError(f"need 0 <= P1 <= P2 <= 191, got {P1}, {P2}")
    gl, gr = gray(left), gray(right)
    C = cost_volume(census(gl), census(gr), min_disparity, num_disparities)
    S = aggregate(C, paths, P1, P2)
    return select(S, min_disparity, uniqueness, lr_max_diff, subpixel, invalid_disparity), gl


def sgm_ref(left, right, min_disparity: int, num_disparities: int, **kwargs):
    """[C,H,W] or [n,C,H,W] frames -> (disparity [H,W] / [n,H,W], left gray of the same shape), both float32."""
    left, right = np.asarray(left), np.asarray(right)
    if left.ndim == 3:
        return sgm_pair(left, right, min_disparity, num_disparities, **kwargs)
    res = [sgm_pair(l, r, min_disparity, num_disparities, **kwargs) for l, r in zip(left, right)]
    return np.stack([d for d, _ in res]), np.stack([g for _, g in res])


def wta_raw(left, right, min_disparity: int, num_disparities: int) -> np.ndarray:
    """The arg-min of the raw census cost, no paths: int32 [H,W] disparities."""
    C = cost_volume(census(gray(left)), census(gray(right)), min_disparity, num_disparities)
    return min_disparity + C.argmin(axis=-1).astype(np.int32)
