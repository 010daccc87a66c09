"""CPU references of the right-view synthesis head (include/stereo_mi355x.h: smx_synthesize_right_view).

synthesize_right_view is the NumPy twin of the rule: float32 arrays, the d loop in the rule's order, one rounding per
operation (NumPy never fuses), np.fmax / np.fmin for the clamp.  It is vectorised over pixels only, which cannot change
a bit, so the HIP kernel must reproduce it bit for bit.

torch_expression is what Deep3D computes after its softmax, restated with torch on the CPU: interpolate the volume, stack
D zero-filled shifted copies of the frame, multiply, sum over the disparity axis, `* 255 + 0.5`, clamp.  It sums in
torch's order, so it agrees with the twin to rounding only (error_bound); it is a check of the rule, not a yardstick for
the kernel."""
import numpy as np

F = np.float32


def taps(length_out: int, scale: int, length_in: int):
    """(i0, i1, l0, l1) of every output index: the half-pixel rule in integers."""
    t = np.arange(length_out, dtype=np.int64)
    u = np.maximum(2 * t + 1 - scale, 0)
    i0 = u // (2 * scale)
    i1 = np.minimum(i0 + 1, length_in - 1)
    l1 = (u % (2 * scale)).astype(F) / F(2 * scale)
    l0 = F(1.0) - l1
    return i0, i1, l0.astype(F), l1.astype(F)


def left_values(left: np.ndarray) -> np.ndarray:
    """The rule's v: float32 as it is, uint8 divided by 255 in float32 (correctly rounded)."""
    if left.dtype == np.uint8:
        return left.astype(F) / F(255.0)
    assert left.dtype == F, left.dtype
    return left


def rescale(acc: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore", over="ignore"):
        return np.fmin(np.fmax(acc.astype(F) * F(255.0) + F(0.5), F(0.0)), F(255.0)).astype(F)


def synthesize_right_view(prob: np.ndarray, left: np.ndarray, scale: int) -> np.ndarray:
    """prob [n, D, h, w] float32, left [n, C, h*scale, w*scale] float32 or uint8 -> [n, C, H, W] float32."""
    assert prob.dtype == F and prob.ndim == 4 and left.ndim == 4
    n, D, h, w = prob.shape
    C, H, W = left.shape[1:]
    assert (H, W) == (h * scale, w * scale) and left.shape[0] == n
    v = left_values(left)
    r0, r1, a0, a1 = taps(H, scale, h)
    c0, c1, b0, b1 = taps(W, scale, w)
    a0, a1 = a0[:, None], a1[:, None]
    acc = np.zeros((n, C, H, W), F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for d in range(min(D, W)):
            P = prob[:, d]                                                  # [n, h, w]
            top = b0 * P[:, r0][:, :, c0] + b1 * P[:, r0][:, :, c1]         # [n, H, W]
            bot = b0 * P[:, r1][:, :, c0] + b1 * P[:, r1][:, :, c1]
            q = (a0 * top + a1 * bot).astype(F)
            acc[..., :W - d] = acc[..., :W - d] + q[:, None, :, :W - d] * v[..., d:]
    assert acc.dtype == F
    return rescale(acc)


def error_bound(D: int) -> float:
    """|twin - torch expression| on outputs in 0..255: two float32 summations of D non-negative terms whose weights sum
    to 1, plus the roundings of the lerps and of the rescale."""
    return 255.0 * 2.0 * (D + 6) * 2.0 ** -24


def torch_expression(prob, left, scale: int):
    """prob [n, D, h, w], left [n, C, H, W] float32 CPU tensors (left in 0..1) -> [n, C, H, W] float32."""
    import torch
    import torch.nn.functional as Fn
    D = prob.shape[1]
    up = Fn.interpolate(prob, scale_factor=scale, mode="bilinear") if scale != 1 else prob
    shifted = []
    for d in range(D):
        s = torch.zeros_like(left)
        if d == 0:
            s = left
        elif d < left.shape[-1]:
            s[..., :-d] = left[..., d:]
        shifted.append(s)
    stack = torch.stack(shifted, dim=1)                                     # [n, D, C, H, W]
    view = torch.sum(torch.mul(up.unsqueeze(2), stack), dim=1)
    return torch.clamp(view * 255 + 0.5, 0, 255)


# ---- inputs the CPU and GPU tests share ----------------------------------------------------------------------------
# (n, C, D, h, w, S): the smallest shapes at which a tiled, chunked kernel can go wrong
SHAPES = [
    (1, 3, 65, 5, 9, 4),        # W = 36 < D: every column has a truncated range
    (2, 3, 65, 7, 40, 4),       # W = 160 > 64 + D, ragged tile rows and columns
    (3, 1, 67, 6, 33, 2),       # odd D, gray
    (1, 3, 5, 9, 70, 1),        # S = 1
    (1, 3, 17, 4, 23, 3),       # S = 3: the weights are not dyadic
    (1, 3, 65, 3, 10, 8),
    (1, 1, 9, 2, 5, 16),
    (1, 3, 1, 4, 70, 4),        # D = 1: the rescale alone
    (1, 3, 2, 4, 70, 4),
    (1, 3, 256, 4, 70, 4),      # several chunks of the disparity axis
    (1, 3, 256, 4, 9, 4),
]


def softmax_noise(rng, n, D, h, w) -> np.ndarray:
    """Softmax over D of N(0, 3^2) logits, float32."""
    logits = rng.normal(0.0, 3.0, (n, D, h, w))
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(F)


def uniform_left(rng, n, C, H, W) -> np.ndarray:
    return rng.random((n, C, H, W)).astype(F)
