"""CPU references of the synthesis head's training form and backward (include/stereo_mi355x.h:
smx_synthesis_head_forward, smx_synthesis_head_backward).

head_forward is synthesis_ref's twin without its rescale.  head_backward follows the header's rule literally: float32
arrays, the plane gradient channel by channel, the two transposes as walks over Y and X in ascending order with one
rounding per operation (NumPy never fuses), vectorised only over axes that are not summed.  With dtype=np.float64 the
same walk is the exact-order evaluation the error bound is measured against; `absolute=True` gives the bound's A, the
same sums over absolute values."""
import numpy as np

import synthesis_ref as ref

F = np.float32

# (n, C, D, h, w, S)
SHAPES = ref.SHAPES + [
    (1, 3, 7, 1, 1, 4),         # one low-resolution cell per axis: both taps hit the same cell everywhere
    (2, 1, 9, 3, 1, 2),
    (1, 3, 7, 1, 3, 5),         # odd S, up to 12 terms
    (1, 3, 9, 37, 45, 2),       # several workgroup tiles in both low-resolution axes at a small D
    (1, 1, 5, 70, 70, 1),
]


def head_forward(prob: np.ndarray, left: np.ndarray, scale: int) -> np.ndarray:
    """The training form: synthesis_ref.synthesize_right_view up to and including acc_c."""
    assert prob.dtype == F and prob.ndim == 4 and left.ndim == 4
    n, D, h, w = prob.shape
    C, H, W = left.shape[1:]
    assert (H, W) == (h * scale, w * scale) and left.shape[0] == n
    v = ref.left_values(left)
    r0, r1, a0, a1 = ref.taps(H, scale, h)
    c0, c1, b0, b1 = ref.taps(W, scale, w)
    a0, a1 = a0[:, None], a1[:, None]
    acc = np.zeros((n, C, H, W), F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for d in range(min(D, W)):
            P = prob[:, d]
            top = b0 * P[:, r0][:, :, c0] + b1 * P[:, r0][:, :, c1]
            bot = b0 * P[:, r1][:, :, c0] + b1 * P[:, r1][:, :, c1]
            q = (a0 * top + a1 * bot).astype(F)
            acc[..., :W - d] = acc[..., :W - d] + q[:, None, :, :W - d] * v[..., d:]
    assert acc.dtype == F
    return acc


def head_backward(grad_view: np.ndarray, left: np.ndarray, D: int, scale: int, dtype=F, absolute: bool = False):
    """grad_view [n, C, H, W] float32, left [n, C, H, W] float32 or uint8 -> grad_prob [n, D, h, w] of `dtype`."""
    assert grad_view.dtype == F and grad_view.ndim == 4 and grad_view.shape == left.shape
    n, C, H, W = grad_view.shape
    assert H % scale == 0 and W % scale == 0
    h, w = H // scale, W // scale
    T_ = dtype
    g = grad_view.astype(T_)
    v = ref.left_values(left).astype(T_)                                    # the division is float32 in every case
    r0, r1, a0, a1 = ref.taps(H, scale, h)
    c0, c1, b0, b1 = ref.taps(W, scale, w)
    a0, a1, b0, b1 = (t.astype(T_) for t in (a0, a1, b0, b1))
    if absolute:
        g, v = np.abs(g), np.abs(v)
    out = np.zeros((n, D, h, w), T_)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for d in range(min(D, W)):
            Wd = W - d                                                      # the columns with Y + d < W
            G = g[:, 0, :, :Wd] * v[:, 0, :, d:]
            for c in range(1, C):
                G = G + g[:, c, :, :Wd] * v[:, c, :, d:]
            T = np.zeros((n, H, w), T_)
            for Y in range(Wd):                                             # ascending; b0 first
                T[:, :, c0[Y]] = T[:, :, c0[Y]] + b0[Y] * G[:, :, Y]
                T[:, :, c1[Y]] = T[:, :, c1[Y]] + b1[Y] * G[:, :, Y]
            acc = np.zeros((n, h, w), T_)
            for X in range(H):
                acc[:, r0[X]] = acc[:, r0[X]] + a0[X] * T[:, X]
                acc[:, r1[X]] = acc[:, r1[X]] + a1[X] * T[:, X]
            out[:, d] = acc
    assert out.dtype == T_
    return out


def torch_view_expression(prob, left, scale: int):
    """synthesis_ref.torch_expression without its last line: what Deep3D's loss sees.  prob [n, D, h, w], left
    [n, C, H, W] tensors of one dtype and device (left in 0..1) -> [n, C, H, W]; differentiable."""
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
    return torch.sum(torch.mul(up.unsqueeze(2), stack), dim=1)


def term_counts(length_out: int, scale: int, length_in: int) -> int:
    """The largest number of terms one cell of an axis receives, from the tap table."""
    i0, i1, _, _ = ref.taps(length_out, scale, length_in)
    return int((np.bincount(i0, minlength=length_in) + np.bincount(i1, minlength=length_in)).max())


def error_factor(C: int, h: int, w: int, scale: int) -> int:
    """k of the bound k * 2^-24 * A: C roundings in G (C products, C - 1 sums, at most C deep), one product and one sum
    per term of each walk (a running sum of t terms: t + 1 roundings on its first term), and the two weights' own
    roundings for non-dyadic scales."""
    return C + term_counts(h * scale, scale, h) + term_counts(w * scale, scale, w) + 2


def gradient_noise(rng, n, C, H, W) -> np.ndarray:
    """What an L1 loss sends back, with some spread: signs over the pixel count, times a log-uniform factor."""
    sign = np.where(rng.random((n, C, H, W)) < 0.5, -1.0, 1.0)
    return (sign * np.exp(rng.uniform(-3.0, 0.0, (n, C, H, W))) / (n * C * H * W)).astype(F)
