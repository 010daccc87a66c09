"""Synthetic stereo video sequences for the temporal filter, built on stereo_synthetic.make_slanted_pair's scene
(multi-scale texture, a ground ramp, two objects, occlusion-free cyclic warp).  Each frame is (left, right, truth):
integer-valued float32 [H, W] gray views and the ground-truth disparity.

    static_sequence: a static camera; every frame has fresh seeded +-2 sensor noise on both views.
    moving_sequence: the same scene with a textured rectangle at its own disparity moving `step` px right per frame."""
from __future__ import annotations

import numpy as np

import stereo_synthetic as syn


def _warp(left: np.ndarray, truth: np.ndarray) -> np.ndarray:
    """The right view of make_slanted_pair's construction: right[x, y] = left[x, (y + truth[x, y]) % W]."""
    W = left.shape[1]
    cols = (np.arange(W)[None, :] + truth.astype(np.int64)) % W
    return np.take_along_axis(left, cols, axis=1)


def _noisy(img: np.ndarray, rng: np.random.Generator) -> np.ndarray:
    return np.clip(img + rng.integers(-2, 3, img.shape), 0, 255).astype(np.float32)


def static_sequence(frames: int, H: int, W: int, D: int, K: int, index: int = 0, seed: int = 0):
    """`frames` (left, right, truth) of one scene seen by a static camera, with fresh +-2 noise per frame."""
    left, _, truth = syn.make_slanted_pair(H, W, D, K, index)
    right = _warp(left, truth)
    rng = np.random.default_rng(seed)
    return [(_noisy(left, rng), _noisy(right, rng), truth) for _ in range(frames)]


def moving_sequence(frames: int, H: int, W: int, D: int, K: int, index: int = 0, seed: int = 0, step: int = 3):
    """As static_sequence, with an object (rows H/8 .. 3H/8, W/8 wide, its own coarse texture, disparity 0.7 (D - 1))
    whose left edge starts at W/2 and moves `step` px right per frame."""
    left0, _, truth0 = syn.make_slanted_pair(H, W, D, K, index)
    rng = np.random.default_rng(seed)
    r0, r1, w = H // 8, (3 * H) // 8, max(W // 8, 1)
    patch = np.kron(rng.integers(0, 256, ((r1 - r0 + 3) // 4, (w + 3) // 4)), np.ones((4, 4)))[:r1 - r0, :w]
    d_obj = np.float32(int((D - 1) * 0.7))
    seq = []
    for f in range(frames):
        c0 = min(W // 2 + f * step, W - w)
        left, truth = left0.copy(), truth0.copy()
        left[r0:r1, c0:c0 + w] = patch
        truth[r0:r1, c0:c0 + w] = d_obj
        seq.append((_noisy(left, rng), _noisy(_warp(left, truth), rng), truth))
    return seq
