"""What the synthesis head's device tests share (tests/test_synthesis_grad_gpu.py, tests/test_synthesis_paths_gpu.py): the
bit-for-bit comparison and the inputs and twin results of a shape, computed once per process and left unchanged."""
import functools

import numpy as np
import torch

import synthesis_grad_ref as gref
import synthesis_ref as ref

F = np.float32


def bits(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def dev(a) -> "torch.Tensor":
    """A device copy (the cached arrays of case() are read-only)."""
    return torch.tensor(a, device="cuda")


def assert_bitwise(got, expect, what):
    g, e = bits(got), bits(expect)
    assert g.shape == e.shape, f"{what}: shape {g.shape} != {e.shape}"
    bad = np.argwhere(g != e)
    assert bad.size == 0, f"{what}: {len(bad)} of {g.size} values differ, first at {tuple(bad[0])}"


@functools.lru_cache(maxsize=None)
def case(shape, u8=False):
    """(prob, left, grad_view, expected view, expected grad_prob) of a shape, computed once and left unchanged."""
    n, C, D, h, w, S = shape
    rng = np.random.default_rng(sum(v * 31 ** i for i, v in enumerate(shape)))
    prob = ref.softmax_noise(rng, n, D, h, w)
    left = rng.integers(0, 256, (n, C, h * S, w * S)).astype(np.uint8) if u8 else ref.uniform_left(rng, n, C, h * S, w * S)
    g = gref.gradient_noise(rng, n, C, h * S, w * S)
    out = prob, left, g, gref.head_forward(prob, left, S), gref.head_backward(g, left, D, S)
    for a in out:
        a.setflags(write=False)
    return out
