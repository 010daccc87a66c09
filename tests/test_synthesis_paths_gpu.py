"""The synthesis head's kernels on the device at every instantiation and path (tests/synthesis_paths.py: CASES; what each
case reaches is proved on the CPU by tests/test_synthesis_paths_cpu.py): the training form, the backward and the rescaled
view against their NumPy twins, bit for bit."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import synthesis_paths as sp                         # noqa: E402
import synthesis_ref as ref                          # noqa: E402
from synthesis_device_cases import assert_bitwise, bits, case, dev     # noqa: E402


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


@pytest.mark.parametrize("c", sp.CASES, ids=sp.case_id)
def test_case(cd, c):
    n, C, dtype, D, h, w, S = c
    prob, left, g, view, grad = case((n, C, D, h, w, S), dtype == "u8")
    assert str(left.dtype) == {"f32": "float32", "u8": "uint8"}[dtype]
    tp, tl, tg = dev(prob), dev(left), dev(g)
    got = cd.synthesis_head(tp, tl, scale=S)
    assert got.dtype == torch.float32
    assert_bitwise(got, view, f"view {tuple(c)}")
    got = cd.synthesis_head_backward(tg, tl, D, scale=S)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, D, h, w)
    assert_bitwise(got, grad, f"grad_prob {tuple(c)}")
    if w * S < D:
        assert not bits(got[:, w * S:]).any(), "the planes d >= W are +0.0"
    got = cd.synthesize_right_view(tp, tl, scale=S)
    assert_bitwise(got, ref.synthesize_right_view(prob, left, S), f"rescaled view {tuple(c)}")
