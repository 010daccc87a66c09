"""The synthesis head's training form and backward on the device (include/stereo_mi355x.h: smx_synthesis_head_forward,
smx_synthesis_head_backward), the autograd function over them and SelectionLayer in a small training loop.

Both rules fix every operation and the order of every sum, so the expected views and gradients come from the NumPy twin
(tests/synthesis_grad_ref.py) and are compared bit for bit, whatever the kernels' tiles, chunks and steps."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import synthesis_grad_ref as gref                    # noqa: E402
import synthesis_ref as ref                          # noqa: E402
from synthesis_device_cases import assert_bitwise, bits, case, dev     # noqa: E402

F = np.float32
IDS = dict(ids=lambda s: "n%d_C%d_D%d_%dx%d_S%d" % s)
PLUMBING = (2, 3, 65, 7, 40, 4)


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


# ----------------------------------------------------------------------------- 1. the kernels against the twin
@pytest.mark.parametrize("shape", gref.SHAPES, **IDS)
def test_shapes(cd, shape):
    n, C, D, h, w, S = shape
    prob, left, g, view, grad = case(shape)
    got = cd.synthesis_head(dev(prob), dev(left), scale=S)
    assert got.dtype == torch.float32 and not got.requires_grad
    assert_bitwise(got, view, f"view {shape}")
    got = cd.synthesis_head_backward(dev(g), dev(left), D, scale=S)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, D, h, w)
    assert_bitwise(got, grad, f"grad_prob {shape}")
    if w * S < D:
        assert not bits(got[:, w * S:]).any(), "the planes d >= W are +0.0"


@pytest.mark.parametrize("shape", gref.SHAPES[:2], **IDS)
def test_uint8_frames(cd, shape):
    prob, left, g, view, grad = case(shape, True)
    assert_bitwise(cd.synthesis_head(dev(prob), dev(left), scale=shape[5]), view, f"u8 view {shape}")
    assert_bitwise(cd.synthesis_head_backward(dev(g), dev(left), shape[2], scale=shape[5]), grad, f"u8 grad_prob {shape}")


def test_the_c_entries_and_unbatched_operands(cd):
    from cuda_depth import _native as N
    n, C, D, h, w, S = shape = gref.SHAPES[1]
    prob, left, g, view, grad = case(shape)
    tp, tl, tg = dev(prob), dev(left), dev(g)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.full(left.shape, float("nan"), device="cuda")
    N.check(N.LIB.smx_synthesis_head_forward(0, n, C, N.DTYPE_F32, D, h, w, S, tp.data_ptr(), tl.data_ptr(), out.data_ptr(),
                                             stream))
    assert_bitwise(out, view, "forward through ctypes")
    out = torch.full(prob.shape, float("nan"), device="cuda")
    N.check(N.LIB.smx_synthesis_head_backward(0, n, C, N.DTYPE_F32, D, h, w, S, tg.data_ptr(), tl.data_ptr(), out.data_ptr(),
                                              stream))
    assert_bitwise(out, grad, "backward through ctypes")
    # out=, and a call that is refused launches nothing
    again = torch.full(prob.shape, float("nan"), device="cuda")
    assert cd.synthesis_head_backward(tg, tl, D, scale=S, out=again) is again
    assert_bitwise(again, grad, "out=")
    with pytest.raises(RuntimeError, match="grad_prob must not overlap grad_view or left"):
        cd.synthesis_head_backward(tg, tl, 3, scale=S, out=tg.view(-1)[:n * 3 * h * w].view(n, 3, h, w))
    assert_bitwise(tg, g, "the refused call wrote nothing")
    assert_bitwise(cd.synthesis_head(tp[1], tl[1], scale=S), view[1], "[D,h,w] and [C,H,W]")
    got = cd.synthesis_head_backward(tg[1], tl[1], D, scale=S)
    assert tuple(got.shape) == (D, h, w)
    assert_bitwise(got, grad[1], "[C,H,W] gradient")
    gp, gl, gg, gview, ggrad = case(gref.SHAPES[2])
    assert_bitwise(cd.synthesis_head(dev(gp[0]), dev(gl[0, 0]), scale=2), gview[0, 0], "[H,W] view")
    assert_bitwise(cd.synthesis_head_backward(dev(gg[0, 0]), dev(gl[0, 0]), gp.shape[1], scale=2), ggrad[0], "[H,W] gradient")


def test_more_frames_than_the_grid_cap(cd):
    n = 66000
    rng = np.random.default_rng(3)
    prob = ref.softmax_noise(rng, n, 2, 1, 2)
    left = ref.uniform_left(rng, n, 1, 1, 2)
    g = gref.gradient_noise(rng, n, 1, 1, 2)
    assert_bitwise(cd.synthesis_head(dev(prob), dev(left), scale=1), gref.head_forward(prob, left, 1), "66000 views")
    assert_bitwise(cd.synthesis_head_backward(dev(g), dev(left), 2, scale=1), gref.head_backward(g, left, 2, 1),
                   "66000 gradients")


def test_zeros_denormals_and_a_nan_in_the_gradient(cd):
    n, C, D, h, w, S = shape = PLUMBING
    _, left, g, _, _ = case(shape)
    g = g.copy()
    g[:, :, ::3] = 0.0
    g[:, :, 1::6] = F(1e-40)
    g[1, 2, 13, 77] = np.nan
    assert 0 < float(g[0, 0, 1, 0]) < np.finfo(F).tiny
    want = gref.head_backward(g, left, D, S)
    nan = np.isnan(want)
    assert nan.any() and not nan[0].any() and nan.sum() == 4 * D       # row 13 and column 77 have two cells each
    got = cd.synthesis_head_backward(dev(g), dev(left), D, scale=S)
    assert np.array_equal(np.isnan(got.cpu().numpy()), nan)
    assert_bitwise(np.nan_to_num(got.cpu().numpy(), nan=7.0), np.nan_to_num(want, nan=7.0), "around the NaN")


# ----------------------------------------------------------------------------- 2. autograd
@functools.lru_cache(maxsize=None)
def plumbing_case():
    """Logits, the frame and a target well away from the view, so that no sign of the L1 gradient is a matter of the
    softmax's last bits."""
    n, C, D, h, w, S = PLUMBING
    rng = np.random.default_rng(17)
    logits = rng.normal(0.0, 1.0, (n, D, h, w)).astype(F)
    left = ref.uniform_left(rng, n, C, h * S, w * S)
    view = gref.head_forward(torch.softmax(torch.from_numpy(logits), dim=1).numpy(), left, S)
    sign = np.where(rng.random(view.shape) < 0.5, -1.0, 1.0)
    target = (view - sign * rng.uniform(0.05, 0.3, view.shape)).astype(F)
    for a in (logits, left, target, sign):
        a.setflags(write=False)
    return logits, left, target, sign


def test_loss_backward_leaves_the_chain_rules_gradient_on_the_logits(cd):
    n, C, D, h, w, S = PLUMBING
    logits, left, target, sign = plumbing_case()
    tl = dev(logits).requires_grad_()
    prob = torch.softmax(tl, dim=1)
    prob.retain_grad()
    view = cd.synthesis_head(prob, dev(left), scale=S)
    assert view.requires_grad
    view.retain_grad()
    loss = torch.nn.functional.l1_loss(view, dev(target))
    loss.backward()
    # what the loss sent back: sign(view - target) / N; the head's gradient of it is the twin's, bit for bit
    g = view.grad.cpu().numpy()
    assert np.array_equal(np.sign(g), sign) and np.allclose(np.abs(g), 1.0 / g.size, rtol=1e-6)
    grad_prob = gref.head_backward(g, left, D, S)
    assert_bitwise(prob.grad, grad_prob, "grad_prob under autograd")
    # torch's own chain from there, on the CPU: grad_i = p_i (g_i - sum_k p_k g_k).  D + 1 roundings in the sum, two more
    # operations, both sides round, and the device's p differs from the CPU's by a few ulp: (D + 12) 2^-24 a side
    cl = torch.tensor(logits).requires_grad_()
    torch.softmax(cl, dim=1).backward(torch.from_numpy(grad_prob))
    want = cl.grad.numpy()
    tol = 2.0 * (D + 12) * 2.0 ** -24 * float(np.abs(grad_prob).max())
    err = float(np.abs(tl.grad.cpu().numpy().astype(np.float64) - want).max())
    print(f"logits' gradient: max err {err:.3g}, tolerance {tol:.3g}, max |grad| {float(np.abs(want).max()):.3g}")
    assert err <= tol
    with pytest.raises(RuntimeError):
        loss.backward()                                   # the graph is freed


def test_the_backward_is_once_differentiable(cd):
    n, C, D, h, w, S = PLUMBING
    logits, left, target, _ = plumbing_case()
    prob = torch.softmax(dev(logits), dim=1).requires_grad_()
    loss = torch.nn.functional.l1_loss(cd.synthesis_head(prob, dev(left), scale=S), dev(target))
    (grad,) = torch.autograd.grad(loss, prob, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        grad.sum().backward()


def test_a_non_contiguous_gradient_gives_the_bits_of_its_contiguous_copy(cd):
    n, C, D, h, w, S = PLUMBING
    prob, left, g, _, grad = case(PLUMBING)
    strided = torch.empty((n, C, w * S, h * S), device="cuda").transpose(2, 3)
    strided.copy_(dev(g))
    assert not strided.is_contiguous()
    for incoming in (strided, strided.contiguous()):
        tp = dev(prob).requires_grad_()
        cd.synthesis_head(tp, dev(left), scale=S).backward(incoming)
        assert_bitwise(tp.grad, grad, "grad_prob")


def test_autocast_runs_the_head_in_float32(cd):
    n, C, D, h, w, S = PLUMBING
    prob, left, g, view, grad = case(PLUMBING)
    tp = dev(prob).requires_grad_()
    with torch.autocast("cuda", dtype=torch.float16):
        out = cd.synthesis_head(tp, dev(left), scale=S)
    assert out.dtype == torch.float32
    assert_bitwise(out, view, "view under autocast")
    out.backward(dev(g))
    assert_bitwise(tp.grad, grad, "grad_prob under autocast")


def test_against_autograd_of_the_reference_expression_on_the_device(cd):
    n, C, D, h, w, S = PLUMBING
    prob, left, g, _, _ = case(PLUMBING)
    tp = dev(prob).requires_grad_()
    gref.torch_view_expression(tp, dev(left), S).backward(dev(g))
    fused = cd.synthesis_head_backward(dev(g), dev(left), D, scale=S)
    A = gref.head_backward(g, left, D, S, dtype=np.float64, absolute=True)
    bound = 2.0 * gref.error_factor(C, h, w, S) * 2.0 ** -24 * A
    err = np.abs(fused.cpu().numpy().astype(np.float64) - tp.grad.cpu().numpy().astype(np.float64))
    print(f"fused against torch autograd: max err / bound = {float((err[A > 0] / bound[A > 0]).max()):.3f}")
    assert np.all(err <= bound)


# ----------------------------------------------------------------------------- 3. determinism, capture, memory
def test_two_calls_give_identical_bits(cd):
    prob, left, g, _, _ = case(PLUMBING)
    tp, tl, tg = dev(prob), dev(left), dev(g)
    a, b = cd.synthesis_head_backward(tg, tl, 65), cd.synthesis_head_backward(tg, tl, 65)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    a, b = cd.synthesis_head(tp, tl), cd.synthesis_head(tp, tl)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_forward_and_backward_replay_from_one_graph(cd):
    n, C, D, h, w, S = PLUMBING
    prob, left, g, view, grad = case(PLUMBING)
    tp, tl, tg = (torch.zeros(a.shape, device="cuda") for a in (prob, left, g))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # warm-up outside the capture
        cd.synthesis_head_backward(tg, tl, D, scale=S)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                         # one branch: forward, then backward
        out_view = cd.synthesis_head(tp, tl, scale=S)
        out_grad = cd.synthesis_head_backward(tg, tl, D, scale=S)
    tp.copy_(dev(prob)), tl.copy_(dev(left)), tg.copy_(dev(g))
    for _ in range(2):
        out_view.fill_(float("nan")), out_grad.fill_(float("nan"))
        graph.replay()
        assert_bitwise(out_view, view, "replayed view")
        assert_bitwise(out_grad, grad, "replayed grad_prob")


def test_peak_memory_stays_below_one_upsampled_volume(cd):
    n, C, D, h, w, S = 1, 3, 65, 24, 80, 4
    rng = np.random.default_rng(9)
    tp = dev(ref.softmax_noise(rng, n, D, h, w)).requires_grad_()
    tl = dev(ref.uniform_left(rng, n, C, h * S, w * S))
    tg = dev(gref.gradient_noise(rng, n, C, h * S, w * S))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    view = cd.synthesis_head(tp, tl, scale=S)
    view.backward(tg)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes; one upsampled volume {D * h * S * w * S * 4}")
    assert tp.grad is not None and rise < D * h * S * w * S * 4


# ----------------------------------------------------------------------------- 4. a tiny training loop
def train(layer, left, target, steps=20):
    torch.manual_seed(5)
    logits = (torch.randn((1, 9, 6, 20)) * 0.1).to("cuda").requires_grad_()
    optimiser = torch.optim.Adam([logits], lr=0.1)
    losses = []
    for _ in range(steps):
        optimiser.zero_grad()
        loss = torch.nn.functional.l1_loss(layer(torch.softmax(logits, dim=1), left), target)
        loss.backward()
        optimiser.step()
        losses.append(loss.item())
    return losses


def test_selection_layer_trains_like_the_torch_expression(cd):
    from pipeline.synthesis import DisparityOracleModel, SelectionLayer
    n, C, D, h, w, S = 1, 3, 9, 6, 20, 4
    rng = np.random.default_rng(23)
    left = dev(ref.uniform_left(rng, n, C, h * S, w * S))
    disparity = torch.from_numpy(rng.uniform(0.0, D - 1.0, (h, w)).astype(F))
    volume = DisparityOracleModel(disparity, D)(left, None)
    target = cd.synthesis_head(volume, left, scale=S)
    fused = train(SelectionLayer(scale=S), left, target)
    plain = train(lambda prob, frame: gref.torch_view_expression(prob, frame, S), left, target)
    print("fused", " ".join(f"{v:.6f}" for v in fused))
    print("torch", " ".join(f"{v:.6f}" for v in plain))
    print("largest relative difference", max(abs(a - b) / b for a, b in zip(fused, plain)))
    assert all(b < a for a, b in zip(fused, fused[1:])) and all(b < a for a, b in zip(plain, plain[1:]))
    assert fused[-1] < 0.5 * fused[0]
    assert all(abs(a - b) <= 1e-4 * b for a, b in zip(fused, plain))
