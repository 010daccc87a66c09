"""The synthesis head's training form and backward without a GPU: the NumPy twin (tests/synthesis_grad_ref.py) against
the existing forward twin, against its own float64 evaluation within the derived bound and against torch's autograd of
the reference expression; the two C entries' declarations and refusals; the Python surface."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import synthesis_grad_ref as gref                    # noqa: E402
import synthesis_ref as ref                          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, ERR_HIP = -1, -3
F = np.float32


def operands(shape, u8=False):
    n, C_, D, h, w, S = shape
    rng = np.random.default_rng(D * 1000 + h * 100 + w + S)
    prob = ref.softmax_noise(rng, n, D, h, w)
    if u8:
        left = rng.integers(0, 256, (n, C_, h * S, w * S)).astype(np.uint8)
    else:
        left = ref.uniform_left(rng, n, C_, h * S, w * S)
    return prob, left, gref.gradient_noise(rng, n, C_, h * S, w * S)


def bits(a):
    return a.view(np.uint32)


# ----------------------------------------------------------------------------- 1. the rule
def test_shape_list():
    assert gref.SHAPES[:len(ref.SHAPES)] == ref.SHAPES
    assert gref.SHAPES[len(ref.SHAPES):] == [(1, 3, 7, 1, 1, 4), (2, 1, 9, 3, 1, 2), (1, 3, 7, 1, 3, 5), (1, 3, 9, 37, 45, 2),
                                             (1, 1, 5, 70, 70, 1)]


@pytest.mark.parametrize("shape", gref.SHAPES)
def test_rescaled_training_form_is_the_existing_twin(shape):
    prob, left, _ = operands(shape)
    view = gref.head_forward(prob, left, shape[5])
    assert view.dtype == F and view.shape == left.shape
    assert np.array_equal(bits(ref.rescale(view)), bits(ref.synthesize_right_view(prob, left, shape[5])))


@pytest.mark.parametrize("shape", gref.SHAPES)
def test_float32_twin_within_the_derived_bound_of_its_float64_evaluation(shape):
    n, C_, D, h, w, S = shape
    _, left, g = operands(shape)
    got = gref.head_backward(g, left, D, S)
    exact = gref.head_backward(g, left, D, S, dtype=np.float64)
    A = gref.head_backward(g, left, D, S, dtype=np.float64, absolute=True)
    k = gref.error_factor(C_, h, w, S)
    assert got.dtype == F and got.shape == (n, D, h, w)
    err = np.abs(got.astype(np.float64) - exact)
    bound = k * 2.0 ** -24 * A
    used = float(np.max(err[A > 0] / bound[A > 0])) if np.any(A > 0) else 0.0
    print(f"{shape}: k = {k}, max err / bound = {used:.3f}")
    assert np.all(err <= bound)
    if w * S < D:                                         # the planes d >= W are +0.0
        assert not bits(got[:, w * S:]).any()


@pytest.mark.parametrize("shape", gref.SHAPES)
def test_float64_evaluation_is_autograd_of_the_reference_expression(shape):
    n, C_, D, h, w, S = shape
    _, left, g = operands(shape)
    exact = gref.head_backward(g, left, D, S, dtype=np.float64)
    A = gref.head_backward(g, left, D, S, dtype=np.float64, absolute=True)
    rng = np.random.default_rng(1)
    prob = torch.from_numpy(rng.random((n, D, h, w))).requires_grad_()                   # the gradient does not depend on it
    view = gref.torch_view_expression(prob, torch.from_numpy(left.astype(np.float64)), S)
    view.backward(torch.from_numpy(g.astype(np.float64)))
    auto = prob.grad.numpy()
    err = np.abs(exact - auto)
    if S & (S - 1) == 0:
        assert float(err.max()) <= 1e-12, float(err.max())
    else:
        assert np.all(err <= 2.0 ** -23 * A), float((err / np.maximum(A, 1e-300)).max())


@pytest.mark.parametrize("shape", [(2, 3, 65, 7, 40, 4), (1, 3, 17, 4, 23, 3), (1, 3, 5, 9, 70, 1)])
def test_the_view_expression_is_the_reference_expression_without_its_rescale(shape):
    prob, left, _ = operands(shape)
    prob, left = torch.from_numpy(prob), torch.from_numpy(left)
    view = gref.torch_view_expression(prob, left, shape[5])
    assert torch.equal(torch.clamp(view * 255 + 0.5, 0, 255), ref.torch_expression(prob, left, shape[5]))


def test_a_nan_gradient_reaches_the_four_cells_of_its_pixel():
    shape = (1, 3, 9, 3, 5, 4)
    n, C_, D, h, w, S = shape
    _, left, g = operands(shape)
    g[0, :, 2, :7] = 0.0
    g[0, 1, 5, 3:9] = F(1e-42)
    g[0, 2, 7, 11] = np.nan
    got = gref.head_backward(g, left, D, S)
    # row 7: u = 11, taps 1 and 2; column 11: u = 19, taps 2 and 3; 11 + d < 20 for every plane
    want = np.zeros((n, D, h, w), bool)
    want[:, :, 1:3, 2:4] = True
    assert np.array_equal(np.isnan(got), want)


# ----------------------------------------------------------------------------- 2. the C entries
@pytest.fixture(scope="module")
def native():
    from cuda_depth import _native
    return _native


ENTRIES = {"smx_synthesis_head_forward": ("prob", "view"), "smx_synthesis_head_backward": ("grad_view", "grad_prob")}


@pytest.mark.parametrize("name", ENTRIES)
def test_symbols_are_declared_listed_exported_and_mirrored(native, name):
    text = open(os.path.join(ROOT, "include", "stereo_mi355x.h")).read()
    first, last = ENTRIES[name]
    assert name in text.split("Conventions")[0], "missing from the header's list of entry points"
    decl = re.search(r"\bint " + name + r"\((.*?)\);", text, flags=re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert params == ["int device_id", "int n", "int channels", "int dtype", "int D", "int h", "int w", "int scale",
                      f"const float *{first}", "const void *left", f"float *{last}", "void *stream"]
    assert re.search(r"\bT " + name + r"\b", os.popen(f"nm -D --defined-only {native.LIB_PATH}").read())
    restype, argtypes = native.EXPORTS[name]
    assert restype is C.c_int and argtypes == [C.c_int] * 8 + [C.c_void_p] * 4
    fn = getattr(native.LIB, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == argtypes
    assert native.LIB.smx_abi_version() == native.SMX_ABI_VERSION == 4


P, L, O = 0x10000000, 0x20000000, 0x30000000             # invented device addresses, far apart


def good(name):
    first, last = ENTRIES[name]                           # the input at P, the output at O
    return dict(device_id=0, n=2, channels=3, dtype=1, D=65, h=5, w=9, scale=4, **{first: P}, left=L, **{last: O}, stream=None)


def call(native, name, **changes):
    a = dict(good(name), **changes)
    rc = getattr(native.LIB, name)(*a.values())
    return rc, native.last_error()


def byte_sizes(a):
    px = a["h"] * a["scale"] * a["w"] * a["scale"]
    volume = a["n"] * a["D"] * a["h"] * a["w"] * 4
    left = a["n"] * a["channels"] * px * (4 if a["dtype"] == 1 else 1)
    return volume, left, a["n"] * a["channels"] * px * 4


REFUSALS = [
    (dict(left=None), "must be non-NULL"),
    (dict(n=0), "need n >= 1, got 0"),
    (dict(n=-3), "need n >= 1, got -3"),
    (dict(channels=2), "channels must be 1 or 3, got 2"),
    (dict(channels=4), "channels must be 1 or 3, got 4"),
    (dict(dtype=2), "unknown dtype 2"),
    (dict(dtype=-1), "unknown dtype -1"),
    (dict(D=0), "D must be in 1..256, got 0"),
    (dict(D=257), "D must be in 1..256, got 257"),
    (dict(scale=0), "scale must be in 1..16, got 0"),
    (dict(scale=17), "scale must be in 1..16, got 17"),
    (dict(h=0), "need h, w >= 1 and h * scale, w * scale <= 32768"),
    (dict(w=0), "need h, w >= 1 and h * scale, w * scale <= 32768"),
    (dict(h=8193), "need h, w >= 1 and h * scale, w * scale <= 32768"),
    (dict(w=8193), "need h, w >= 1 and h * scale, w * scale <= 32768"),
    (dict(scale=16, w=2049), "need h, w >= 1 and h * scale, w * scale <= 32768"),
    (dict(stream=-1), "needs a caller stream"),
]


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("changes,text", REFUSALS)
def test_refusals_before_the_device_is_touched(native, name, changes, text):
    if "stream" in changes:
        changes = dict(changes, stream=native.STREAM_ENGINE)
    rc, msg = call(native, name, **changes)
    assert rc == INVALID_ARG and msg.startswith(name) and text in msg, (rc, msg)


@pytest.mark.parametrize("name", ENTRIES)
def test_null_operands_and_the_order_of_the_rules(native, name):
    first, last = ENTRIES[name]
    for operand in (first, "left", last):
        rc, msg = call(native, name, **{operand: None})
        assert rc == INVALID_ARG and msg.startswith(name) and f"{first}, left and {last} must be non-NULL" in msg, (rc, msg)
    # the earlier rule answers a doubly wrong call: synthesize_right_view's order
    order = [({first: None}, "non-NULL"), (dict(n=0), "n >= 1"), (dict(channels=2), "channels"), (dict(dtype=7), "dtype"),
             (dict(D=0), "D must"), (dict(scale=0), "scale must"), (dict(h=0), "need h, w"), ({last: L}, "overlap"),
             (dict(stream=native.STREAM_ENGINE), "caller stream")]
    for (early, word), (late, _) in zip(order, order[1:]):
        rc, msg = call(native, name, **early, **late)
        assert rc == INVALID_ARG and word in msg, (early, late, msg)


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("dtype", [0, 1])
def test_an_output_must_not_overlap_an_input(native, name, dtype):
    first, last = ENTRIES[name]
    a = dict(good(name), dtype=dtype)
    volume, left_bytes, image = byte_sizes(a)
    in_bytes, out_bytes = (volume, image) if name.endswith("forward") else (image, volume)
    es = 4 if dtype == 1 else 1
    overlapping = [P, P + in_bytes - 4, P - out_bytes + 4, P + 400,
                   L, L + left_bytes - es, L - out_bytes + es, L + 40]
    for out in overlapping:
        rc, msg = call(native, name, dtype=dtype, **{last: out})
        assert rc == INVALID_ARG and f"{last} must not overlap {first} or left" in msg, (hex(out), rc, msg)


@pytest.mark.parametrize("name", ENTRIES)
def test_adjacent_operands_and_a_valid_call_reach_the_device(native, name):
    if torch.cuda.is_available():
        pytest.skip("GPU present: an accepted call would launch on invented addresses")
    first, last = ENTRIES[name]
    volume, left_bytes, image = byte_sizes(good(name))
    in_bytes, out_bytes = (volume, image) if name.endswith("forward") else (image, volume)
    for changes in (dict(), {last: P + in_bytes}, {last: P - out_bytes}, {last: L + left_bytes}, {last: L - out_bytes},
                    dict(left=P)):                        # left = the other input: the inputs may alias each other
        rc, msg = call(native, name, **changes)
        assert rc == ERR_HIP and "cannot select HIP device 0" in msg, (changes, rc, msg)


# ----------------------------------------------------------------------------- 3. the Python surface
def test_signatures():
    import cuda_depth
    import pipeline.synthesis as synthesis
    sig = inspect.signature(cuda_depth.synthesis_head)
    assert [(n, p.default) for n, p in sig.parameters.items()] == [("probabilities", inspect.Parameter.empty),
                                                                   ("left", inspect.Parameter.empty), ("scale", 4)]
    sig = inspect.signature(cuda_depth.synthesis_head_backward)
    assert [(n, p.default) for n, p in sig.parameters.items()] == [
        ("grad_view", inspect.Parameter.empty), ("left", inspect.Parameter.empty), ("D", inspect.Parameter.empty),
        ("scale", 4), ("out", None)]
    layer = synthesis.SelectionLayer()
    assert isinstance(layer, torch.nn.Module) and layer.scale == 4 and synthesis.SelectionLayer(scale=2).scale == 2
    assert list(inspect.signature(synthesis.SelectionLayer.forward).parameters) == ["self", "probabilities", "left_full"]
    assert "low-resolution" in synthesis.SelectionLayer.__doc__ and "SelectionLayer" in synthesis.__all__
    assert not list(layer.parameters())
    assert "differentiable head" in synthesis.__doc__
    for exc, scale in ((TypeError, 2.0), (TypeError, True), (ValueError, 0), (ValueError, 17)):
        with pytest.raises(exc, match="scale"):
            synthesis.SelectionLayer(scale=scale)


def test_head_checks_that_return_before_a_launch():
    import cuda_depth
    f = cuda_depth.synthesis_head
    prob, left = torch.zeros((2, 5, 3, 4)), torch.zeros((2, 3, 12, 16))
    with pytest.raises(TypeError, match="probabilities must be a torch.Tensor"):
        f(prob.numpy(), left)
    with pytest.raises(TypeError, match="probabilities must be float32"):
        f(prob.double(), left)
    with pytest.raises(TypeError, match="probabilities must be float32"):
        f(prob.to(torch.int32), left)
    with pytest.raises(TypeError, match="left must be uint8 or float32"):
        f(prob, left.to(torch.int32))
    with pytest.raises(TypeError, match="scale must be an int"):
        f(prob, left, scale=4.0)
    with pytest.raises(ValueError, match="scale must be in 1..16"):
        f(prob, left, scale=0)
    with pytest.raises(ValueError, match="left gets no gradient"):
        f(prob, left.clone().requires_grad_())
    with pytest.raises(ValueError, match="left must be 2 frames of 12 x 16"):
        f(prob, torch.zeros((2, 3, 12, 20)))
    with pytest.raises(ValueError, match="left must be 2 frames of 12 x 16"):
        f(prob, torch.zeros((3, 3, 12, 16)))
    with pytest.raises(ValueError, match="1 or 3 channels"):
        f(prob, torch.zeros((2, 2, 12, 16)))
    with pytest.raises(ValueError, match="1..256 disparity planes"):
        f(torch.zeros((2, 257, 3, 4)), left)
    with pytest.raises(ValueError, match=r"left must be \[n, C, H, W\]"):
        f(prob, left[0])
    with pytest.raises(ValueError, match="left must be contiguous"):
        f(prob, torch.zeros((2, 3, 16, 12)).transpose(2, 3))
    with pytest.raises(ValueError, match="must live on one GPU"):
        f(prob.requires_grad_(), left)


def test_backward_checks_that_return_before_a_launch():
    import cuda_depth
    f = cuda_depth.synthesis_head_backward
    g, left = torch.zeros((2, 3, 12, 16)), torch.zeros((2, 3, 12, 16))
    with pytest.raises(TypeError, match="grad_view must be a torch.Tensor"):
        f(g.numpy(), left, 5)
    with pytest.raises(TypeError, match="grad_view must be float32"):
        f(g.double(), left, 5)
    with pytest.raises(TypeError, match="left must be uint8 or float32"):
        f(g, left.half(), 5)
    with pytest.raises(TypeError, match="out must be float32"):
        f(g, left, 5, out=torch.zeros((2, 5, 3, 4), dtype=torch.float64))
    with pytest.raises(TypeError, match="D must be an int"):
        f(g, left, 5.0)
    with pytest.raises(TypeError, match="scale must be an int"):
        f(g, left, 5, scale=True)
    with pytest.raises(ValueError, match="D must be in 1..256"):
        f(g, left, 0)
    with pytest.raises(ValueError, match="scale must be in 1..16"):
        f(g, left, 5, scale=17)
    with pytest.raises(ValueError, match="like grad_view"):
        f(g, left[:, :1], 5)
    with pytest.raises(ValueError, match="1 or 3 channels"):
        f(torch.zeros((2, 2, 12, 16)), torch.zeros((2, 2, 12, 16)), 5)
    with pytest.raises(ValueError, match="must divide"):
        f(g, left, 5, scale=5)
    with pytest.raises(ValueError, match=r"out must be \(2, 5, 3, 4\)"):
        f(g, left, 5, out=torch.zeros((2, 5, 3, 5)))
    with pytest.raises(ValueError, match="grad_view must be contiguous"):
        f(torch.zeros((2, 3, 16, 12)).transpose(2, 3), left, 5)
    with pytest.raises(ValueError, match="must live on one GPU"):
        f(g, left, 5)
