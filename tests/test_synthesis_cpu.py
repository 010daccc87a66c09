"""Right-view synthesis head without a GPU: the rule's NumPy twin (tests/synthesis_ref.py) against the torch expression
of what Deep3D computes and against known answers, the C entry's declaration and refusals, the Python wrapper's checks
that return before a launch, and the stand-in model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import synthesis_ref as ref                          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, ERR_HIP = -1, -3
F = np.float32


# ----------------------------------------------------------------------------- 1. the rule
@pytest.mark.parametrize("n,C_,D,h,w,S", [s for s in ref.SHAPES if s[5] in (1, 2, 4, 8)])
def test_twin_against_the_torch_expression(n, C_, D, h, w, S):
    rng = np.random.default_rng(D * 1000 + h * 100 + w + S)
    prob = ref.softmax_noise(rng, n, D, h, w)
    left = ref.uniform_left(rng, n, C_, h * S, w * S)
    twin = ref.synthesize_right_view(prob, left, S)
    expr = ref.torch_expression(torch.from_numpy(prob), torch.from_numpy(left), S).numpy()
    err = float(np.max(np.abs(twin.astype(np.float64) - expr.astype(np.float64))))
    print(f"(n {n}, C {C_}, D {D}, {h}x{w}, S {S}): max |twin - torch| = {err:.3g}, bound {ref.error_bound(D):.3g}")
    assert twin.dtype == F and twin.shape == left.shape
    assert err <= ref.error_bound(D)


@pytest.mark.parametrize("k", [0, 1, 4, 30])
def test_one_hot_plane_at_scale_1_shifts_the_frame(k):
    rng = np.random.default_rng(k)
    n, C_, D, H, W = 2, 3, 31, 6, 40
    prob = np.zeros((n, D, H, W), F)
    prob[:, k] = 1.0
    left = ref.uniform_left(rng, n, C_, H, W)
    got = ref.synthesize_right_view(prob, left, 1)
    want = np.full_like(left, 0.5)
    want[..., :W - k] = ref.rescale(left[..., k:])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_one_plane_is_the_rescale_alone():
    rng = np.random.default_rng(5)
    left = (rng.random((1, 3, 8, 12)) * 1.2 - 0.1).astype(F)            # also outside 0..1: the clamp
    for S in (1, 2, 4):
        prob = np.ones((1, 1, 8 // S, 12 // S), F)
        got = ref.synthesize_right_view(prob, left, S)
        assert np.array_equal(got.view(np.uint32), ref.rescale(left).view(np.uint32))
    assert ref.rescale(np.array([np.nan, -1.0, 2.0, 0.0], F)).tolist() == [0.0, 0.0, 255.0, 0.5]


def test_uint8_frames_are_the_float_frames_of_byte_over_255():
    rng = np.random.default_rng(6)
    n, C_, D, h, w, S = 1, 3, 20, 3, 11, 4
    prob = ref.softmax_noise(rng, n, D, h, w)
    left8 = rng.integers(0, 256, (n, C_, h * S, w * S)).astype(np.uint8)
    leftf = left8.astype(F) / F(255.0)
    assert leftf.dtype == F
    a, b = ref.synthesize_right_view(prob, left8, S), ref.synthesize_right_view(prob, leftf, S)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ----------------------------------------------------------------------------- 2. the C entry
@pytest.fixture(scope="module")
def native():
    from cuda_depth import _native
    return _native


def test_symbol_is_declared_listed_and_exported(native):
    header = open(os.path.join(ROOT, "include", "stereo_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+smx_synthesize_right_view\s*\(int device_id, int n, int channels, int dtype, int D, "
                     r"int h, int w, int scale,\s*const float \*prob, const void \*left, float \*out, void \*stream\);",
                     header)
    assert len(native.EXPORTS["smx_synthesize_right_view"][1]) == 12
    assert hasattr(C.CDLL(native.LIB_PATH), "smx_synthesize_right_view")
    assert native.LIB.smx_abi_version() == native.SMX_ABI_VERSION == 4


P, L, O = 0x10000000, 0x20000000, 0x30000000             # invented device addresses, far apart
GOOD = dict(device_id=0, n=2, channels=3, dtype=1, D=65, h=5, w=9, scale=4, prob=P, left=L, out=O, stream=None)


def call(native, **changes):
    a = dict(GOOD, **changes)
    rc = native.LIB.smx_synthesize_right_view(a["device_id"], a["n"], a["channels"], a["dtype"], a["D"], a["h"], a["w"],
                                              a["scale"], a["prob"], a["left"], a["out"], a["stream"])
    return rc, native.last_error()


def sizes(a):
    px = a["h"] * a["scale"] * a["w"] * a["scale"]
    prob = a["n"] * a["D"] * a["h"] * a["w"] * 4
    left = a["n"] * a["channels"] * px * (4 if a["dtype"] == 1 else 1)
    return prob, left, a["n"] * a["channels"] * px * 4


REFUSALS = [
    (dict(prob=None), "prob, left and out must be non-NULL"),
    (dict(left=None), "prob, left and out must be non-NULL"),
    (dict(out=None), "prob, left and out must be non-NULL"),
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


@pytest.mark.parametrize("changes,text", REFUSALS)
def test_refusals_before_the_device_is_touched(native, changes, text):
    if "stream" in changes:
        changes = dict(changes, stream=native.STREAM_ENGINE)
    rc, msg = call(native, **changes)
    assert rc == INVALID_ARG and msg.startswith("smx_synthesize_right_view") and text in msg, (rc, msg)


@pytest.mark.parametrize("dtype", [0, 1])
def test_out_must_not_overlap_an_input(native, dtype):
    a = dict(GOOD, dtype=dtype)
    prob_bytes, left_bytes, out_bytes = sizes(a)
    es = 4 if dtype == 1 else 1
    overlapping = [P, P + prob_bytes - 4, P - out_bytes + 4, P + 400,            # prob: same start, one element at each end, inside
                   L, L + left_bytes - es, L - out_bytes + es, L + 40]           # left: the same
    for out in overlapping:
        rc, msg = call(native, dtype=dtype, out=out)
        assert rc == INVALID_ARG and "out must not overlap prob or left" in msg, (hex(out), rc, msg)


def test_adjacent_operands_and_a_valid_call_reach_the_device(native):
    if torch.cuda.is_available():
        pytest.skip("GPU present: an accepted call would launch on invented addresses")
    prob_bytes, left_bytes, out_bytes = sizes(GOOD)
    for changes in (dict(), dict(out=P + prob_bytes), dict(out=P - out_bytes), dict(out=L + left_bytes),
                    dict(out=L - out_bytes), dict(left=P),             # left = prob: the inputs may alias each other
                    dict(dtype=0, channels=1, D=256, scale=16, h=2048, w=2048, n=1,
                                                                out=0x7000000000)):
        rc, msg = call(native, **changes)
        assert rc == ERR_HIP and "cannot select HIP device 0" in msg, (changes, rc, msg)


# ----------------------------------------------------------------------------- 3. the Python wrapper
def test_wrapper_checks_that_return_before_a_launch():
    import cuda_depth
    f = cuda_depth.synthesize_right_view
    prob, left = torch.zeros((2, 5, 3, 4)), torch.zeros((2, 3, 12, 16))
    with pytest.raises(TypeError, match="probabilities must be float32"):
        f(prob.double(), left)
    with pytest.raises(TypeError, match="left must be uint8 or float32"):
        f(prob, left.to(torch.int32))
    with pytest.raises(TypeError, match="out must be float32"):
        f(prob, left, out=left.double())
    with pytest.raises(TypeError, match="scale must be an int"):
        f(prob, left, scale=4.0)
    with pytest.raises(TypeError, match="must be a torch.Tensor"):
        f(prob.numpy(), left)
    with pytest.raises(ValueError, match="scale must be in 1..16"):
        f(prob, left, scale=17)
    with pytest.raises(ValueError, match="probabilities must be a non-empty"):
        f(prob[0, 0], left)
    with pytest.raises(ValueError, match=r"left must be \[n, C, H, W\]"):
        f(prob, left[0])
    with pytest.raises(ValueError, match=r"left must be \[C, H, W\] or \[H, W\]"):
        f(prob[0], left)
    with pytest.raises(ValueError, match="1 or 3 channels"):
        f(prob, torch.zeros((2, 2, 12, 16)))
    with pytest.raises(ValueError, match="1..256 disparity planes"):
        f(torch.zeros((2, 257, 3, 4)), left)
    with pytest.raises(ValueError, match="12 x 16"):
        f(prob, torch.zeros((2, 3, 12, 15)))
    with pytest.raises(ValueError, match="2 frames of 12 x 16"):
        f(prob, torch.zeros((3, 3, 12, 16)))
    with pytest.raises(ValueError, match="out must be"):
        f(prob, left, out=torch.zeros((2, 3, 12, 17)))
    with pytest.raises(ValueError, match="left must be contiguous"):
        f(prob, torch.zeros((2, 3, 16, 12)).transpose(2, 3))
    with pytest.raises(ValueError, match="must live on one GPU"):
        f(prob, left)                                                    # CPU tensors


def test_synthesis_module_and_pipeline_keyword():
    import inspect
    from pipeline import DepthEstimationPipeline
    from pipeline.synthesis import DisparityOracleModel, RightViewSynthesis
    sig = inspect.signature(RightViewSynthesis.__init__)
    got = [(n, p.default, p.kind == p.KEYWORD_ONLY) for n, p in sig.parameters.items() if n not in ("self", "model")]
    assert got == [("full_resolution", (384, 1280), True), ("scale", 4, True), ("model_output", "probabilities", True),
                   ("downscale", None, True)]
    p = inspect.signature(DepthEstimationPipeline.__init__).parameters["right_view_synthesis"]
    assert p.default is None and p.kind == p.KEYWORD_ONLY
    model = DisparityOracleModel(torch.zeros((2, 2)), 4)
    with pytest.raises(ValueError, match="multiple of scale"):
        RightViewSynthesis(model, full_resolution=(10, 16))
    with pytest.raises(ValueError, match="model_output"):
        RightViewSynthesis(model, model_output="logits")
    with pytest.raises(ValueError, match=r"left_view must be \[3, 8, 16\]"):
        RightViewSynthesis(model, full_resolution=(8, 16)).process(torch.zeros((3, 8, 12)))


def test_oracle_model_planes_are_a_partition_of_one():
    from pipeline.synthesis import DisparityOracleModel
    rng = np.random.default_rng(8)
    D = 33
    disp = torch.from_numpy((rng.random((7, 9)) * (D + 6) - 3).astype(F))      # also outside 0 .. D-1
    disp[0, 0], disp[0, 1], disp[0, 2] = 0.0, float(D - 1), 4.0
    planes = DisparityOracleModel(disp, D)(torch.zeros((1, 3, 28, 36)), torch.zeros((1, 3, 7, 9)))
    assert tuple(planes.shape) == (1, D, 7, 9) and planes.dtype == torch.float32
    assert float(planes.min()) >= 0.0
    assert float((planes.sum(dim=1) - 1.0).abs().max()) <= 2.0 ** -22
    assert planes[0, :, 0, 2].tolist() == [1.0 if d == 4 else 0.0 for d in range(D)]
    mean = (planes[0] * torch.arange(D, dtype=torch.float32).view(D, 1, 1)).sum(0)
    assert float((mean - disp.clamp(0, D - 1)).abs().max()) <= 1e-5
