"""Right-view synthesis head on the device (include/stereo_mi355x.h: smx_synthesize_right_view) and in the pipeline.

The rule is a fixed sequence of float32 operations with the order of the sum over d fixed, so every expected view comes
from the NumPy twin (tests/synthesis_ref.py) and is compared bit for bit, whatever the kernel's tiles and chunks."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stereo_synthetic as syn                       # noqa: E402
import synthesis_ref as ref                          # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def bits(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def dev(a) -> "torch.Tensor":
    """A device copy (the cached arrays of case() are read-only)."""
    return torch.tensor(a, device="cuda")


def assert_bitwise(got, expect, what):
    g, e = bits(got), bits(expect)
    assert g.shape == e.shape, f"{what}: shape {g.shape} != {e.shape}"
    bad = np.argwhere(g != e)
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first at {tuple(bad[0])}"


@functools.lru_cache(maxsize=None)
def case(shape, u8=False):
    """(prob, left, expected view) of a shape, computed once: softmax noise, a uniform frame."""
    n, C, D, h, w, S = shape
    rng = np.random.default_rng(sum(v * 31 ** i for i, v in enumerate(shape)))
    prob = ref.softmax_noise(rng, n, D, h, w)
    left = rng.integers(0, 256, (n, C, h * S, w * S)).astype(np.uint8) if u8 else ref.uniform_left(rng, n, C, h * S, w * S)
    for a in (prob, left):
        a.setflags(write=False)
    return prob, left, ref.synthesize_right_view(prob, left, S)


# ----------------------------------------------------------------------------- 1. the kernel against the twin
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "n%d_C%d_D%d_%dx%d_S%d" % s)
def test_shapes(cd, shape):
    prob, left, want = case(shape)
    got = cd.synthesize_right_view(dev(prob), dev(left), scale=shape[5])
    assert got.dtype == torch.float32
    assert_bitwise(got, want, str(shape))


@pytest.mark.parametrize("shape", ref.SHAPES[:2], ids=lambda s: "n%d_C%d_D%d_%dx%d_S%d" % s)
def test_uint8_frames(cd, shape):
    prob, left, want = case(shape, True)
    got = cd.synthesize_right_view(dev(prob), dev(left), scale=shape[5])
    assert_bitwise(got, want, f"u8 {shape}")


def test_unbatched_operands_and_the_c_entry(cd):
    from cuda_depth import _native as N
    shape = ref.SHAPES[1]
    n, C, D, h, w, S = shape
    prob, left, want = case(shape)
    tp, tl = dev(prob), dev(left)
    out = torch.full(left.shape, float("nan"), device="cuda")
    N.check(N.LIB.smx_synthesize_right_view(0, n, C, N.DTYPE_F32, D, h, w, S, tp.data_ptr(), tl.data_ptr(), out.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream))
    assert_bitwise(out, want, "through ctypes")
    assert_bitwise(cd.synthesize_right_view(tp[1], tl[1], scale=S), want[1], "[D,h,w] and [C,H,W]")
    gray = case(ref.SHAPES[2])
    got = cd.synthesize_right_view(dev(gray[0][0]), dev(gray[1][0, 0]), scale=2)
    assert_bitwise(got, gray[2][0, 0], "[H,W]")


def test_more_frames_than_the_grid_cap(cd):
    n = 66000
    rng = np.random.default_rng(3)
    prob = ref.softmax_noise(rng, n, 2, 1, 2)
    left = ref.uniform_left(rng, n, 1, 1, 2)
    got = cd.synthesize_right_view(dev(prob), dev(left), scale=1)
    assert_bitwise(got, ref.synthesize_right_view(prob, left, 1), "66000 frames")


@pytest.mark.parametrize("content", ["one_hot", "last_plane", "zeros_and_denormals"])
def test_probability_contents(cd, content):
    n, C, D, h, w, S = shape = ref.SHAPES[1]
    _, left, _ = case(shape)
    rng = np.random.default_rng(11)
    prob = np.zeros((n, D, h, w), F)
    if content == "one_hot":
        k = rng.integers(0, D, (n, h, w))
        np.put_along_axis(prob, k[:, None], 1.0, axis=1)
    elif content == "last_plane":
        prob[:, D - 1] = 1.0
    else:
        prob = ref.softmax_noise(rng, n, D, h, w)
        prob[:, ::3] = 0.0
        prob[:, 1::6] = F(1e-40)
        assert 0 < float(prob[0, 1, 0, 0]) < np.finfo(F).tiny
    got = cd.synthesize_right_view(dev(prob), dev(left), scale=S)
    want = ref.synthesize_right_view(prob, left, S)
    assert_bitwise(got, want, content)
    if content == "last_plane":
        assert np.all(want[..., w * S - (D - 1):] == 0.5)


@pytest.mark.parametrize("u8", [False, True])
def test_offset_operands_sentinels_side_stream_and_repeatability(cd, u8):
    """Every operand starts one element into its allocation (a uint8 frame at an odd address); out lies between two
    64-float sentinels; the call runs on a side stream, twice."""
    shape = ref.SHAPES[1]
    n, C, D, h, w, S = shape
    prob, left, want = case(shape, u8)
    pbuf = torch.zeros(prob.size + 1, device="cuda")
    lbuf = torch.zeros(left.size + 1, dtype=torch.uint8 if u8 else torch.float32, device="cuda")
    tp, tl = pbuf[1:].view(prob.shape), lbuf[1:].view(left.shape)
    tp.copy_(dev(prob))
    tl.copy_(dev(left))
    sentinel = -12345.5
    obuf = torch.full((1 + 64 + want.size + 64,), sentinel, device="cuda")
    out = obuf[65:65 + want.size].view(want.shape)
    assert tp.data_ptr() % 8 == 4 and out.data_ptr() % 8 == 4 and tl.is_contiguous() and out.is_contiguous()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert cd.synthesize_right_view(tp, tl, scale=S, out=out) is out
        first = out.clone()
        out.fill_(sentinel)
        cd.synthesize_right_view(tp, tl, scale=S, out=out)
    s.synchronize()
    assert_bitwise(first, want, "side stream, offset operands")
    assert_bitwise(out, first, "second run")
    guard = obuf.cpu().numpy()
    assert np.all(guard[:65] == sentinel) and np.all(guard[65 + want.size:] == sentinel)
    assert_bitwise(tp, prob, "prob untouched")


# ----------------------------------------------------------------------------- 2. the pipeline
H, W, K, DISP, SCALE, PLANES = 96, 160, 2, 32, 4, 33


@pytest.fixture(scope="module")
def scene():
    left, right, truth = syn.make_pair(H, W, DISP, K, 0)
    lowres = np.ascontiguousarray(truth[SCALE // 2::SCALE, SCALE // 2::SCALE], F)
    return syn.gray_to_rgb(left), syn.gray_to_rgb(right), lowres


def make_pipeline(synthesis=None):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=0, max_disparity=DISP - 1)
    return DepthEstimationPipeline(cfg, right_view_synthesis=synthesis)


@pytest.mark.parametrize("u8", [True, False])
def test_pipeline_synthesises_the_right_view(cd, scene, u8):
    from pipeline.synthesis import DisparityOracleModel, RightViewSynthesis
    left_rgb, _, lowres = scene
    model = DisparityOracleModel(torch.from_numpy(lowres), PLANES)
    left = torch.from_numpy(left_rgb.astype(np.uint8) if u8 else left_rgb).cuda()
    # what the head is given: the bytes, or the float frame over 255 as the device divides it
    head_left = left.cpu().numpy() if u8 else (left / 255.0).cpu().numpy()
    prob = model(torch.zeros((1, 3, H, W)), None).numpy()
    twin = ref.synthesize_right_view(prob, head_left[None], SCALE)[0]
    pipe = make_pipeline(RightViewSynthesis(model, full_resolution=(H, W), scale=SCALE))
    res = pipe.process(left)
    assert_bitwise(res.right_image, twin, "generated right view")
    assert res.left_image.data_ptr() == left.data_ptr()
    disparity = res.disparity_map.clone()
    again = pipe.process(left, torch.from_numpy(twin).cuda())
    assert_bitwise(again.disparity_map, disparity, "matching against the generated view")


def test_pipeline_accepts_a_model_that_returns_the_view(cd, scene):
    from pipeline.synthesis import RightViewSynthesis
    left_rgb, right_rgb, _ = scene
    view01 = torch.from_numpy(right_rgb * F(1.2 / 255.0) - F(0.1)).cuda()          # also outside 0..1: the clamp
    calls = []

    def traced(left_full, left_downscaled):
        calls.append((tuple(left_full.shape), tuple(left_downscaled.shape), float(left_full.max())))
        return view01[None]

    synthesis = RightViewSynthesis(traced, full_resolution=(H, W), scale=SCALE, model_output="view")
    got = synthesis.process(torch.from_numpy(left_rgb).cuda())
    assert_bitwise(got, ref.rescale(view01.cpu().numpy()), "rescale rule")
    assert calls[0][:2] == ((1, 3, H, W), (1, 3, H // SCALE, W // SCALE)) and calls[0][2] <= 1.0001
    assert synthesis.process(torch.from_numpy(left_rgb).cuda()).data_ptr() == got.data_ptr()       # persistent buffer


def test_pipeline_without_a_synthesiser_still_refuses(cd, scene):
    left = torch.from_numpy(scene[0]).cuda()
    with pytest.raises(RuntimeError) as e:
        make_pipeline().process(left)
    assert str(e.value) == "right_image is required: right-view synthesis (Deep3D) is not part of this build."
