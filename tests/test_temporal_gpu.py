"""Motion-gated temporal filter on the device (include/stereo_mi355x.h: smx_temporal_filter), cuda_depth.TemporalFilter
and the pipeline's temporal option.

The rule is a fixed sequence of float32 operations, so every expected map, state and guide copy comes from the CPU
reference (tests/temporal_ref.py), carried across the same sequence of calls, and is compared bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stereo_sequences as seqs                     # noqa: E402
import stereo_synthetic as syn                      # noqa: E402
import temporal_ref as ref                          # noqa: E402

NAN, INF = float("nan"), float("inf")
PARAMS = dict(motion_radius=2, motion_threshold=3.0, decay=0.7, max_diff=0.8, max_weight=5.0, min_weight=0.3,
              invalid_disparity=-1.0)


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def bits(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bitwise(got, expect, what):
    g, e = bits(got), bits(expect)
    assert g.shape == e.shape, f"{what}: shape {g.shape} != {e.shape}"
    bad = np.argwhere(g != e)
    assert bad.size == 0, f"{what}: {len(bad)} pixels differ, first at {tuple(bad[0])}"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def run(d, c, g, G, D, A, gout, out, p, stream=None):
    """smx_temporal_filter through the C ABI on device tensors; c and gout may be None."""
    from cuda_depth import _native as N
    n = 1 if d.dim() == 2 else int(d.shape[0])
    H, W = int(d.shape[-2]), int(d.shape[-1])
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    N.check(N.LIB.smx_temporal_filter(0, n, H, W, d.data_ptr(), None if c is None else c.data_ptr(), g.data_ptr(),
                                      G.data_ptr(), D.data_ptr(), A.data_ptr(), None if gout is None else gout.data_ptr(),
                                      out.data_ptr(), p["motion_radius"], p["motion_threshold"], p["decay"],
                                      p["max_diff"], p["max_weight"], p["min_weight"], p["invalid_disparity"], s))
    return out


def frames(rng, shape, count, inv=-1.0, special=0.02):
    """`count` (d, c, g): a map near a slanted surface with jitter and holes, a confidence with zeros and values > 1, a
    static noisy guide with a patch that moves every frame, and a few NaN / inf / marker values in each."""
    n, H, W = shape
    base = rng.integers(0, 200, shape).astype(np.float32)
    truth = (np.arange(H)[None, :, None] * 0.2 + 3.0 + np.zeros(shape)).astype(np.float32)
    out = []
    for f in range(count):
        d = (truth + rng.uniform(-0.6, 0.6, shape)).astype(np.float32)
        d[rng.random(shape) < 0.15] = inv
        c = rng.uniform(-0.2, 1.4, shape).astype(np.float32)
        g = np.clip(base + rng.integers(-2, 3, shape), 0, 255).astype(np.float32)
        x = (5 * f) % max(W - 8, 1)
        g[:, H // 3:H // 2, x:x + 8] += 60.0                                 # moving patch
        for a, vals in ((d, [NAN, INF, -INF, inv, -0.0, 1e-41]), (c, [NAN, INF, 0.0, -0.0, 1e-41]), (g, [NAN, INF])):
            m = rng.random(shape) < special
            a[m] = rng.choice(np.array(vals, np.float32), int(m.sum()))
        out.append((d, c, g))
    return out


# ----------------------------------------------------------------------------- 1. the C entry over sequences
@pytest.mark.parametrize("n,H,W", [(1, 1, 1), (1, 37, 61), (3, 20, 70), (2, 1, 300), (1, 300, 1), (4, 33, 129)])
@pytest.mark.parametrize("radius", [0, 1, 7])
@pytest.mark.parametrize("with_conf", [False, True])
def test_sequences_match_the_reference(cd, n, H, W, radius, with_conf):
    rng = np.random.default_rng(n * 1000 + H * 7 + W + radius * 3 + with_conf)
    p = dict(PARAMS, motion_radius=radius)
    shape = (n, H, W)
    r = ref.TemporalRef(shape, **p)
    D = dev(r.D)
    A = dev(r.A)
    G = dev(r.G)
    for f, (d, c, g) in enumerate(frames(rng, shape, 6)):
        td, tc, tg = dev(d), dev(c) if with_conf else None, dev(g)
        gout = torch.full_like(td, NAN)
        out = torch.full_like(td, NAN)
        run(td, tc, tg, G, D, A, gout, out, p)
        want = r.apply(d, g, c if with_conf else None)
        assert_bitwise(out, want, f"frame {f}: out")
        assert_bitwise(D, r.D, f"frame {f}: state_disp")
        assert_bitwise(A, r.A, f"frame {f}: state_weight")
        assert_bitwise(gout, g, f"frame {f}: guide_out")
        assert_bitwise(td, d, "disp untouched")
        G = gout


def test_streams_are_independent_and_in_place(cd):
    rng = np.random.default_rng(11)
    n, H, W = 5, 45, 140
    seq = frames(rng, (n, H, W), 5)
    batch = cd.TemporalFilter(n, H, W, **PARAMS)
    alone = [cd.TemporalFilter(1, H, W, **PARAMS) for _ in range(n)]
    for f, (d, c, g) in enumerate(seq):
        td, tc, tg = dev(d), dev(c), dev(g)
        got = batch.apply(td, tg, confidence=tc, out=td)                    # in place
        assert got.data_ptr() == td.data_ptr()
        for i in range(n):
            one = alone[i].apply(dev(d[i]), dev(g[i]), confidence=dev(c[i]))
            assert_bitwise(got[i], one, f"frame {f} stream {i}")


def test_class_ping_pong_against_caller_managed_guides(cd):
    """The class's guide buffers against the C entry with guide_out = NULL and the previous guide passed by hand."""
    rng = np.random.default_rng(12)
    shape = (3, 50, 90)
    seq = frames(rng, shape, 6)
    filt = cd.TemporalFilter(*shape, **PARAMS)
    r = ref.TemporalRef(shape, **PARAMS)
    D, A, prev = dev(r.D), dev(r.A), dev(r.G)
    for f, (d, c, g) in enumerate(seq):
        got = filt.apply(dev(d), dev(g))
        tg = dev(g)
        out = torch.empty_like(tg)
        run(dev(d), None, tg, prev, D, A, None, out, PARAMS)
        prev = tg
        want = r.apply(d, g)
        assert_bitwise(got, want, f"frame {f}: class")
        assert_bitwise(out, want, f"frame {f}: guide_out NULL")
        sd, sw = filt.state
        assert_bitwise(sd, r.D, "state D")
        assert_bitwise(sw, r.A, "state A")


def test_reset_one_stream(cd):
    rng = np.random.default_rng(13)
    shape = (4, 30, 64)
    seq = frames(rng, shape, 6, special=0.0)
    filt = cd.TemporalFilter(*shape, **PARAMS)
    r = ref.TemporalRef(shape, **PARAMS)
    for f, (d, c, g) in enumerate(seq):
        if f == 3:
            filt.reset(streams=[2])
            r.reset([2])
        if f == 5:
            filt.reset()
            r.reset()
        assert_bitwise(filt.apply(dev(d), dev(g), confidence=dev(c)), r.apply(d, g, c), f"frame {f}")
    # the first call after a full reset: the valid measurements, invalid_disparity elsewhere
    d = seq[-1][0]
    valid = np.isfinite(d) & (d != -1.0)
    filt.reset()
    assert_bitwise(filt.apply(dev(d), dev(seq[-1][2])), np.where(valid, d, np.float32(-1.0)), "reset semantics")


def test_full_c2_maps_and_an_hw_view(cd):
    rng = np.random.default_rng(14)
    n, H, W = 32, 375, 1242
    seq = frames(rng, (n, H, W), 3, inv=0.0, special=0.002)
    p = dict(PARAMS, motion_radius=1, invalid_disparity=0.0)
    filt = cd.TemporalFilter(n, H, W, **p)
    one = cd.TemporalFilter(1, H, W, **p)
    r = ref.TemporalRef((n, H, W), **p)
    for f, (d, c, g) in enumerate(seq):
        got = filt.apply(dev(d), dev(g), confidence=dev(c))
        assert_bitwise(got, r.apply(d, g, c), f"32 C2 maps, frame {f}")
        assert_bitwise(one.apply(dev(d[7]), dev(g[7]), confidence=dev(c[7])), got[7], "one [H, W] map alone")


def test_call_inside_a_captured_graph(cd):
    rng = np.random.default_rng(15)
    shape = (2, 40, 100)
    seq = frames(rng, shape, 3)
    r = ref.TemporalRef(shape, **PARAMS)
    d0, c0, g0 = seq[0]
    td, tc, tg = dev(d0), dev(c0), dev(g0)
    D, A, G = dev(r.D), dev(r.A), dev(r.G)
    gout, out = torch.empty_like(td), torch.empty_like(td)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run(td, tc, tg, G, D, A, gout, out, PARAMS, stream=torch.cuda.current_stream().cuda_stream)
    for f, (d, c, g) in enumerate(seq):                       # capture ran nothing: the state is still the reset one
        td.copy_(dev(d))
        tc.copy_(dev(c))
        tg.copy_(dev(g))
        graph.replay()
        G.copy_(gout)
        torch.cuda.synchronize()
        assert_bitwise(out, r.apply(d, g, c), f"replay {f}")


def test_python_entry_rejects_bad_operands(cd):
    filt = cd.TemporalFilter(2, 4, 8)
    t = torch.zeros((2, 4, 8), device="cuda")
    with pytest.raises(RuntimeError, match=r"disp must be float32 \(2, 4, 8\)"):
        filt.apply(t[0], t[0])
    with pytest.raises(RuntimeError, match="disp must be float32"):
        filt.apply(t.double(), t)
    with pytest.raises(RuntimeError, match="guide must be float32"):
        filt.apply(t, t[:1])
    with pytest.raises(RuntimeError, match="confidence must be float32"):
        filt.apply(t, t.clone(), confidence=t.half())
    with pytest.raises(RuntimeError, match="out must not overlap an operand other than disp"):
        filt.apply(t, t.clone(), out=filt.state[0])
    with pytest.raises(RuntimeError, match="stream index must be in 0..1"):
        filt.reset(streams=[2])


# ----------------------------------------------------------------------------- 2. pipeline
def _video(backend, H, W, dmax, count):
    """RGB frames of the moving synthetic sequence: static noisy background, an object moving 3 px per frame."""
    seq = seqs.moving_sequence(count, H, W, dmax + 1, 2, index=3, seed=17, step=3)
    return [(torch.from_numpy(syn.gray_to_rgb(l)).cuda(), torch.from_numpy(syn.gray_to_rgb(r)).cuda())
            for l, r, _ in seq]


@pytest.mark.parametrize("backend", ["cuda", "sgm"])
@pytest.mark.parametrize("confidence", [False, True])
def test_pipeline_temporal(cd, backend, confidence):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, dmax, inv = 64, 160, 31, -1.0
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=0, max_disparity=dmax, invalid_disparity=inv,
                                        stereo_matching_backend=backend, left_right_check=True)
    tp = dict(temporal_motion_radius=1, temporal_motion_threshold=4.0, temporal_decay=0.75, temporal_max_diff=1.0,
              temporal_max_weight=6.0, temporal_min_weight=0.25)
    post = dict(speckle_max_size=20, speckle_max_diff=1.0, confidence=confidence)
    plain = DepthEstimationPipeline(cfg, **post)
    pipe = DepthEstimationPipeline(cfg, temporal=True, **post, **tp)
    r = ref.TemporalRef((H, W), **{k[len("temporal_"):]: v for k, v in tp.items()}, invalid_disparity=inv)
    held = 0
    for f, (tl, tr) in enumerate(_video(backend, H, W, dmax, 6)):
        base_res = plain.process(tl, tr)
        base = base_res.disparity_map.clone()
        conf = base_res.confidence_map.cpu().numpy() if confidence else None
        res = pipe.process(tl, tr)
        guide = pipe._stereo_matching._median_guide.cpu().numpy()           # the matcher's left gray plane
        want = r.apply(base.cpu().numpy(), guide, conf)
        if f == 0 and not torch.isnan(base).any():
            assert_bitwise(res.disparity_map, base, "first frame equals temporal=False")
        assert_bitwise(res.disparity_map, want, f"{backend} frame {f}")
        if confidence:
            assert_bitwise(res.confidence_map, conf, "the confidence map is not changed")
        held += int(((base.cpu().numpy() == inv) & (want != inv)).sum())
    assert held > 0, "some pixels hold their history through an invalid measurement"
    # reset_temporal(): the next frame is the temporal=False map again
    pipe.reset_temporal()
    tl, tr = _video(backend, H, W, dmax, 1)[0]
    base = plain.process(tl, tr).disparity_map.clone()
    if not torch.isnan(base).any():
        assert_bitwise(pipe.process(tl, tr).disparity_map, base, "after reset_temporal")


@pytest.mark.parametrize("backend", ["cuda", "sgm"])
def test_pipeline_without_temporal_is_unchanged(cd, backend):
    """temporal=False keeps no history: the same frame gives the same bits whatever came before, and equals the map of a
    pipeline built without the temporal keywords."""
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, dmax = 64, 160, 31
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=0, max_disparity=dmax,
                                        stereo_matching_backend=backend, left_right_check=True)
    video = _video(backend, H, W, dmax, 3)
    a = DepthEstimationPipeline(cfg, speckle_max_size=20, temporal=False, temporal_decay=0.5)
    b = DepthEstimationPipeline(cfg, speckle_max_size=20)
    first = a.process(*video[0]).disparity_map.clone()
    for frame in video[1:]:
        a.process(*frame)
    assert_bitwise(a.process(*video[0]).disparity_map, first, "no state")
    assert_bitwise(b.process(*video[0]).disparity_map, first, "same as without the keywords")
    assert a._stereo_matching._temporal_filter is None
