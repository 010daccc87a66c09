"""Per-pixel confidence on the device (include/stereo_mi355x.h: smx_confidence_map), the SGM right-view map
(smx_sgm_with_right_map) and the pipeline's confidence option.

The confidence rule is a fixed sequence of float32 operations, so every expected map comes from the CPU reference
(tests/confidence_ref.py) and is compared bit for bit, whatever the kernel's split of the work."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import confidence_ref as ref                        # noqa: E402
import sgm_ref                                      # noqa: E402
import stereo_synthetic as syn                      # noqa: E402
import wls_ref                                      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REAL = os.path.join(HERE, "golden", "real", "real_crop_c2.npz")


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


def run(d, r=None, g=None, radius=2, lr_scale=1.0, texture_scale=10.0, invalid=-1.0, out=None, stream=None):
    """smx_confidence_map through the C ABI on device tensors; returns out."""
    from cuda_depth import _native as N
    n = 1 if d.dim() == 2 else int(d.shape[0])
    H, W = int(d.shape[-2]), int(d.shape[-1])
    if out is None:
        out = torch.full_like(d, float("nan"))
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    N.check(N.LIB.smx_confidence_map(0, n, H, W, d.data_ptr(), None if r is None else r.data_ptr(),
                                     None if g is None else g.data_ptr(), radius, lr_scale, texture_scale, invalid,
                                     out.data_ptr(), s))
    return out


def random_map(rng, shape, invalid=-1.0, special_frac=0.1, invalid_frac=0.2):
    d = (rng.integers(0, 12, shape) + rng.uniform(-0.7, 0.7, shape)).astype(np.float32)
    d[rng.random(shape) < invalid_frac] = invalid
    payload = np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]
    specials = np.array([np.nan, payload, np.inf, -np.inf, invalid, -0.0, 0.0, 1e-42], np.float32)
    mask = rng.random(shape) < special_frac
    d[mask] = rng.choice(specials, int(mask.sum()))
    return d


def random_guide(rng, shape, nan_frac=0.03):
    g = (rng.integers(0, 6, shape) * 3.0 + rng.uniform(0, 2, shape)).astype(np.float32)
    m = rng.random(shape)
    g[m < nan_frac] = np.nan
    g[(m >= nan_frac) & (m < nan_frac + 0.01)] = np.inf
    g[(m >= nan_frac + 0.01) & (m < nan_frac + 0.02)] = -0.0
    return g


# ----------------------------------------------------------------------------- 1. random maps, shapes, operands
@pytest.mark.parametrize("n,H,W", [(1, 1, 1), (1, 1, 300), (1, 300, 1), (3, 37, 61), (1, 33, 200), (32, 20, 70),
                                   (1, 2, 32768), (3, 71, 129)])
@pytest.mark.parametrize("radius", [1, 2, 15])
def test_random_maps(cd, n, H, W, radius):
    rng = np.random.default_rng(n * 7 + H * 1000 + W + radius)
    d = random_map(rng, (n, H, W))
    r = random_map(rng, (n, H, W))
    g = random_guide(rng, (n, H, W))
    td, tr, tg = dev(d), dev(r), dev(g)
    for right, tright in ((None, None), (r, tr)):
        for guide, tguide in ((None, None), (g, tg)):
            got = run(td, tright, tguide, radius=radius, lr_scale=0.75, texture_scale=6.0)
            want = ref.confidence_map(d, right, guide, radius=radius, lr_scale=0.75, texture_scale=6.0)
            assert_bitwise(got, want, f"right {right is not None} guide {guide is not None}")
    assert_bitwise(td, d, "left untouched")


def test_full_c2_maps_and_other_marker(cd):
    rng = np.random.default_rng(21)
    n, H, W = 32, 375, 1242
    d = random_map(rng, (n, H, W), invalid=0.0, special_frac=0.01)
    r = random_map(rng, (n, H, W), invalid=0.0, special_frac=0.01)
    g = random_guide(rng, (n, H, W), nan_frac=0.001)
    got = run(dev(d), dev(r), dev(g), invalid=0.0)
    assert_bitwise(got, ref.confidence_map(d, r, g, invalid_disparity=0.0), "32 C2 maps")
    one = run(dev(d[5]), dev(r[5]), dev(g[5]), invalid=0.0)
    assert_bitwise(one, got[5], "one map alone")


def test_tiny_scales_and_aliased_inputs(cd):
    rng = np.random.default_rng(22)
    d = random_map(rng, (2, 40, 90))
    g = random_guide(rng, d.shape)
    td, tg = dev(d), dev(g)
    assert_bitwise(run(td, td, td, radius=3, lr_scale=3e-39, texture_scale=1e-40),
                   ref.confidence_map(d, d, d, radius=3, lr_scale=3e-39, texture_scale=1e-40), "aliased, denormals")
    assert_bitwise(run(td, None, tg, radius=1, lr_scale=1e30, texture_scale=3e38),
                   ref.confidence_map(d, None, g, radius=1, lr_scale=1e30, texture_scale=3e38), "huge scales")


def test_garbage_out_is_rewritten(cd):
    rng = np.random.default_rng(23)
    d = random_map(rng, (3, 50, 130))
    r, g = random_map(rng, d.shape), random_guide(rng, d.shape)
    want = ref.confidence_map(d, r, g)
    for fill in (0xFF, 0x7F, 0x00):
        out = torch.full(d.shape, 0, dtype=torch.float32, device="cuda")
        out.view(torch.uint8).fill_(fill)
        assert_bitwise(run(dev(d), dev(r), dev(g), out=out), want, f"out filled with {fill:#x}")


def test_side_stream_and_python_entry(cd):
    rng = np.random.default_rng(24)
    d = random_map(rng, (2, 64, 150))
    r, g = random_map(rng, d.shape), random_guide(rng, d.shape)
    td, tr, tg = dev(d), dev(r), dev(g)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = cd.confidence_map(td, tr, tg, radius=3, lr_scale=2.0, texture_scale=5.0)
        out2 = cd.confidence_map(td[0], guide=tg[0])
    s.synchronize()
    assert_bitwise(out, ref.confidence_map(d, r, g, radius=3, lr_scale=2.0, texture_scale=5.0), "side stream")
    assert_bitwise(out2, ref.confidence_map(d[0], None, g[0]), "[H,W], defaults")


def test_call_inside_a_captured_graph(cd):
    rng = np.random.default_rng(25)
    n, H, W = 3, 64, 150
    d = random_map(rng, (n, H, W))
    r, g = random_map(rng, d.shape), random_guide(rng, d.shape)
    td, tr, tg = dev(d), dev(r), dev(g)
    out1, out2 = torch.empty_like(td), torch.empty_like(td)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        run(td, tr, tg, radius=2, out=out1, stream=cs)
        run(td, None, tg, radius=15, out=out2, stream=cs)
    out1.zero_()
    out2.zero_()
    d2 = random_map(rng, d.shape)                                     # new inputs in the captured buffers
    td.copy_(dev(d2))
    graph.replay()
    torch.cuda.synchronize()
    assert_bitwise(out1, ref.confidence_map(d2, r, g, radius=2), "replay, LR and texture")
    assert_bitwise(out2, ref.confidence_map(d2, None, g, radius=15), "replay, texture, radius 15")


def test_python_entry_rejects_bad_operands(cd):
    t = torch.zeros((2, 4, 8), device="cuda")
    with pytest.raises(RuntimeError, match="float32"):
        cd.confidence_map(t.double())
    with pytest.raises(RuntimeError, match="right_disp must be float32"):
        cd.confidence_map(t, t[0])
    with pytest.raises(RuntimeError, match="guide must be float32"):
        cd.confidence_map(t, guide=t.double())
    with pytest.raises(RuntimeError, match="out must not overlap"):
        cd.confidence_map(t, out=t)


# ----------------------------------------------------------------------------- 2. real inputs
@pytest.mark.parametrize("rgb", [False, True])
def test_engine_lr_maps_on_c2_pairs(cd, rgb):
    n, H, W, D = 4, 375, 1242, 128
    cfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=2, min_disparity=0, max_disparity=D - 1)
    sm = cd.StereoMatching(cfg, max_batch=2 * n)
    ls, rs = syn.make_batch(n, H, W, D, 2, 40)
    if rgb:
        ls, rs = np.stack([syn.gray_to_rgb(x) for x in ls]), np.stack([syn.gray_to_rgb(x) for x in rs])
    right_out = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
    lr = sm.compute_disparity_map_batch_lr(torch.from_numpy(ls).cuda(), torch.from_numpy(rs).cuda(),
                                           right_out=right_out).clone()
    if rgb:                                                           # the engine's gray planes
        guides = torch.stack([sm.intermediate(0, k).clone() for k in range(n)])
    else:                                                             # gray inputs are their own gray planes
        guides = torch.from_numpy(np.ascontiguousarray(ls)).cuda()
    got = cd.confidence_map(lr, right_out, guides)
    want = ref.confidence_map(lr.cpu().numpy(), right_out.cpu().numpy(), guides.cpu().numpy())
    assert_bitwise(got, want, "engine LR maps")
    valid = lr.cpu().numpy() != -1.0
    print(f"mean confidence of the valid pixels {float(want[valid].mean()):.3f}")
    assert float(want[valid].mean()) > 0.3


@pytest.mark.skipif(not os.path.exists(REAL), reason="tests/golden/real/real_crop_c2.npz not present")
def test_real_crop(cd):
    z = np.load(REAL)
    L, R = z["left_rgb"].astype(np.float32), z["right_rgb"].astype(np.float32)
    dmin, dmax = (int(v) for v in z["disparity_range"])
    H, W = L.shape[1:]
    cfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=2, min_disparity=dmin, max_disparity=dmax)
    sm = cd.StereoMatching(cfg, max_batch=2)
    right_out = torch.empty((1, H, W), dtype=torch.float32, device="cuda")
    lr = sm.compute_disparity_map_batch_lr(torch.from_numpy(L[None]).cuda(), torch.from_numpy(R[None]).cuda(),
                                           right_out=right_out)[0].clone()
    guide = sm.intermediate(0, 0).clone()
    spk = cd.filter_speckles(lr, max_speckle_size=100, max_diff=1.0)
    got = cd.confidence_map(spk, right_out[0], guide)
    assert_bitwise(got, ref.confidence_map(spk.cpu().numpy(), right_out[0].cpu().numpy(), guide.cpu().numpy()),
                   "real crop")


def _sgm_expect(left, right, dmin, D, paths, P1, P2, invalid):
    """sgm_ref's right-view winners iR as the right-view map: f32(dmin + iR), invalid where iR = -1."""
    maps = []
    for lf, rf in zip(left, right):
        cv = sgm_ref.cost_volume(sgm_ref.census(sgm_ref.gray(lf)), sgm_ref.census(sgm_ref.gray(rf)), dmin, D)
        iR = sgm_ref.right_wta(sgm_ref.aggregate(cv, paths, P1, P2), dmin)
        maps.append(np.where(iR >= 0, (dmin + iR).astype(np.float32), np.float32(invalid)).astype(np.float32))
    return np.stack(maps)


@pytest.mark.parametrize("lr", [None, 1.0])
@pytest.mark.parametrize("n,H,W,dmin,D,paths", [(1, 17, 23, 2, 12, 8), (3, 20, 70, 0, 24, 4), (1, 9, 120, 75, 65, 8)])
def test_sgm_right_map(cd, lr, n, H, W, dmin, D, paths):
    rng = np.random.default_rng(H * W + D)
    base = rng.integers(0, 256, (n, 3, H, W + 8)).astype(np.float64)
    base = (base + np.roll(base, 1, -1) + np.roll(base, 1, -2)) / 3
    left = np.rint(base[..., 4:4 + W]).astype(np.uint8)
    right = np.rint(np.clip(base[..., :W] + rng.integers(-3, 4, (n, 3, H, W)), 0, 255)).astype(np.uint8)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    sgm = cd.StereoSGM(dmin, dmin + D - 1, paths=paths, lr_max_diff=lr, invalid_disparity=-3.5)
    shape = (n, H, W)
    out_a, gray_a = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
    out_b, gray_b = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
    right_map = torch.full(shape, float("nan"), device="cuda")
    sgm.compute(tl, tr, out=out_a, gray_out=gray_a)
    sgm.compute(tl, tr, out=out_b, gray_out=gray_b, right_out=right_map)
    assert_bitwise(out_b, out_a, "out equals smx_sgm's")
    assert_bitwise(gray_b, gray_a, "gray plane equals smx_sgm's")
    assert_bitwise(right_map, _sgm_expect(left, right, dmin, D, paths, 10, 120, -3.5), "right-view map")
    conf = cd.confidence_map(out_b, right_map, gray_b, invalid_disparity=-3.5)
    assert_bitwise(conf, ref.confidence_map(out_b.cpu().numpy(), right_map.cpu().numpy(), gray_b.cpu().numpy(),
                                            invalid_disparity=-3.5), "SGM maps")


# ----------------------------------------------------------------------------- 3. pipeline
def _pipeline_pair(H, W, dmin, dmax, seed=5):
    return syn.random_rgb_pair(H, W, dmax + 1, 2, seed, dmin=dmin)


@pytest.mark.parametrize("backend", ["cuda", "sgm"])
@pytest.mark.parametrize("lr_check", [False, True])
def test_pipeline_confidence_and_wls(cd, backend, lr_check):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, dmin, dmax, inv = 64, 128, 8, 39, -7.0
    L, R = _pipeline_pair(H, W, dmin, dmax)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=dmin, max_disparity=dmax,
                                        invalid_disparity=inv, stereo_matching_backend=backend,
                                        left_right_check=lr_check)
    conf_kw = dict(confidence=True, confidence_lr_scale=0.8, confidence_radius=3, confidence_texture_scale=12.0)
    plain = DepthEstimationPipeline(cfg, speckle_max_size=10, speckle_max_diff=0.5)
    base = plain.process(tl, tr).disparity_map.clone()
    pipe = DepthEstimationPipeline(cfg, speckle_max_size=10, speckle_max_diff=0.5, **conf_kw)
    res = pipe.process(tl, tr)
    assert_bitwise(res.disparity_map, base, "confidence=True leaves the map as it was")
    backend_obj = pipe._stereo_matching
    guide = backend_obj._median_guide.cpu().numpy()
    right = backend_obj._right_map.reshape(H, W).cpu().numpy() if lr_check else None
    assert (backend_obj._right_map is None) == (not lr_check)
    conf = ref.confidence_map(base.cpu().numpy(), right, guide, radius=3, lr_scale=0.8, texture_scale=12.0,
                              invalid_disparity=inv)
    assert_bitwise(res.confidence_map, conf, f"{backend} LR {lr_check}: confidence")
    assert plain.process(tl, tr).confidence_map is None
    if lr_check:                                                      # the right-view map is the matcher's own
        if backend == "cuda":
            ecfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=2, min_disparity=dmin,
                                                  max_disparity=dmax)
            ro = torch.empty((1, H, W), dtype=torch.float32, device="cuda")
            cd.StereoMatching(ecfg, max_batch=2).compute_disparity_map_batch_lr(tl[None], tr[None], right_out=ro,
                                                                                invalid_disparity=inv)
            assert_bitwise(ro[0], right, "cuda right-view map")
        else:
            ro = torch.empty((H, W), dtype=torch.float32, device="cuda")
            cd.StereoSGM(dmin, dmax, lr_max_diff=1.0, invalid_disparity=inv).compute(tl, tr, right_out=ro)
            assert_bitwise(ro, right, "sgm right-view map")
    # with the WLS filter, the filter is weighted by that confidence
    wpipe = DepthEstimationPipeline(cfg, speckle_max_size=10, speckle_max_diff=0.5, wls_lambda=3000.0,
                                    wls_sigma_color=2.0, wls_iterations=2, **conf_kw)
    wres = wpipe.process(tl, tr)
    assert_bitwise(wres.confidence_map, conf, "confidence beside the WLS filter")
    lam, rw = cd.wls_tables(3000.0, 2.0, 2, 0.25)
    want = wls_ref.wls_filter(base.cpu().numpy(), guide, lam, rw, confidence=conf, invalid_disparity=inv)
    assert_bitwise(wres.disparity_map, want, f"{backend} LR {lr_check}: WLS driven by the confidence")
    wres2 = wpipe.process(tl, tr)                                     # the buffers are reused
    assert_bitwise(wres2.disparity_map, want, "second frame")
    assert wres2.confidence_map.data_ptr() == wres.confidence_map.data_ptr()


def test_pipeline_confidence_with_rectification_and_fill(cd):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, dmin, dmax, inv = 48, 96, 4, 35, -1.0
    L, R = _pipeline_pair(H, W, dmin, dmax, seed=9)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    mx, my = np.meshgrid(np.arange(W, dtype=np.float64) + 0.5, np.arange(H, dtype=np.float64))   # half-pixel shift
    qmap = cd.quantize_map(mx, my, (H, W))
    rect = cd.StereoRectification(qmap, qmap, (H, W), (H, W))
    valid_rect = rect.left_valid.cpu().numpy()
    assert not valid_rect.all(), "the shift leaves an invalid border"
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=dmin, max_disparity=dmax,
                                        invalid_disparity=inv, stereo_matching_backend="cuda", left_right_check=True)
    holes = DepthEstimationPipeline(cfg, speckle_max_size=5, confidence=True, rectification=rect)
    r0 = holes.process(tl, tr)
    d0, c0 = r0.disparity_map.cpu().numpy(), r0.confidence_map.cpu().numpy()
    pipe = DepthEstimationPipeline(cfg, speckle_max_size=5, fill_invalid=True, confidence=True, rectification=rect)
    res = pipe.process(tl, tr)
    conf, d = res.confidence_map.cpu().numpy(), res.disparity_map.cpu().numpy()
    assert_bitwise(conf, c0, "the fill does not change the confidence")
    assert np.all(conf[~valid_rect] == 0)
    assert np.all(conf[d0 == inv] == 0), "removed and filled pixels have confidence 0"
    assert np.all(d[valid_rect] != inv) and np.any(d0[valid_rect] == inv)
    assert np.all((conf >= 0) & (conf <= 1)) and float(conf[d0 != inv].mean()) > 0.2
