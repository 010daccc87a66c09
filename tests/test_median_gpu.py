"""Image-guided weighted median on the device (include/stereo_mi355x.h: smx_weighted_median).

The rule names one value per pixel (a sample of its window), so the output does not depend on how the kernel splits
the work: every expected value comes from the CPU reference (tests/median_ref.py) and is compared bit for bit.  The
occlusion scene is the one behavioural test."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import median_ref as ref                            # noqa: E402
import postprocess_ref as post                      # noqa: E402
import stereo_synthetic as syn                      # noqa: E402

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
    bad = np.argwhere(g != e)
    assert bad.size == 0, f"{what}: {len(bad)} pixels differ, first at {tuple(bad[0])}"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def run(cd, d, g, radius, rw, sw, holes=None, out=None, invalid=-1.0, workspace=None, stream=None):
    """smx_weighted_median through the C ABI on tensors (d, g, holes, out on the device); returns out."""
    from cuda_depth import _native as N
    n = 1 if d.dim() == 2 else int(d.shape[0])
    H, W = int(d.shape[-2]), int(d.shape[-1])
    if out is None:
        out = torch.empty_like(d)
    rw, sw = np.ascontiguousarray(rw, np.uint16), np.ascontiguousarray(sw, np.uint16)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    N.check(N.LIB.smx_weighted_median(0, n, H, W, d.data_ptr(), None if holes is None else holes.data_ptr(),
                                      g.data_ptr(), out.data_ptr(), radius, rw.ctypes.data, sw.ctypes.data, invalid,
                                      None if workspace is None else workspace.data_ptr(),
                                      0 if workspace is None else workspace.numel(), s))
    return out


def random_map(rng, shape, invalid=-1.0, special_frac=0.15):
    """A few disparity levels plus noise (so that windows hold ties and spreads), with the specials sprinkled in: NaN
    (with a payload), +-inf, the invalid value, -0.0 and +0.0."""
    d = (rng.integers(0, 6, shape) * 4.0 + rng.uniform(-0.5, 0.5, shape)).astype(np.float32)
    payload = np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]
    specials = np.array([np.nan, payload, np.inf, -np.inf, invalid, -0.0, 0.0], np.float32)
    mask = rng.random(shape) < special_frac
    d[mask] = rng.choice(specials, int(mask.sum()))
    return d


def random_guide(rng, shape):
    g = rng.uniform(0, 255, shape).astype(np.float32)
    g[rng.random(shape) < 0.02] = np.nan
    g[rng.random(shape) < 0.02] = 400.0                              # differences of 255 and more
    return g


def random_tables(rng, radius):
    rw = rng.integers(0, 1024, 256).astype(np.uint16)
    sw = rng.integers(0, 1024, (radius + 1) ** 2).astype(np.uint16)
    rw[rng.random(256) < 0.2] = 0
    sw[rng.random(sw.size) < 0.2] = 0
    rw[:4] = 1023                                                    # similar pixels always count
    sw[0] = 1023
    return rw, sw


def holes_of(rng, d, frac=0.3, invalid=-1.0):
    h = d.copy()
    h[rng.random(d.shape) < frac] = invalid
    return h


# ----------------------------------------------------------------------------- 1. random maps, radii, shapes, modes
@pytest.mark.parametrize("radius", [1, 9, 15])
@pytest.mark.parametrize("n,H,W", [(1, 1, 1), (1, 1, 300), (1, 300, 1), (2, 37, 61), (1, 64, 64), (3, 33, 95),
                                   (1, 19, 129)])
def test_random_maps_both_modes(cd, radius, n, H, W):
    rng = np.random.default_rng(radius * 100000 + H * 1000 + W)
    d = random_map(rng, (n, H, W))
    g = random_guide(rng, (n, H, W))
    h = holes_of(rng, d)
    rw, sw = random_tables(rng, radius)
    td, tg, th = dev(d), dev(g), dev(h)
    assert_bitwise(run(cd, td, tg, radius, rw, sw), ref.weighted_median(d, g, radius, rw, sw), "whole map")
    assert_bitwise(run(cd, td, tg, radius, rw, sw, holes=th), ref.weighted_median(d, g, radius, rw, sw, holes=h),
                   "holes")
    assert_bitwise(td, d, "in untouched")
    assert_bitwise(th, h, "holes untouched")


def test_other_marker_and_two_dimensional_entry(cd):
    rng = np.random.default_rng(7)
    d = random_map(rng, (50, 70), invalid=0.0, special_frac=0.3)
    g = random_guide(rng, (50, 70))
    for radius, sc, ss in ((2, 10.0, 5.0), (6, 3.0, 2.0)):
        rw, sw = cd.median_weight_tables(radius, sc, ss)
        got = cd.weighted_median(dev(d), dev(g), radius=radius, sigma_color=sc, sigma_space=ss, invalid_disparity=0.0)
        assert_bitwise(got, ref.weighted_median(d, g, radius, rw, sw, invalid_disparity=0.0), f"r {radius} marker 0")
        h = holes_of(rng, d, invalid=0.0)
        got = cd.weighted_median(dev(d), dev(g), radius=radius, sigma_color=sc, sigma_space=ss, holes=dev(h),
                                 invalid_disparity=0.0)
        assert_bitwise(got, ref.weighted_median(d, g, radius, rw, sw, holes=h, invalid_disparity=0.0),
                       f"r {radius} marker 0 holes")


def test_maps_are_independent(cd):
    """Map i's last rows equal map i + 1's first rows with other values: a window that ran across the boundary would
    see them."""
    rng = np.random.default_rng(8)
    n, H, W = 4, 12, 40
    d = np.stack([np.full((H, W), 3.0 * (i + 1), np.float32) for i in range(n)])
    d[:, H // 2] = -1.0
    g = np.zeros_like(d)
    rw, sw = np.full(256, 1023, np.uint16), np.full(16, 1023, np.uint16)
    got = run(cd, dev(d), dev(g), 3, rw, sw, holes=dev(d))
    exp = ref.weighted_median(d, g, 3, rw, sw, holes=d)
    assert_bitwise(got, exp, "independent maps")
    for i in range(n):
        assert np.all(exp[i] == 3.0 * (i + 1))
    r2, g2 = random_map(rng, (n, H, W)), random_guide(rng, (n, H, W))
    batch = run(cd, dev(r2), dev(g2), 3, rw, sw)
    for i in range(n):                                                 # each map alone gives the same bits
        assert_bitwise(batch[i], run(cd, dev(r2[i]), dev(g2[i]), 3, rw, sw), f"map {i} alone")


# ----------------------------------------------------------------------------- 2. aliasing, workspace, graphs
def test_out_is_holes_and_holes_is_in(cd):
    rng = np.random.default_rng(9)
    d = random_map(rng, (2, 45, 77))
    g = random_guide(rng, d.shape)
    h = holes_of(rng, d)
    rw, sw = random_tables(rng, 5)
    filled = post.fill_invalid(h)                                    # the usual pair: (filled map, pre-fill map)
    tf, th = dev(filled), dev(h)
    run(cd, tf, dev(g), 5, rw, sw, holes=th, out=th)                 # writes over the pre-fill map
    assert_bitwise(th, ref.weighted_median(filled, g, 5, rw, sw, holes=h), "out == holes")
    assert_bitwise(tf, filled, "in untouched")
    td = dev(d)
    got = run(cd, td, dev(g), 5, rw, sw, holes=td)                    # weighted-median fill, no background fill
    assert_bitwise(got, ref.weighted_median(d, g, 5, rw, sw, holes=d), "holes == in")
    tg = dev(g)
    got = run(cd, tg, tg, 5, rw, sw, holes=tg)                        # every input the same buffer
    assert_bitwise(got, ref.weighted_median(g, g, 5, rw, sw, holes=g), "in == holes == guide")


def test_workspace_contents_do_not_matter(cd):
    rng = np.random.default_rng(10)
    d = random_map(rng, (2, 40, 66))
    g = random_guide(rng, d.shape)
    h = holes_of(rng, d)
    rw, sw = random_tables(rng, 4)
    from cuda_depth import _native as N
    nbytes = max(int(N.LIB.smx_median_workspace_bytes(2, 40, 66)), 4096)   # more than the query is allowed
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    for _ in range(2):
        got = run(cd, dev(d), dev(g), 4, rw, sw, holes=dev(h), workspace=ws)
        assert_bitwise(got, ref.weighted_median(d, g, 4, rw, sw, holes=h), "garbage workspace")


def test_call_inside_a_captured_graph(cd):
    rng = np.random.default_rng(12)
    n, H, W = 3, 64, 150
    d, g = random_map(rng, (n, H, W)), random_guide(rng, (n, H, W))
    h = holes_of(rng, d)
    rw, sw = random_tables(rng, 9)
    rw0 = rw.copy()
    td, tg, th = dev(d), dev(g), dev(h)
    out1, out2 = torch.empty_like(td), torch.empty_like(td)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        run(cd, td, tg, 9, rw, sw, holes=th, out=out1, stream=cs)
        run(cd, td, tg, 9, rw, sw, out=out2, stream=cs)
    rw[:] = 0                                                         # the tables were copied at capture
    out1.zero_()
    out2.zero_()
    graph.replay()
    torch.cuda.synchronize()
    rw = rw0
    assert_bitwise(out1, ref.weighted_median(d, g, 9, rw, sw, holes=h), "replay, holes")
    assert_bitwise(out2, ref.weighted_median(d, g, 9, rw, sw), "replay, whole map")


def test_python_entry_rejects_bad_operands(cd):
    t = torch.zeros((2, 4, 8), device="cuda")
    g = torch.zeros((2, 4, 8), device="cuda")
    kw = dict(radius=2, sigma_color=10.0, sigma_space=5.0)
    with pytest.raises(RuntimeError, match="float32"):
        cd.weighted_median(t.double(), g, **kw)
    with pytest.raises(RuntimeError, match="guide must be float32"):
        cd.weighted_median(t, g[0], **kw)
    with pytest.raises(RuntimeError, match="holes must be float32"):
        cd.weighted_median(t, g, holes=t.double(), **kw)
    with pytest.raises(RuntimeError, match="out must not overlap in or guide"):
        cd.weighted_median(t, g, out=t, **kw)
    with pytest.raises(RuntimeError, match="out must not overlap in or guide"):
        cd.weighted_median(t, g, out=g, **kw)


# ----------------------------------------------------------------------------- 3. end to end, behaviour, pipeline
@pytest.mark.skipif(not os.path.exists(REAL), reason="tests/golden/real/real_crop_c2.npz not present")
def test_real_crop_lr_speckles_fill_median(cd):
    z = np.load(REAL)
    L, R = z["left_rgb"].astype(np.float32), z["right_rgb"].astype(np.float32)
    dmin, dmax = (int(v) for v in z["disparity_range"])
    H, W = L.shape[1:]
    cfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=2, min_disparity=dmin, max_disparity=dmax)
    sm = cd.StereoMatching(cfg, max_batch=2)
    lr = sm.compute_disparity_map_batch_lr(torch.from_numpy(L[None]).cuda(), torch.from_numpy(R[None]).cuda())[0]
    guide = sm.intermediate(0, 0).clone()                            # the left gray plane of the LR call
    spk = cd.filter_speckles(lr, max_speckle_size=100, max_diff=1.0)
    filled = cd.fill_invalid(spk)
    got = cd.weighted_median(filled, guide, radius=9, sigma_color=10.0, sigma_space=5.0, holes=spk)
    exp_spk = post.filter_speckles(lr.cpu().numpy(), 100, 1.0, -1.0)
    exp_fill = post.fill_invalid(exp_spk)
    g = guide.cpu().numpy()
    rw, sw = cd.median_weight_tables(9, 10.0, 5.0)
    exp = ref.weighted_median(exp_fill, g, 9, rw, sw, holes=exp_spk)
    assert_bitwise(spk, exp_spk, "real crop speckles")
    assert_bitwise(filled, exp_fill, "real crop fill")
    assert_bitwise(got, exp, "real crop median")
    changed = int((bits(exp) != bits(exp_fill)).sum())
    holes = int((exp_spk == -1.0).sum())
    print(f"real crop: {holes} filled pixels, {changed} changed by the median")
    assert 0 < changed <= holes
    rw2, sw2 = cd.median_weight_tables(2, 10.0, 5.0)                 # whole-map mode, small window (fast reference)
    assert_bitwise(cd.weighted_median(filled, guide, radius=2, sigma_color=10.0, sigma_space=5.0),
                   ref.weighted_median(exp_fill, g, 2, rw2, sw2), "real crop whole map")


def occlusion_scene(H=128, W=256, d_bg=8, d_fg=28, fg_rows=(32, 96), fg_cols=(120, 200), seed=4):
    """A textured background at d_bg and a brighter textured box at d_fg in front of it.  Right image: the background
    shifted by d_bg, the box by d_fg on top.  Returns (left gray, right gray, true left disparity, occluded mask)."""
    rng = np.random.default_rng(seed)
    bg = rng.uniform(20, 110, (H, W + d_fg + 8)).astype(np.float32)
    fg = rng.uniform(150, 240, (H, W + d_fg + 8)).astype(np.float32)
    x = np.arange(H)[:, None]
    y = np.arange(W)[None, :]
    in_rows = (x >= fg_rows[0]) & (x < fg_rows[1])
    in_box = in_rows & (y >= fg_cols[0]) & (y < fg_cols[1])
    left = np.where(in_box, fg[:, :W], bg[:, :W]).astype(np.float32)
    yr = y + d_fg                                                     # right pixel yr shows left column yr + d
    box_r = in_rows & (yr >= fg_cols[0]) & (yr < fg_cols[1])
    right = np.where(box_r, fg[:, d_fg:d_fg + W], bg[:, d_bg:d_bg + W]).astype(np.float32)
    truth = np.where(in_box, float(d_fg), float(d_bg)).astype(np.float32)
    occluded = in_rows & (y >= fg_cols[0] - (d_fg - d_bg)) & (y < fg_cols[0])
    return left, right, truth, occluded


@pytest.mark.xfail(strict=True, reason="measured on an MI355X: on this scene the background fill is already exact on "
                   "the strip (MAE 0.000) and fill + median has MAE 0.191; the expectation does not hold here (DESIGN.md)")
def test_median_pulls_filled_pixels_towards_similar_neighbours(cd):
    """LR check, fill, then fill + median on the occlusion scene.  On the pixels the fill wrote around the box's left
    edge (the occluded strip and whatever the check removed next to it), fill + median should be closer to the true
    disparity than the fill alone.  It is not: the background here has one disparity, so the fill's value is the true
    one, and the median can only move a filled pixel to another value of its window.  The kernel is still compared bit
    for bit with the reference before the expectation is checked."""
    H, W, D = 128, 256, 48
    left, right, truth, occluded = occlusion_scene(H, W)
    cfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=2, min_disparity=0, max_disparity=D - 1)
    sm = cd.StereoMatching(cfg, max_batch=2)
    L, R = syn.gray_to_rgb(left), syn.gray_to_rgb(right)
    lr = sm.compute_disparity_map_batch_lr(torch.from_numpy(L[None]).cuda(), torch.from_numpy(R[None]).cuda())[0]
    guide = sm.intermediate(0, 0).clone()
    filled = cd.fill_invalid(lr)
    med = cd.weighted_median(filled, guide, radius=9, sigma_color=10.0, sigma_space=5.0, holes=lr)
    holes = (lr == -1.0).cpu().numpy()
    x = np.arange(H)[:, None]
    y = np.arange(W)[None, :]
    strip = holes & (x >= 32) & (x < 96) & (y >= 120 - 2 * 20) & (y < 120 + 8)
    assert occluded.sum() > 0 and strip.sum() >= 0.5 * occluded.sum(), (strip.sum(), occluded.sum())
    f, m = filled.cpu().numpy(), med.cpu().numpy()
    mae_fill = float(np.abs(f[strip] - truth[strip]).mean())
    mae_med = float(np.abs(m[strip] - truth[strip]).mean())
    print(f"occlusion strip: {int(strip.sum())} filled pixels, MAE fill {mae_fill:.3f}, fill + median {mae_med:.3f}")
    g = guide.cpu().numpy()
    rw, sw = cd.median_weight_tables(9, 10.0, 5.0)
    assert_bitwise(med, ref.weighted_median(f, g, 9, rw, sw, holes=lr.cpu().numpy()), "scene median")
    assert mae_med < mae_fill, (mae_med, mae_fill)


def _pipeline_pair(H, W, dmin, dmax, seed=5):
    return syn.random_rgb_pair(H, W, dmax + 1, 2, seed, dmin=dmin)


def test_pipeline_options_equal_the_standalone_chain(cd):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, dmin, dmax = 64, 128, 8, 39
    L, R = _pipeline_pair(H, W, dmin, dmax)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    cfg = dict(image_shape=(H, W), min_disparity=dmin, max_disparity=dmax, invalid_disparity=-7.0)
    ecfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=2, min_disparity=dmin,
                                          max_disparity=dmax)
    sm = cd.StereoMatching(ecfg, max_batch=2)
    for lr in (True, False):
        if lr:
            base = sm.compute_disparity_map_batch_lr(tl[None], tr[None], invalid_disparity=-7.0)[0].clone()
        else:
            base = sm.compute_disparity_map(tl, tr).clone()
        guide = sm.intermediate(0, 0).clone()
        for size, fill, radius in ((0, False, 3), (0, True, 3), (10, True, 7)):
            pipe = DepthEstimationPipeline(DepthEstimationPipelineConfig(**cfg, left_right_check=lr),
                                           speckle_max_size=size, speckle_max_diff=0.5, fill_invalid=fill,
                                           median_radius=radius, median_sigma_color=12.0, median_sigma_space=4.0)
            got = pipe.process(tl, tr).disparity_map
            want = base.clone()
            if size:
                want = cd.filter_speckles(want, max_speckle_size=size, max_diff=0.5, invalid_disparity=-7.0)
            kw = dict(radius=radius, sigma_color=12.0, sigma_space=4.0, invalid_disparity=-7.0)
            if fill:
                want = cd.weighted_median(cd.fill_invalid(want, invalid_disparity=-7.0), guide, holes=want, **kw)
            else:
                want = cd.weighted_median(want, guide, **kw)
            assert_bitwise(got, want, f"lr {lr} size {size} fill {fill} radius {radius}")
            got2 = pipe.process(tl, tr).disparity_map                   # the buffers are reused
            assert_bitwise(got2, want, f"second frame, lr {lr} size {size} fill {fill}")
            tag = f"lr {lr} fill {fill}"
            assert_bitwise(pipe._stereo_matching._median_guide, guide, f"{tag}: the guide is the engine's gray plane")


def test_pipeline_u8_frames_use_the_same_guide(cd):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, dmin, dmax = 64, 128, 0, 31
    L, R = _pipeline_pair(H, W, dmin, dmax, seed=6)
    L8, R8 = np.clip(L, 0, 255).astype(np.uint8), np.clip(R, 0, 255).astype(np.uint8)
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=dmin, max_disparity=dmax,
                                        left_right_check=True)
    p8 = DepthEstimationPipeline(cfg, fill_invalid=True, median_radius=5)
    pf = DepthEstimationPipeline(cfg, fill_invalid=True, median_radius=5)
    got8 = p8.process(torch.from_numpy(L8).cuda(), torch.from_numpy(R8).cuda()).disparity_map
    gotf = pf.process(torch.from_numpy(L8.astype(np.float32)).cuda(),
                      torch.from_numpy(R8.astype(np.float32)).cuda()).disparity_map
    assert_bitwise(p8._stereo_matching._median_guide, pf._stereo_matching._median_guide, "u8 and f32 guides")
    assert_bitwise(got8, gotf, "u8 and f32 frames")


def test_pipeline_defaults_return_the_plain_map(cd):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, dmin, dmax = 64, 128, 8, 39
    L, R = _pipeline_pair(H, W, dmin, dmax)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    for lr in (False, True):
        cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=dmin, max_disparity=dmax,
                                            left_right_check=lr)
        pipe = DepthEstimationPipeline(cfg)
        got = pipe.process(tl, tr).disparity_map
        ecfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=2, min_disparity=dmin,
                                              max_disparity=dmax)
        sm = cd.StereoMatching(ecfg, max_batch=2)
        want = sm.compute_disparity_map_batch_lr(tl[None], tr[None])[0] if lr else sm.compute_disparity_map(tl, tr)
        assert_bitwise(got, want, f"defaults, lr {lr}")
        backend = pipe._stereo_matching
        assert backend._median_guide is None and backend._median_scratch is None    # nothing allocated or run
