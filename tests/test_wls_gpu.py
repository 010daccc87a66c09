"""Image-guided weighted least squares filter on the device (include/stereo_mi355x.h: smx_wls_filter).

The rule is a fixed sequence of float32 operations, so every expected map comes from the CPU reference
(tests/wls_ref.py) and is compared bit for bit, whatever the kernels' split of the work."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import postprocess_ref as post                      # noqa: E402
import stereo_synthetic as syn                      # noqa: E402
import wls_ref as ref                               # noqa: E402

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


def run(d, g, lam, rw, conf=None, out=None, min_weight=1e-3, invalid=-1.0, workspace=None, stream=None):
    """smx_wls_filter through the C ABI on device tensors; returns out."""
    from cuda_depth import _native as N
    n = 1 if d.dim() == 2 else int(d.shape[0])
    H, W = int(d.shape[-2]), int(d.shape[-1])
    if out is None:
        out = torch.empty_like(d)
    if workspace is None:
        workspace = torch.empty(int(N.LIB.smx_wls_workspace_bytes(n, H, W)), dtype=torch.uint8, device="cuda")
    lam, rw = np.ascontiguousarray(lam, np.float32), np.ascontiguousarray(rw, np.float32)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    N.check(N.LIB.smx_wls_filter(0, n, H, W, d.data_ptr(), None if conf is None else conf.data_ptr(), g.data_ptr(),
                                 out.data_ptr(), int(lam.size), lam.ctypes.data, rw.ctypes.data, min_weight, invalid,
                                 workspace.data_ptr(), workspace.numel(), s))
    return out


def random_map(rng, shape, invalid=-1.0, special_frac=0.15, invalid_frac=0.25):
    d = (rng.integers(0, 6, shape) * 4.0 + rng.uniform(-0.5, 0.5, shape)).astype(np.float32)
    d[rng.random(shape) < invalid_frac] = invalid
    payload = np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]
    specials = np.array([np.nan, payload, np.inf, -np.inf, invalid, -0.0, 0.0], np.float32)
    mask = rng.random(shape) < special_frac
    d[mask] = rng.choice(specials, int(mask.sum()))
    return d


def random_guide(rng, shape, nan_frac=0.0):
    g = (rng.integers(0, 8, shape) * 20.0 + rng.uniform(0, 3, shape)).astype(np.float32)
    g[rng.random(shape) < nan_frac] = np.nan
    return g


def random_conf(rng, shape):
    c = rng.uniform(-0.3, 1.3, shape).astype(np.float32)
    c[rng.random(shape) < 0.05] = np.nan
    c[rng.random(shape) < 0.02] = np.inf
    return c


def tables(T, lam0=500.0, sigma=4.0):
    lam = np.array([lam0 * 0.25 ** t for t in range(T)], np.float64).astype(np.float32)
    rw = np.exp(-np.arange(256) / sigma).astype(np.float32)
    return lam, rw


# ----------------------------------------------------------------------------- 1. shapes, iterations, confidence
@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("n,H,W", [(1, 1, 1), (1, 1, 300), (1, 300, 1), (1, 37, 61), (3, 33, 95), (1, 64, 65),
                                   (2, 70, 129)])
def test_random_maps(cd, T, n, H, W):
    rng = np.random.default_rng(T * 100000 + H * 1000 + W)
    d = random_map(rng, (n, H, W))
    g = random_guide(rng, (n, H, W), nan_frac=0.02)
    lam, rw = tables(T)
    td, tg = dev(d), dev(g)
    assert_bitwise(run(td, tg, lam, rw), ref.wls_filter(d, g, lam, rw), "NULL confidence")
    c = random_conf(rng, (n, H, W))
    assert_bitwise(run(td, tg, lam, rw, conf=dev(c), min_weight=0.0),
                   ref.wls_filter(d, g, lam, rw, confidence=c, min_weight=0.0), "soft confidence")
    assert_bitwise(td, d, "in untouched")


def test_full_c2_map(cd):
    rng = np.random.default_rng(11)
    H, W = 375, 1242
    d = random_map(rng, (H, W), special_frac=0.02, invalid_frac=0.3)
    g = random_guide(rng, (H, W))
    lam, rw = tables(3, 8000.0, 1.5)
    assert_bitwise(run(dev(d), dev(g), lam, rw), ref.wls_filter(d, g, lam, rw), "C2 map")


def test_large_lambda_and_denormals(cd):
    H, W = 40, 300
    d = np.full((H, W), -1.0, np.float32)
    d[20, 0] = 10.0
    g = np.zeros((H, W), np.float32)
    rw = np.full(256, 0.01, np.float32)
    lam1 = np.array([1.0], np.float32)
    exp = ref.wls_filter(d, g, lam1, rw, min_weight=0.0)
    assert_bitwise(run(dev(d), dev(g), lam1, rw, min_weight=0.0), exp, "denormal decay")
    rng = np.random.default_rng(12)
    d2 = random_map(rng, (H, W), special_frac=0.0)
    lam2 = np.array([2.0 ** 20, 2.0 ** 18], np.float32)
    ones = np.ones(256, np.float32)
    assert_bitwise(run(dev(d2), dev(g), lam2, ones), ref.wls_filter(d2, g, lam2, ones), "lambda 2^20, weights 1")


def test_lambda_zero_and_other_marker(cd):
    rng = np.random.default_rng(13)
    d = random_map(rng, (50, 70), invalid=0.0, special_frac=0.3)
    g = random_guide(rng, (50, 70))
    lam, rw = np.zeros(2, np.float32), np.ones(256, np.float32)
    got = run(dev(d), dev(g), lam, rw, invalid=0.0)
    assert_bitwise(got, ref.wls_filter(d, g, lam, rw, invalid_disparity=0.0), "lambda 0")


def test_maps_are_independent(cd):
    rng = np.random.default_rng(14)
    n, H, W = 4, 23, 77
    d = random_map(rng, (n, H, W))
    g = random_guide(rng, (n, H, W))
    lam, rw = tables(3)
    batch = run(dev(d), dev(g), lam, rw)
    for i in range(n):
        assert_bitwise(batch[i], run(dev(d[i]), dev(g[i]), lam, rw), f"map {i} alone")


# ----------------------------------------------------------------------------- 2. aliasing, workspace, streams, graphs
def test_out_is_in_and_inputs_alias(cd):
    rng = np.random.default_rng(15)
    d = random_map(rng, (2, 45, 77))
    g = random_guide(rng, d.shape)
    lam, rw = tables(3)
    td = dev(d)
    run(td, dev(g), lam, rw, out=td)
    assert_bitwise(td, ref.wls_filter(d, g, lam, rw), "out == in")
    tg = dev(g)
    got = run(tg, tg, lam, rw, conf=tg, min_weight=0.0)
    assert_bitwise(got, ref.wls_filter(g, g, lam, rw, confidence=g, min_weight=0.0), "in == confidence == guide")


def test_workspace_contents_do_not_matter(cd):
    rng = np.random.default_rng(16)
    d = random_map(rng, (2, 40, 66))
    g = random_guide(rng, d.shape)
    lam, rw = tables(2)
    from cuda_depth import _native as N
    nbytes = int(N.LIB.smx_wls_workspace_bytes(2, 40, 66)) + 4096
    for fill in (0xFF, 0x7F):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        assert_bitwise(run(dev(d), dev(g), lam, rw, workspace=ws), ref.wls_filter(d, g, lam, rw), "garbage workspace")


def test_side_stream(cd):
    rng = np.random.default_rng(17)
    d = random_map(rng, (2, 64, 150))
    g = random_guide(rng, d.shape)
    lam, rw = tables(3)
    td, tg = dev(d), dev(g)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = cd.wls_filter(td, tg, lam=500.0, sigma_color=4.0, iterations=3)
    s.synchronize()
    assert_bitwise(out, ref.wls_filter(d, g, lam, rw), "side stream")


def test_call_inside_a_captured_graph(cd):
    rng = np.random.default_rng(18)
    n, H, W = 3, 64, 150
    d, g = random_map(rng, (n, H, W)), random_guide(rng, (n, H, W))
    c = random_conf(rng, (n, H, W))
    lam, rw = tables(3)
    lam0, rw0 = lam.copy(), rw.copy()
    td, tg, tc = dev(d), dev(g), dev(c)
    out1, out2 = torch.empty_like(td), torch.empty_like(td)
    from cuda_depth import _native as N
    ws = torch.empty(int(N.LIB.smx_wls_workspace_bytes(n, H, W)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        run(td, tg, lam, rw, out=out1, workspace=ws, stream=cs)
        run(td, tg, lam, rw, conf=tc, out=out2, workspace=ws, stream=cs)
    lam[:] = 0                                                        # the tables were copied at capture
    rw[:] = 0
    out1.zero_()
    out2.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert_bitwise(out1, ref.wls_filter(d, g, lam0, rw0), "replay, NULL confidence")
    assert_bitwise(out2, ref.wls_filter(d, g, lam0, rw0, confidence=c), "replay, soft confidence")


def test_python_entry_rejects_bad_operands(cd):
    t = torch.zeros((2, 4, 8), device="cuda")
    g = torch.zeros((2, 4, 8), device="cuda")
    with pytest.raises(RuntimeError, match="float32"):
        cd.wls_filter(t.double(), g)
    with pytest.raises(RuntimeError, match="guide must be float32"):
        cd.wls_filter(t, g[0])
    with pytest.raises(RuntimeError, match="confidence must be float32"):
        cd.wls_filter(t, g, confidence=t.double())
    with pytest.raises(RuntimeError, match="out must not overlap confidence or guide"):
        cd.wls_filter(t, g, out=g)


# ----------------------------------------------------------------------------- 3. end to end, pipeline
@pytest.mark.skipif(not os.path.exists(REAL), reason="tests/golden/real/real_crop_c2.npz not present")
def test_real_crop_lr_speckles_wls(cd):
    z = np.load(REAL)
    L, R = z["left_rgb"].astype(np.float32), z["right_rgb"].astype(np.float32)
    dmin, dmax = (int(v) for v in z["disparity_range"])
    H, W = L.shape[1:]
    cfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=2, min_disparity=dmin, max_disparity=dmax)
    sm = cd.StereoMatching(cfg, max_batch=2)
    lr = sm.compute_disparity_map_batch_lr(torch.from_numpy(L[None]).cuda(), torch.from_numpy(R[None]).cuda())[0]
    guide = sm.intermediate(0, 0).clone()
    spk = cd.filter_speckles(lr, max_speckle_size=100, max_diff=1.0)
    got = cd.wls_filter(spk, guide)
    exp_spk = post.filter_speckles(lr.cpu().numpy(), 100, 1.0, -1.0)
    lam, rw = cd.wls_tables(8000.0, 1.5, 3, 0.25)
    exp = ref.wls_filter(exp_spk, guide.cpu().numpy(), lam, rw)
    assert_bitwise(spk, exp_spk, "real crop speckles")
    assert_bitwise(got, exp, "real crop wls")
    holes = int((exp_spk == -1.0).sum())
    left = int((exp == -1.0).sum())
    print(f"real crop: {holes} invalid pixels before the filter, {left} after")
    assert holes > 0 and left < holes


def _pipeline_pair(H, W, dmin, dmax, seed=5):
    return syn.random_rgb_pair(H, W, dmax + 1, 2, seed, dmin=dmin)


@pytest.mark.parametrize("backend", ["cuda", "sgm"])
def test_pipeline_option_equals_the_standalone_chain(cd, backend):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, dmin, dmax, inv = 64, 128, 8, 39, -7.0
    L, R = _pipeline_pair(H, W, dmin, dmax)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    for size, iters in ((0, 3), (10, 2)):
        cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=dmin, max_disparity=dmax,
                                            invalid_disparity=inv, stereo_matching_backend=backend,
                                            left_right_check=True)
        pipe = DepthEstimationPipeline(cfg, speckle_max_size=size, speckle_max_diff=0.5, wls_lambda=3000.0,
                                       wls_sigma_color=2.0, wls_iterations=iters)
        got = pipe.process(tl, tr).disparity_map.clone()
        # the same chain by hand
        if backend == "cuda":
            ecfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=2, min_disparity=dmin,
                                                  max_disparity=dmax)
            sm = cd.StereoMatching(ecfg, max_batch=2)
            base = sm.compute_disparity_map_batch_lr(tl[None], tr[None], invalid_disparity=inv)[0].clone()
            guide = sm.intermediate(0, 0).clone()
        else:
            sgm = cd.StereoSGM(dmin, dmax, lr_max_diff=1.0, invalid_disparity=inv)
            guide = torch.empty((H, W), dtype=torch.float32, device="cuda")
            base = sgm.compute(tl, tr, gray_out=guide)
        if size:
            base = cd.filter_speckles(base, max_speckle_size=size, max_diff=0.5, invalid_disparity=inv)
        want = cd.wls_filter(base, guide, lam=3000.0, sigma_color=2.0, iterations=iters, invalid_disparity=inv)
        assert_bitwise(got, want, f"{backend}: size {size} iterations {iters}")
        assert_bitwise(pipe._stereo_matching._median_guide, guide, f"{backend}: the guide is the matcher's gray plane")
        got2 = pipe.process(tl, tr).disparity_map                      # the buffers are reused
        assert_bitwise(got2, want, f"{backend}: second frame")


@pytest.mark.parametrize("backend", ["cuda", "sgm"])
def test_pipeline_defaults_return_the_plain_map(cd, backend):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, dmin, dmax = 64, 128, 8, 39
    L, R = _pipeline_pair(H, W, dmin, dmax)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=dmin, max_disparity=dmax,
                                        stereo_matching_backend=backend, left_right_check=True)
    pipe = DepthEstimationPipeline(cfg)
    got = pipe.process(tl, tr).disparity_map
    if backend == "cuda":
        ecfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=2, min_disparity=dmin,
                                              max_disparity=dmax)
        want = cd.StereoMatching(ecfg, max_batch=2).compute_disparity_map_batch_lr(tl[None], tr[None])[0]
    else:
        want = cd.StereoSGM(dmin, dmax, lr_max_diff=1.0).compute(tl, tr)
    assert_bitwise(got, want, f"{backend} defaults")
    backend_obj = pipe._stereo_matching
    assert backend_obj._median_guide is None and backend_obj._wls_workspace is None    # nothing allocated or run
