"""Semi-global matching on the device (include/stereo_mi355x.h: smx_sgm).

The rule is integer up to one float32 division, so every expected map comes from the CPU reference (tests/sgm_ref.py)
and is compared bit for bit, whatever the kernels' split of the work."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import median_ref                                   # noqa: E402
import postprocess_ref as post                      # noqa: E402
import rectify_ref                                  # noqa: E402
import sgm_ref as ref                               # noqa: E402
import stereo_synthetic as syn                      # noqa: E402


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def assert_same(got, expect, what):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    e = np.asarray(expect, np.float32)
    assert g.shape == e.shape, f"{what}: shape {g.shape} != {e.shape}"
    if not np.array_equal(g, e, equal_nan=True):
        bad = np.argwhere(~((g == e) | (np.isnan(g) & np.isnan(e))))
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first at {i}: got {g[i]!r}, expected {e[i]!r}")


def frames(n, C, H, W, dtype, seed, D=8, specials=False):
    """n pairs of [C,H,W] frames: a textured left view and a right view shifted by about D/2 with noise."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n, C, H, W + D)).astype(np.float64)
    base = (base + np.roll(base, 1, -1) + np.roll(base, 1, -2)) / 3             # some spatial correlation
    left = base[..., D // 2:D // 2 + W]
    right = np.clip(base[..., :W] + rng.integers(-3, 4, (n, C, H, W)), 0, 255)
    if dtype == "u8":
        return np.rint(left).astype(np.uint8), np.rint(right).astype(np.uint8)
    left, right = left.astype(np.float32), right.astype(np.float32)
    if specials:
        for img in (left, right):
            flat = img.reshape(-1)
            idx = rng.choice(flat.size, max(3, flat.size // 50), replace=False)
            flat[idx] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), idx.size)
    return left, right


def run(cd, left, right, dmin, D, gray=False, stream=None, **kw):
    sgm = cd.StereoSGM(dmin, dmin + D - 1, **kw)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    g = torch.empty(tl.shape[:-3] + tl.shape[-2:], dtype=torch.float32, device="cuda") if gray else None
    out = sgm.compute(tl, tr, gray_out=g)
    torch.cuda.synchronize()
    return (out, g) if gray else out


def expect(left, right, dmin, D, lr_max_diff=None, **kw):
    return ref.sgm_ref(left, right, dmin, D, lr_max_diff=-1.0 if lr_max_diff is None else lr_max_diff, **kw)


@pytest.mark.parametrize("dtype,C", [("u8", 1), ("u8", 3), ("f32", 1), ("f32", 3)])
@pytest.mark.parametrize("paths", [4, 8])
def test_inputs_and_paths(cd, dtype, C, paths):
    left, right = frames(1, C, 17, 23, dtype, 10 + C + paths, specials=dtype == "f32")
    want, gray = expect(left[0], right[0], 2, 12, paths=paths)
    got, g = run(cd, left[0], right[0], 2, 12, gray=True, paths=paths)
    assert_same(got, want, f"{dtype} C={C} paths={paths}")
    assert_same(g, gray, f"{dtype} C={C} gray_out")


@pytest.mark.parametrize("D", [1, 63, 64, 65, 128, 188, 256])
@pytest.mark.parametrize("dmin", [0, 5, 75])
def test_disparity_ranges(cd, D, dmin):
    left, right = frames(1, 1, 9, 120, "u8", D * 7 + dmin, D=16)
    want, _ = expect(left[0], right[0], dmin, D, uniqueness=10, lr_max_diff=1.0)
    assert_same(run(cd, left[0], right[0], dmin, D, uniqueness=10, lr_max_diff=1.0), want, f"D={D} dmin={dmin}")


@pytest.mark.parametrize("H,W", [(1, 1), (3, 300), (300, 3), (17, 23)])
@pytest.mark.parametrize("paths", [4, 8])
def test_shapes(cd, H, W, paths):
    left, right = frames(1, 3, H, W, "f32", H * 1000 + W)
    for dmin, D in ((0, 1), (0, 64), (1, 65)):
        want, _ = expect(left[0], right[0], dmin, D, paths=paths, lr_max_diff=0.0)
        assert_same(run(cd, left[0], right[0], dmin, D, paths=paths, lr_max_diff=0.0), want,
                    f"{H}x{W} D={D} dmin={dmin} paths={paths}")


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("uniqueness", [0, 15])
@pytest.mark.parametrize("lr", [None, 0.0, 1.5])
@pytest.mark.parametrize("subpixel", [False, True])
def test_options(cd, paths, uniqueness, lr, subpixel):
    left, right = frames(1, 1, 24, 60, "u8", 5, D=12)
    for P1, P2 in ((10, 120), (0, 0), (30, 30), (0, 191), (191, 191)):
        kw = dict(paths=paths, P1=P1, P2=P2, uniqueness=uniqueness, lr_max_diff=lr, subpixel=subpixel,
                  invalid_disparity=-3.5)
        want, _ = expect(left[0], right[0], 3, 20, **kw)
        assert_same(run(cd, left[0], right[0], 3, 20, **kw), want, f"{kw}")


@pytest.mark.parametrize("n", [3, 16])
def test_batches_are_independent(cd, n):
    left, right = frames(n, 3, 20, 50, "u8", 100 + n, D=10)
    want, gray = expect(left, right, 0, 24, uniqueness=5, lr_max_diff=1.0)
    got, g = run(cd, left, right, 0, 24, gray=True, uniqueness=5, lr_max_diff=1.0)
    assert_same(got, want, f"batch of {n}")
    assert_same(g, gray, f"batch of {n}: gray_out")
    for k in (0, n - 1):                                  # one pair alone gives the same map as inside the batch
        assert_same(run(cd, left[k], right[k], 0, 24, uniqueness=5, lr_max_diff=1.0), want[k], f"pair {k} alone")


def test_full_c2_frame(cd):
    l, r, _ = syn.make_slanted_pair(375, 1242, 128, 1)
    left, right = l.astype(np.uint8)[None], r.astype(np.uint8)[None]
    want, _ = expect(left, right, 0, 128, paths=8, uniqueness=10, lr_max_diff=1.0)
    assert_same(run(cd, left, right, 0, 128, paths=8, uniqueness=10, lr_max_diff=1.0), want, "C2 375x1242 D=128")


def test_workspace_contents_do_not_matter(cd):
    left, right = frames(2, 1, 30, 70, "f32", 77, specials=True)
    sgm = cd.StereoSGM(4, 40, lr_max_diff=1.0, uniqueness=20)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    ws = sgm.workspace(2, 30, 70, tl.device)
    ws.fill_(0xFF)
    a = sgm.compute(tl, tr).clone()
    ws.random_(0, 256)
    b = sgm.compute(tl, tr)
    want, _ = expect(left, right, 4, 37, lr_max_diff=1.0, uniqueness=20)
    assert_same(a, want, "0xFF workspace")
    assert_same(b, want, "random workspace")


def test_non_default_stream(cd):
    left, right = frames(4, 3, 40, 90, "u8", 3)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    sgm = cd.StereoSGM(0, 31, lr_max_diff=1.0)
    out = torch.full((4, 40, 90), 7.0, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sgm.compute(tl, tr, out=out)
    s.synchronize()
    want, _ = expect(left, right, 0, 32, lr_max_diff=1.0)
    assert_same(out, want, "side stream")


def test_graph_capture_and_replay(cd):
    left, right = frames(2, 3, 32, 80, "u8", 21)
    left2, right2 = frames(2, 3, 32, 80, "u8", 22)
    sgm = cd.StereoSGM(0, 47, paths=8, lr_max_diff=1.0, uniqueness=10)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    out = torch.empty((2, 32, 80), device="cuda")
    gray = torch.empty((2, 32, 80), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sgm.compute(tl, tr, out=out, gray_out=gray)        # warm-up: the workspace is allocated outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sgm.compute(tl, tr, out=out, gray_out=gray)
    for lft, rgt in ((left2, right2), (left, right)):
        tl.copy_(torch.from_numpy(lft))
        tr.copy_(torch.from_numpy(rgt))
        out.fill_(123.0)
        g.replay()
        torch.cuda.synchronize()
        want, wgray = expect(lft, rgt, 0, 48, paths=8, lr_max_diff=1.0, uniqueness=10)
        assert_same(out, want, "graph replay")
        assert_same(gray, wgray, "graph replay: gray_out")


def _qmap(H, W, Hi, Wi, seed):
    """A smooth int32 map of 1/32-pixel raw coordinates, slightly rotated and scaled (rectify_ref's format)."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a, s = rng.uniform(-0.01, 0.01), rng.uniform(0.97, 1.0)
    mx = s * (np.cos(a) * u - np.sin(a) * v) + rng.uniform(1, 3)
    my = s * (np.sin(a) * u + np.cos(a) * v) + rng.uniform(1, 3)
    return rectify_ref.quantize_map(mx, my, (Hi, Wi))


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_pipeline_sgm_chain(cd, dtype):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, dmin, dmax, inv = 48, 120, 2, 33, -2.0
    Hi, Wi = 54, 130
    L, R = syn.random_rgb_pair(Hi, Wi, 32, 1, 3)
    L, R = np.clip(L, 0, 255), np.clip(R, 0, 255)
    cast = (lambda a: np.rint(a).astype(np.uint8)) if dtype == "u8" else (lambda a: a.astype(np.float32))
    L, R = cast(L), cast(R)
    qL, qR = _qmap(H, W, Hi, Wi, 1), _qmap(H, W, Hi, Wi, 2)
    qL[..., 0] += 32 * 10                                         # the left view's right columns reach past the frame
    rect = cd.StereoRectification(qL, qR, (Hi, Wi), (H, W))
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=dmin, max_disparity=dmax,
                                        invalid_disparity=inv, stereo_matching_backend="sgm", left_right_check=True,
                                        lr_max_diff=1.0)
    pipe = DepthEstimationPipeline(cfg, speckle_max_size=20, speckle_max_diff=1.0, fill_invalid=True, median_radius=3,
                                   median_sigma_color=10.0, median_sigma_space=5.0, rectification=rect, sgm_paths=4,
                                   sgm_p1=8, sgm_p2=96, sgm_uniqueness=5)
    res = pipe.process(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())
    got = res.disparity_map.cpu().numpy()
    # the same chain from the references
    lo = rectify_ref.remap(L[None], qL)[0]
    ro = rectify_ref.remap(R[None], qR)[0]
    d, gray = ref.sgm_ref(lo, ro, dmin, dmax - dmin + 1, paths=4, P1=8, P2=96, uniqueness=5, lr_max_diff=1.0,
                          invalid_disparity=inv)
    d = post.filter_speckles(d, 20, 1.0, inv)
    filled = post.fill_invalid(d, inv)
    rw, sw = cd.median_weight_tables(3, 10.0, 5.0)
    d = median_ref.weighted_median(filled, gray, 3, rw, sw, holes=d, invalid_disparity=inv)
    d = np.where(rectify_ref.valid_mask(qL, (Hi, Wi)), d, np.float32(inv))
    assert_same(got, d, f"sgm pipeline chain ({dtype})")
    assert_same(res.left_image, lo, "the result carries the rectified left frame")
    got2 = pipe.process(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()).disparity_map
    assert_same(got2, d, "second frame, persistent buffers reused")
