"""Rectification on the device (include/stereo_mi355x.h: smx_remap_pairs), bit for bit against the CPU reference
(tests/rectify_ref.py): random and smooth maps, int32 extremes, both borders, both dtypes, C = 1, 3 and 4, edge shapes,
batches, left-only calls, graph replay and a non-default stream.  Then the end-to-end checks: a synthetic pair warped
into raw frames through a distorted, rotated rig, rectified and matched, and the pipeline with rectification=."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import rectify_ref as ref                           # noqa: E402
import stereo_synthetic as syn                      # noqa: E402

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def assert_bitwise(got, expect, what):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    e = np.asarray(expect)
    assert g.dtype == e.dtype and g.shape == e.shape, (what, g.dtype, g.shape, e.dtype, e.shape)
    gb = g.view(np.uint32) if g.dtype == np.float32 else g
    eb = e.view(np.uint32) if e.dtype == np.float32 else e
    bad = np.argwhere(gb != eb)
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first at {tuple(bad[0])}"


def random_qmap(rng, Ho, Wo, Hi, Wi, extreme_frac=0.1):
    q = np.stack([rng.integers(-96, (Wi + 2) * 32, (Ho, Wo)), rng.integers(-96, (Hi + 2) * 32, (Ho, Wo))], -1)
    pick = rng.random((Ho, Wo, 2)) < extreme_frac
    q[pick] = rng.choice([I32_MIN, I32_MAX, I32_MIN + 1, I32_MAX - 31, -1, -33, 0, 31], int(pick.sum()))
    return q.astype(np.int32)


def smooth_qmap(Ho, Wo, Hi, Wi, seed):
    """A realistic map: a mildly distorted, rotated camera (cuda_depth.rectification_map + quantize_map)."""
    import cuda_depth
    rng = np.random.default_rng(seed)
    K = np.array([[0.9 * Wi, 0.0, Wi / 2 + rng.uniform(-3, 3)], [0.0, 0.9 * Wi, Hi / 2 + rng.uniform(-3, 3)], [0, 0, 1]])
    P = np.array([[0.85 * Wi, 0.0, Wo / 2], [0.0, 0.85 * Wi, Ho / 2], [0, 0, 1]])
    a = rng.uniform(-0.02, 0.02, 3)
    R = _rot(*a)
    D = [rng.uniform(-0.3, -0.1), rng.uniform(0.0, 0.1), 1e-3, -1e-3, 0.0]
    return cuda_depth.quantize_map(*cuda_depth.rectification_map(K, D, R, P, (Hi, Wi), (Ho, Wo)), (Hi, Wi))


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))


def random_images(rng, n, C, H, W, dtype):
    if dtype == np.uint8:
        return rng.integers(0, 256, (n, C, H, W)).astype(np.uint8)
    img = rng.uniform(-300, 300, (n, C, H, W)).astype(np.float32)
    pick = rng.random(img.shape) < 0.03
    payload = np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]
    img[pick] = rng.choice(np.array([np.nan, payload, np.inf, -np.inf, -0.0, 0.0], np.float32), int(pick.sum()))
    return img


def run(cd, L, R, qL, qR, border=0, bv=0.0, outs=None, stream=None):
    """smx_remap_pairs through the C ABI; R / qR None: left only.  Returns the output tensors."""
    from cuda_depth import _native as N
    n, C, Hi, Wi = L.shape
    Ho, Wo = qL.shape[:2]
    if outs is None:
        outs = (torch.empty((n, C, Ho, Wo), dtype=L.dtype, device="cuda"),
                None if R is None else torch.empty((n, C, Ho, Wo), dtype=L.dtype, device="cuda"))
    dt = N.DTYPE_U8 if L.dtype == torch.uint8 else N.DTYPE_F32
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    ptr = (lambda t: None if t is None else t.data_ptr())
    N.check(N.LIB.smx_remap_pairs(0, n, C, dt, Hi, Wi, Ho, Wo, ptr(L), ptr(R), ptr(qL), ptr(qR), ptr(outs[0]),
                                  ptr(outs[1]), border, bv, s))
    return outs


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ----------------------------------------------------------------------------- 1. bit for bit against the reference
SHAPES = [  # (n, C, Hi, Wi, Ho, Wo)
    (1, 1, 1, 1, 1, 1), (2, 3, 1, 37, 1, 41), (1, 4, 29, 1, 33, 1), (3, 3, 23, 45, 19, 53), (1, 1, 64, 64, 48, 80),
    (2, 4, 40, 70, 37, 66), (1, 3, 17, 13, 31, 30), (5, 1, 8, 8, 9, 7),
]


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("border", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_random_maps_match_the_reference(cd, dtype, border, shape):
    n, C, Hi, Wi, Ho, Wo = shape
    rng = np.random.default_rng(hash((n, C, Hi, Wi, Ho, Wo, border, dtype == np.uint8)) % 2 ** 32)
    L, R = random_images(rng, n, C, Hi, Wi, dtype), random_images(rng, n, C, Hi, Wi, dtype)
    qL, qR = random_qmap(rng, Ho, Wo, Hi, Wi), random_qmap(rng, Ho, Wo, Hi, Wi)
    bv = 201.0 if dtype == np.uint8 else -3.75
    tL, tR = dev(L), dev(R)
    lo, ro = run(cd, tL, tR, dev(qL), dev(qR), border, bv)
    assert_bitwise(lo, ref.remap(L, qL, border, bv), f"left {shape}")
    assert_bitwise(ro, ref.remap(R, qR, border, bv), f"right {shape}")
    assert_bitwise(tL, L, "left input untouched")


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("border", [0, 1])
def test_smooth_maps_match_the_reference(cd, dtype, border):
    rng = np.random.default_rng(11 + border)
    Hi, Wi, Ho, Wo, n, C = 96, 160, 90, 150, 3, 3
    L, R = random_images(rng, n, C, Hi, Wi, dtype), random_images(rng, n, C, Hi, Wi, dtype)
    qL, qR = smooth_qmap(Ho, Wo, Hi, Wi, 1), smooth_qmap(Ho, Wo, Hi, Wi, 2)
    lo, ro = run(cd, dev(L), dev(R), dev(qL), dev(qR), border, 9.0)
    assert_bitwise(lo, ref.remap(L, qL, border, 9.0), "left")
    assert_bitwise(ro, ref.remap(R, qR, border, 9.0), "right")


def test_all_extreme_maps(cd):
    rng = np.random.default_rng(5)
    L = random_images(rng, 2, 3, 6, 9, np.uint8)
    q = random_qmap(rng, 12, 16, 6, 9, extreme_frac=1.0)
    for border in (0, 1):
        lo, ro = run(cd, dev(L), dev(L), dev(q), dev(q[::-1].copy()), border, 255.0)
        assert_bitwise(lo, ref.remap(L, q, border, 255), "left")
        assert_bitwise(ro, ref.remap(L, q[::-1].copy(), border, 255), "right")


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 17, 33, 64])
def test_batch_sizes(cd, n):
    rng = np.random.default_rng(100 + n)
    Hi, Wi, Ho, Wo = 20, 36, 18, 40
    L, R = random_images(rng, n, 3, Hi, Wi, np.uint8), random_images(rng, n, 3, Hi, Wi, np.uint8)
    qL, qR = smooth_qmap(Ho, Wo, Hi, Wi, n), random_qmap(rng, Ho, Wo, Hi, Wi)
    lo, ro = run(cd, dev(L), dev(R), dev(qL), dev(qR), 0, 0.0)
    assert_bitwise(lo, ref.remap(L, qL), f"left n={n}")
    assert_bitwise(ro, ref.remap(R, qR), f"right n={n}")


def test_left_only_and_unaligned_operands(cd):
    rng = np.random.default_rng(21)
    n, C, Hi, Wi, Ho, Wo = 2, 3, 15, 22, 12, 24
    L = random_images(rng, n, C, Hi, Wi, np.float32)
    q = random_qmap(rng, Ho, Wo, Hi, Wi)
    sentinel = torch.full((n, C, Ho, Wo), 123.0, device="cuda")
    (lo, _) = run(cd, dev(L), None, dev(q), None, 1, 0.0)
    assert_bitwise(lo, ref.remap(L, q, 1), "left only")
    assert_bitwise(sentinel, np.full((n, C, Ho, Wo), 123.0, np.float32), "nothing else written")
    # the map and the output one element off their allocation's alignment: the per-pixel path
    qbuf = torch.empty(q.size + 1, dtype=torch.int32, device="cuda")
    qbuf[1:] = dev(q.reshape(-1))
    obuf = torch.full((n * C * Ho * Wo + 2,), 7.0, device="cuda")
    out = obuf[1:-1].view(n, C, Ho, Wo)
    run(cd, dev(L), None, qbuf[1:].view(Ho, Wo, 2), None, 0, 2.0, outs=(out, None))
    assert_bitwise(out, ref.remap(L, q, 0, 2.0), "unaligned")
    assert float(obuf[0]) == 7.0 and float(obuf[-1]) == 7.0


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("Wo", [1242, 513, 259, 256, 255, 7, 2])
def test_row_widths_and_output_offsets(cd, dtype, Wo):
    """The dword / float4 stores for any width: rows of several waves whose start lies at every offset modulo 4
    elements (the width and the plane size move it from row to row and plane to plane, the output's offset in its
    buffer moves all of it), with guards around the output that must stay untouched."""
    rng = np.random.default_rng(Wo * 7 + (dtype == np.uint8))
    n, C, Hi, Wi, Ho = 3, 3, 23, 300, 5
    L, R = random_images(rng, n, C, Hi, Wi, dtype), random_images(rng, n, C, Hi, Wi, dtype)
    qL, qR = random_qmap(rng, Ho, Wo, Hi, Wi, 0.02), random_qmap(rng, Ho, Wo, Hi, Wi, 0.02)
    tdt = torch.uint8 if dtype == np.uint8 else torch.float32
    size = n * C * Ho * Wo
    for off in range(4):
        buf_l = torch.full((size + 8,), 77, dtype=tdt, device="cuda")
        buf_r = torch.full((size + 8,), 77, dtype=tdt, device="cuda")
        outs = (buf_l[off:off + size].view(n, C, Ho, Wo), buf_r[off:off + size].view(n, C, Ho, Wo))
        run(cd, dev(L), dev(R), dev(qL), dev(qR), 0, 5.0, outs=outs)
        assert_bitwise(outs[0], ref.remap(L, qL, 0, 5.0), f"left, offset {off}")
        assert_bitwise(outs[1], ref.remap(R, qR, 0, 5.0), f"right, offset {off}")
        for b in (buf_l, buf_r):
            guard = torch.cat([b[:off], b[off + size:]]).cpu().numpy()
            assert (guard == 77).all(), f"a guard element was written (offset {off})"


def test_graph_capture_and_replay(cd):
    rng = np.random.default_rng(31)
    n, C, Hi, Wi, Ho, Wo = 4, 3, 30, 50, 28, 48
    L, R = dev(random_images(rng, n, C, Hi, Wi, np.uint8)), dev(random_images(rng, n, C, Hi, Wi, np.uint8))
    qL, qR = smooth_qmap(Ho, Wo, Hi, Wi, 3), smooth_qmap(Ho, Wo, Hi, Wi, 4)
    rect = cd.StereoRectification(qL, qR, (Hi, Wi), (Ho, Wo))
    outs = (torch.empty((n, C, Ho, Wo), dtype=torch.uint8, device="cuda"),
            torch.empty((n, C, Ho, Wo), dtype=torch.uint8, device="cuda"))
    rect.rectify(L, R, out=outs)                                  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rect.rectify(L, R, out=outs)
    for k in range(2):
        Ln, Rn = random_images(rng, n, C, Hi, Wi, np.uint8), random_images(rng, n, C, Hi, Wi, np.uint8)
        L.copy_(dev(Ln))
        R.copy_(dev(Rn))
        outs[0].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert_bitwise(outs[0], ref.remap(Ln, qL), f"replay {k} left")
        assert_bitwise(outs[1], ref.remap(Rn, qR), f"replay {k} right")


def test_non_default_stream_ordering(cd):
    rng = np.random.default_rng(41)
    n, C, Hi, Wi, Ho, Wo = 8, 3, 200, 320, 180, 300
    Ln = random_images(rng, n, C, Hi, Wi, np.float32)
    q = smooth_qmap(Ho, Wo, Hi, Wi, 5)
    rect = cd.StereoRectification(q, q, (Hi, Wi), (Ho, Wo), border_mode="replicate")
    s = torch.cuda.Stream()
    L = torch.empty((n, C, Hi, Wi), device="cuda")
    with torch.cuda.stream(s):
        L.copy_(dev(Ln))                                          # producer, consumer and reader all on s
        lo, ro = rect.rectify(L, L)
        lo2 = lo * 1.0
    s.synchronize()
    expect = ref.remap(Ln, q, ref.REPLICATE)
    assert_bitwise(lo2, expect, "ordered on the stream")
    assert_bitwise(ro, expect, "right")


def test_python_wrapper_shapes_and_checks(cd):
    rng = np.random.default_rng(51)
    Hi, Wi, Ho, Wo = 21, 34, 20, 30
    q = random_qmap(rng, Ho, Wo, Hi, Wi)
    rect = cd.StereoRectification(q, q, (Hi, Wi), (Ho, Wo), border_value=17)
    L = random_images(rng, 1, 3, Hi, Wi, np.uint8)[0]
    lo, ro = rect.rectify(dev(L), dev(L))
    assert tuple(lo.shape) == (3, Ho, Wo) and lo.dtype == torch.uint8
    assert_bitwise(lo, ref.remap(L[None], q, 0, 17)[0], "single frame")
    assert_bitwise(rect.rectify(dev(L)), ref.remap(L[None], q, 0, 17)[0], "left only")
    np.testing.assert_array_equal(rect.left_valid.cpu().numpy(), ref.valid_mask(q, (Hi, Wi)))
    with pytest.raises(RuntimeError, match="in_shape"):
        rect.rectify(dev(L[:, :-1]), dev(L[:, :-1]))
    with pytest.raises(RuntimeError, match="right must be"):
        rect.rectify(dev(L), dev(L).float())
    with pytest.raises(RuntimeError, match="uint8 or float32"):
        rect.rectify(dev(L).int(), dev(L).int())
    with pytest.raises(RuntimeError, match="C in 1..4"):
        rect.rectify(dev(np.zeros((5, Hi, Wi), np.uint8)), dev(np.zeros((5, Hi, Wi), np.uint8)))
    with pytest.raises(RuntimeError, match="integer in 0..255"):
        cd.StereoRectification(q, q, (Hi, Wi), (Ho, Wo), border_value=0.5).rectify(dev(L), dev(L))
    with pytest.raises(RuntimeError, match="out"):
        rect.rectify(dev(L), dev(L), out=(torch.empty((3, Ho, Wo), dtype=torch.uint8, device="cuda"),
                                          torch.empty((3, Ho, Wo + 1), dtype=torch.uint8, device="cuda")))
    same = dev(L)
    square = cd.StereoRectification(random_qmap(rng, Hi, Wi, Hi, Wi), random_qmap(rng, Hi, Wi, Hi, Wi), (Hi, Wi),
                                    (Hi, Wi))
    with pytest.raises(RuntimeError, match="overlaps"):            # an output on top of an input, caught by the ABI
        square.rectify(same, dev(L), out=(same, torch.empty_like(same)))


# ----------------------------------------------------------------------------- 2. end to end
def _warp_to_raw(rect_img, K, D, R, P, raw_shape):
    """The raw frame of a camera whose rectified view is rect_img: each raw pixel is undistorted (fixed-point
    iteration), rotated and projected by P into the rectified image, which is sampled bilinearly in float64."""
    Hr, Wr = raw_shape
    v, u = np.mgrid[0:Hr, 0:Wr].astype(float)
    xd, yd = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    k1, k2, p1, p2, k3 = D
    x, y = xd.copy(), yd.copy()
    for _ in range(20):
        r2 = x * x + y * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        x = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / kr
        y = (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / kr
    X = np.einsum("ij,jhw->ihw", P @ R, np.stack([x, y, np.ones_like(x)]))
    su, sv = X[0] / X[2], X[1] / X[2]
    H, W = rect_img.shape
    u0, v0 = np.floor(su).astype(int), np.floor(sv).astype(int)
    au, av = su - u0, sv - v0
    out = np.zeros_like(su)
    for dy, dx, w in ((0, 0, (1 - au) * (1 - av)), (0, 1, au * (1 - av)), (1, 0, (1 - au) * av), (1, 1, au * av)):
        out += w * rect_img[np.clip(v0 + dy, 0, H - 1), np.clip(u0 + dx, 0, W - 1)]
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def _d1(disp, truth, margin, dmax):
    inner = (slice(margin, -margin), slice(margin + dmax, -margin))
    return float(np.mean(np.abs(disp[inner] - truth[inner]) > 3.0))


def test_rectify_then_match_keeps_d1(cd):
    H, W, D, K = 256, 448, 64, 2
    left, right, truth = syn.make_pair(H, W, D, K, 3)
    raw_shape = (H + 24, W + 40)
    P = np.array([[0.9 * W, 0.0, W / 2], [0.0, 0.9 * W, H / 2], [0, 0, 1]])
    cams = []
    for k, (ang, dist) in enumerate((((0.004, -0.006, 0.003), (-0.08, 0.02, 2e-4, -1e-4, 0.0)),
                                     ((-0.003, 0.005, -0.002), (-0.06, 0.01, -1e-4, 2e-4, 0.0)))):
        Kc = np.array([[0.92 * W, 0.0, raw_shape[1] / 2 + 1.5 * k], [0.0, 0.92 * W, raw_shape[0] / 2 - k], [0, 0, 1]])
        cams.append((Kc, np.array(dist), _rot(*ang), P))
    raw = [_warp_to_raw(img, *cam, raw_shape) for img, cam in zip((left, right), cams)]
    rect = cd.StereoRectification.from_calibration(cams[0], cams[1], raw_shape, (H, W))
    lo, ro = rect.rectify(dev(raw[0])[None], dev(raw[1])[None])
    cfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
    sm = cd.StereoMatching(cfg)
    d_rect = sm.compute_disparity_map_gray(lo[0], ro[0]).cpu().numpy()          # [1, H, W]: one gray plane
    d_orig = sm.compute_disparity_map_gray(dev(left), dev(right)).cpu().numpy()
    e_rect, e_orig = _d1(d_rect, truth, 16, D), _d1(d_orig, truth, 16, D)
    print(f"D1 (>3 px) on the interior: original pair {100 * e_orig:.2f} %, raw -> rectified {100 * e_rect:.2f} %")
    assert e_rect <= e_orig + 0.02, (e_rect, e_orig)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_pipeline_with_rectification(cd, dtype):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, dmin, dmax = 64, 128, 0, 31
    Hi, Wi = 72, 140
    L, R = syn.random_rgb_pair(H + 8, W + 12, dmax + 1, 2, 7)
    L, R = np.clip(L[:, :Hi, :Wi], 0, 255), np.clip(R[:, :Hi, :Wi], 0, 255)
    qL, qR = smooth_qmap(H, W, Hi, Wi, 8), smooth_qmap(H, W, Hi, Wi, 9)
    qL[..., 0] += 32 * 12                                         # the right columns of the left view reach past the frame
    rect = cd.StereoRectification(qL, qR, (Hi, Wi), (H, W))
    assert not rect.left_valid.all()                              # the map reaches outside the raw frame
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=dmin, max_disparity=dmax,
                                        invalid_disparity=-5.0)
    pipe = DepthEstimationPipeline(cfg, rectification=rect)
    tl = torch.from_numpy(np.ascontiguousarray(L).astype(np.uint8 if dtype == torch.uint8 else np.float32)).cuda()
    tr = torch.from_numpy(np.ascontiguousarray(R).astype(np.uint8 if dtype == torch.uint8 else np.float32)).cuda()
    res = pipe.process(tl, tr)
    got = res.disparity_map.clone()
    lo, ro = rect.rectify(tl, tr)
    assert_bitwise(res.left_image, lo.cpu().numpy(), "the result carries the rectified left frame")
    assert_bitwise(res.right_image, ro.cpu().numpy(), "the result carries the rectified right frame")
    plain = DepthEstimationPipeline(cfg).process(lo, ro).disparity_map.clone()
    want = torch.where(rect.left_valid, plain, torch.full_like(plain, -5.0))
    assert_bitwise(got, want.cpu().numpy(), f"pipeline {dtype}")
    assert (got[~rect.left_valid] == -5.0).all()
    got2 = pipe.process(tl, tr).disparity_map                     # persistent buffers reused
    assert_bitwise(got2, want.cpu().numpy(), "second frame")
