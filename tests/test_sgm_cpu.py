"""Semi-global matching without a GPU: the NumPy reference (tests/sgm_ref.py) against a plain per-pixel, per-path
loop implementation of the rule in include/stereo_mi355x.h, hand-computed cases, the quality of the rule on a synthetic
scene, every argument rejection of the C ABI, and the Python and pipeline keywords."""
import ctypes as C
import itertools

import numpy as np
import pytest

import sgm_ref as ref
import stereo_synthetic as syn

F = np.float32


# ---------------------------------------------------------------------------------------------------------- plain rule
def plain_census(g):
    H, W = g.shape
    out = np.zeros((H, W), np.uint64)
    for y in range(H):
        for x in range(W):
            bits, k = 0, 0
            for dy in range(-3, 4):
                for dx in range(-4, 5):
                    if dy == 0 and dx == 0:
                        continue
                    nb = g[min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)]
                    if nb < g[y, x]:
                        bits |= 1 << k
                    k += 1
            out[y, x] = bits
    return out


def plain_sgm(left, right, dmin, D, paths, P1, P2, uniqueness, lr, subpixel, invalid):
    with np.errstate(invalid="ignore"):
        cl, cr = plain_census(ref.gray(left)), plain_census(ref.gray(right))
    H, W = cl.shape

    def cost(y, x, i):
        xr = x - dmin - i
        return 64 if xr < 0 else bin(int(cl[y, x]) ^ int(cr[y, xr])).count("1")

    S = [[[0] * D for _ in range(W)] for _ in range(H)]
    for dy, dx in (ref.DIRECTIONS4 if paths == 4 else ref.DIRECTIONS8):
        for y in range(H):
            for x in range(W):
                # walk back to where the path enters the image, then forward to (y, x)
                sy, sx = y, x
                while 0 <= sy - dy < H and 0 <= sx - dx < W:
                    sy, sx = sy - dy, sx - dx
                L = [cost(sy, sx, i) for i in range(D)]
                while (sy, sx) != (y, x):
                    sy, sx = sy + dy, sx + dx
                    M = min(L)
                    new = []
                    for i in range(D):
                        cand = [L[i], M + P2]
                        if i > 0:
                            cand.append(L[i - 1] + P1)
                        if i < D - 1:
                            cand.append(L[i + 1] + P1)
                        new.append(cost(sy, sx, i) + min(cand) - M)
                    L = new
                assert max(L) <= 255
                for i in range(D):
                    S[y][x][i] += L[i]
    out = np.zeros((H, W), F)
    for y in range(H):
        for x in range(W):
            s = S[y][x]
            ist = min(range(D), key=lambda i: (s[i], i))
            d = dmin + ist
            bad = x - d < 0
            if uniqueness and any(s[i] * (100 - uniqueness) < s[ist] * 100 for i in range(D) if abs(i - ist) > 1):
                bad = True
            if lr >= 0 and not bad:
                xp = x - d
                cands = [(S[y][xp + dmin + i][i], i) for i in range(D) if xp + dmin + i <= W - 1]
                iR = min(cands)[1]
                if F(abs(dmin + iR - d)) > F(lr):
                    bad = True
            v = F(d)
            if subpixel and 0 < ist < D - 1:
                den = s[ist - 1] + s[ist + 1] - 2 * s[ist]
                if den > 0:
                    v = F(v + F(F(s[ist - 1] - s[ist + 1]) / F(2 * den)))
            out[y, x] = F(invalid) if bad else v
    return out


def small_pair(C_, H, W, dtype, seed, shift=2):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (C_, H, W + shift))
    left = base[..., shift:]
    right = np.clip(base[..., :W] + rng.integers(-2, 3, (C_, H, W)), 0, 255)
    if dtype == "u8":
        return left.astype(np.uint8), right.astype(np.uint8)
    return left.astype(F), right.astype(F)


CASES = [
    # (paths, D, dmin, P1, P2, uniqueness, lr, subpixel)
    (4, 1, 0, 10, 120, 0, -1.0, True),
    (8, 1, 2, 10, 120, 0, 0.0, False),
    (4, 2, 0, 0, 50, 10, -1.0, True),
    (8, 2, 1, 7, 7, 0, 1.0, True),
    (4, 5, 0, 0, 0, 0, -1.0, False),
    (8, 5, 0, 10, 191, 25, 0.0, True),
    (4, 5, 3, 191, 191, 0, 1.5, True),
    (8, 5, 1, 3, 120, 40, -1.0, True),
    (8, 5, 0, 20, 60, 0, -1.0, False),
]


@pytest.mark.parametrize("paths,D,dmin,P1,P2,uniqueness,lr,subpixel", CASES)
def test_reference_matches_plain_loops(paths, D, dmin, P1, P2, uniqueness, lr, subpixel):
    for k, (C_, dtype, H, W) in enumerate([(1, "u8", 5, 9), (3, "f32", 6, 7)]):
        left, right = small_pair(C_, H, W, dtype, 31 * D + k + paths)
        want = plain_sgm(left, right, dmin, D, paths, P1, P2, uniqueness, lr, subpixel, -2.0)
        got, _ = ref.sgm_ref(left, right, dmin, D, paths=paths, P1=P1, P2=P2, uniqueness=uniqueness, lr_max_diff=lr,
                             subpixel=subpixel, invalid_disparity=-2.0)
        assert np.array_equal(got, want), (k, np.argwhere(got != want)[:5])


def test_reference_matches_plain_loops_with_nan_and_inf():
    left, right = small_pair(3, 6, 8, "f32", 99)
    left[0, 1, 2], left[1, 3, 3], right[2, 2, 5], right[0, 4, 1] = np.nan, np.inf, -np.inf, np.nan
    want = plain_sgm(left, right, 0, 4, 8, 10, 120, 10, 1.0, True, -1.0)
    got, _ = ref.sgm_ref(left, right, 0, 4, paths=8, uniqueness=10, lr_max_diff=1.0)
    assert np.array_equal(got, want)


def test_hand_computed_row():
    """A 1x4 row, D = 2, P1 = 1, P2 = 3, 4 paths.  Costs are set directly on the recurrence."""
    Cv = np.array([[[0, 4], [5, 1], [2, 2], [6, 0]]], np.int32)            # [1, 4, 2]
    # left-to-right: L(0) = (0, 4); q = (0, 4), M = 0: L(1) = (5 + min(0, 4+1, 3), 1 + min(4, 0+1, 3)) - 0 = (5, 2)
    # M = 2: L(2) = (2 + min(5, 2+1, 5) - 2, 2 + min(2, 5+1, 5) - 2) = (3, 2); M = 2: L(3) = (6 + 3 - 2, 0 + 2 - 2) = (7, 0)
    assert ref.path_cost(Cv, (0, 1), 1, 3).tolist() == [[[0, 4], [5, 2], [3, 2], [7, 0]]]
    # right-to-left: L(3) = (6, 0); M = 0: L(2) = (2 + min(6, 1, 3), 2 + 0) = (3, 2); M = 2: L(1) = (5 + 3 - 2, 1 + 2 - 2)
    # = (6, 1); M = 1: L(0) = (0 + min(6, 2, 4) - 1, 4 + 1 - 1) = (1, 4)
    assert ref.path_cost(Cv, (0, -1), 1, 3).tolist() == [[[1, 4], [6, 1], [3, 2], [6, 0]]]
    # vertical paths on one row: every predecessor lies outside, L = C
    assert np.array_equal(ref.path_cost(Cv, (1, 0), 1, 3), Cv)
    S = ref.aggregate(Cv, 4, 1, 3)
    assert S.tolist() == [[[1, 16], [21, 5], [10, 8], [25, 0]]]            # L-> + L<- + 2 C
    # subpixel at x = 1..2 is not inner for D = 2: the values are the integer winners
    out = ref.select(S, 0, subpixel=True, invalid_disparity=-1.0)
    assert out.tolist() == [[0.0, 1.0, 1.0, 1.0]]


@pytest.mark.parametrize("H,W", [(1, 1), (2, 9), (7, 3)])
def test_census_clamps_into_small_images(H, W):
    rng = np.random.default_rng(H * 10 + W)
    g = rng.integers(0, 6, (H, W)).astype(F)
    assert np.array_equal(ref.census(g), plain_census(g))
    if H == W == 1:
        assert ref.census(g)[0, 0] == 0                                      # every neighbour is the centre


def test_census_nan_gives_zero_bits():
    g = np.arange(63, dtype=F).reshape(7, 9)
    g[3, 4] = np.nan                                                         # the centre of the middle pixel
    assert ref.census(g)[3, 4] == 0
    g2 = np.full((7, 9), 5.0, F)
    g2[0, 0] = np.nan
    assert ref.census(g2)[3, 4] == 0


def test_gray_is_the_engine_formula():
    import stereo_numpy
    rng = np.random.default_rng(4)
    rgb = rng.uniform(-5, 300, (3, 6, 7)).astype(F)
    assert np.array_equal(ref.gray(rgb), stereo_numpy.rgb_to_gray(rgb, conv=0))
    u8 = rng.integers(0, 256, (3, 4, 5)).astype(np.uint8)
    assert np.array_equal(ref.gray(u8), stereo_numpy.rgb_to_gray(u8.astype(F), conv=0))
    assert np.array_equal(ref.gray(u8[:1]), u8[0].astype(F))


# ------------------------------------------------------------------------------------------------------------- quality
def _left_truth(g):
    """g is indexed by right-image columns: gl(y, x) = the smallest d with g(y, (x - d) mod W) == d, -1 if none."""
    H, W = g.shape
    gl = np.full((H, W), -1, np.int64)
    for d in range(int(g.max()), -1, -1):
        hit = g[:, (np.arange(W) - d) % W] == d
        gl[hit] = d
    return gl


def test_quality_on_slanted_scene():
    left, right, g = syn.make_slanted_pair(120, 240, 32, 1)
    gl = _left_truth(g.astype(np.int64))
    score = gl >= 0
    score[:, :31] = False
    d, _ = ref.sgm_ref(left[None], right[None], 0, 32, paths=8)
    good = float(np.mean(np.abs(d - gl)[score] <= 1))
    raw = ref.wta_raw(left[None], right[None], 0, 32)
    good_raw = float(np.mean(np.abs(raw - gl)[score] <= 1))
    print(f"within 1 px: sgm 8 paths {good:.4f}, raw census WTA {good_raw:.4f}, scored {score[:, 31:].mean():.4f}")
    assert good >= 0.97
    assert good > good_raw


# -------------------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def nat():
    from cuda_depth import _native
    return _native


def _sgm_args(**over):
    a = dict(device_id=0, n=1, channels=3, dtype=0, H=8, W=16, left=0x10000, right=0x20000, min_disparity=0,
             num_disparities=8, paths=8, P1=10, P2=120, uniqueness=0, lr_max_diff=-1.0, subpixel=1,
             invalid_disparity=-1.0, out=0x40000, gray_left_out=None, workspace=0x100000, workspace_bytes=1 << 30,
             stream=None)
    a.update(over)
    return list(a.values())


REJECTIONS = [
    (dict(left=None), "must be non-NULL"),
    (dict(right=None), "must be non-NULL"),
    (dict(out=None), "must be non-NULL"),
    (dict(workspace=None), "must be non-NULL"),
    (dict(n=0), "need n >= 1"),
    (dict(H=0), "1 <= H, W <= 32768"),
    (dict(W=32769), "1 <= H, W <= 32768"),
    (dict(n=40000, H=32768, W=32768), "exceeds 2^31"),
    (dict(channels=2), "channels must be 1 or 3"),
    (dict(channels=4), "channels must be 1 or 3"),
    (dict(dtype=2), "unknown dtype"),
    (dict(min_disparity=-1), "min_disparity must be in 0..32768"),
    (dict(min_disparity=32769), "min_disparity must be in 0..32768"),
    (dict(num_disparities=0), "num_disparities must be in 1..256"),
    (dict(num_disparities=257), "num_disparities must be in 1..256"),
    (dict(paths=6), "paths must be 4 or 8"),
    (dict(P1=-1), "0 <= P1 <= P2 <= 191"),
    (dict(P1=50, P2=40), "0 <= P1 <= P2 <= 191"),
    (dict(P2=192), "0 <= P1 <= P2 <= 191"),
    (dict(uniqueness=-1), "uniqueness must be in 0..99"),
    (dict(uniqueness=100), "uniqueness must be in 0..99"),
    (dict(lr_max_diff=float("nan")), "lr_max_diff must be finite"),
    (dict(lr_max_diff=float("inf")), "lr_max_diff must be finite"),
    (dict(invalid_disparity=float("nan")), "invalid_disparity must be finite"),
    (dict(workspace_bytes=100), "is below smx_sgm_workspace_bytes"),
    (dict(out=0x10000 + 100), "must not overlap left, right or the workspace"),
    (dict(out=0x20000 + 100), "must not overlap left, right or the workspace"),
    (dict(out=0x100000 + 64), "must not overlap left, right or the workspace"),
    (dict(gray_left_out=0x20000 + 4), "must not overlap left, right or the workspace"),
    (dict(gray_left_out=0x40000 + 4), "out and gray_left_out overlap"),
    (dict(workspace=0x10000 - 256, workspace_bytes=1 << 20, out=0x10000000), "workspace must not overlap left or right"),
    (dict(workspace=0x100000 + 8), "workspace must be 256-byte aligned"),
    (dict(workspace=0x100000 + 128), "workspace must be 256-byte aligned"),
]


@pytest.mark.parametrize("over,msg", REJECTIONS, ids=[f"{i}-{m[:24]}" for i, (_, m) in enumerate(REJECTIONS)])
def test_c_abi_rejections(nat, over, msg):
    rc = nat.LIB.smx_sgm(*_sgm_args(**over))
    assert rc != nat.SMX_OK
    assert msg in nat.last_error(), nat.last_error()


def test_c_abi_rejects_the_engine_stream(nat):
    rc = nat.LIB.smx_sgm(*_sgm_args(stream=nat.STREAM_ENGINE))
    assert rc != nat.SMX_OK and "needs a caller stream" in nat.last_error()


def test_workspace_query_formula(nat):
    def R(v):
        return (v + 255) // 256 * 256

    for n, H, W, D, paths in itertools.product((1, 3), (1, 375), (1, 1242), (1, 63, 65, 128, 188, 256), (4, 8)):
        dp = D if D <= 64 else (D + 1) // 2 * 2 if D <= 128 else (D + 3) // 4 * 4
        P = n * H * W
        assert nat.LIB.smx_sgm_workspace_bytes(n, H, W, D, paths) == R(8 * P) * 2 + R(2 * dp * P) + R(2 * P)
    for bad in ((0, 8, 8, 8, 8), (1, 0, 8, 8, 8), (1, 8, 32769, 8, 8), (1, 8, 8, 0, 8), (1, 8, 8, 257, 8),
                (1, 8, 8, 8, 5), (40000, 32768, 32768, 8, 8)):
        assert nat.LIB.smx_sgm_workspace_bytes(*bad) == 0


# ------------------------------------------------------------------------------------------------- Python and pipeline
def test_stereo_sgm_arguments():
    import cuda_depth
    s = cuda_depth.StereoSGM()
    assert (s.min_disparity, s.max_disparity, s.num_disparities, s.paths, s.P1, s.P2) == (0, 127, 128, 8, 10, 120)
    assert s.uniqueness == 0 and s.lr_max_diff is None and s.subpixel is True and s.invalid_disparity == -1.0
    for kw, exc in ((dict(paths=5), RuntimeError), (dict(P1=20, P2=10), RuntimeError), (dict(P2=192), RuntimeError),
                    (dict(uniqueness=100), RuntimeError), (dict(lr_max_diff=-1.0), RuntimeError),
                    (dict(lr_max_diff=float("nan")), RuntimeError), (dict(invalid_disparity=float("inf")), RuntimeError),
                    (dict(paths=8.0), TypeError), (dict(subpixel=1), TypeError), (dict(lr_max_diff="1"), TypeError)):
        with pytest.raises(exc):
            cuda_depth.StereoSGM(**kw)
    with pytest.raises(RuntimeError):
        cuda_depth.StereoSGM(10, 9)
    with pytest.raises(RuntimeError):
        cuda_depth.StereoSGM(0, 256)
    with pytest.raises(RuntimeError):
        cuda_depth.StereoSGM(-1, 10)
    assert cuda_depth.StereoSGM(0, 255).num_disparities == 256
    with pytest.raises(TypeError):
        s.compute(np.zeros((1, 4, 4), np.uint8), np.zeros((1, 4, 4), np.uint8))


def test_pipeline_sgm_backend_and_keywords():
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    from pipeline.depth import AVAILABLE_DNN_BACKENDS, SgmStereoMatchingBackend
    assert AVAILABLE_DNN_BACKENDS == ("msnet2d", "msnet3d", "gwcnet")
    cfg = DepthEstimationPipelineConfig(image_shape=(40, 64), min_disparity=2, max_disparity=33,
                                        stereo_matching_backend="sgm", left_right_check=True, lr_max_diff=2.0)
    pipe = DepthEstimationPipeline(cfg, sgm_paths=4, sgm_p1=5, sgm_p2=60, sgm_uniqueness=7, speckle_max_size=10)
    be = pipe._stereo_matching
    assert isinstance(be, SgmStereoMatchingBackend)
    s = be._sgm
    assert (s.min_disparity, s.num_disparities, s.paths, s.P1, s.P2, s.uniqueness, s.lr_max_diff) == \
        (2, 32, 4, 5, 60, 7, 2.0)
    assert DepthEstimationPipeline(cfg.update(left_right_check=False))._stereo_matching._sgm.lr_max_diff is None
    for kw, exc in ((dict(sgm_paths=6), ValueError), (dict(sgm_p1=-1), ValueError), (dict(sgm_p1=9, sgm_p2=8), ValueError),
                    (dict(sgm_p2=192), ValueError), (dict(sgm_uniqueness=100), ValueError),
                    (dict(sgm_paths=8.0), TypeError), (dict(sgm_p1=True), TypeError)):
        with pytest.raises(exc):
            DepthEstimationPipeline(cfg, **kw)
        with pytest.raises(exc):                                # checked whatever the backend
            DepthEstimationPipeline(DepthEstimationPipelineConfig(stereo_matching_backend="msnet2d"), **kw)
    with pytest.raises(RuntimeError):                           # more than 256 candidates
        DepthEstimationPipeline(DepthEstimationPipelineConfig(stereo_matching_backend="sgm", max_disparity=400))
    with pytest.raises(TypeError):
        DepthEstimationPipeline(cfg, rectification="not a rectification")
    with pytest.raises(RuntimeError, match="gwcnet"):
        DepthEstimationPipeline(DepthEstimationPipelineConfig(stereo_matching_backend="gwcnet"))
