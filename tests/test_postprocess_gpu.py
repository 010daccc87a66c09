"""Speckle filter and hole fill on the device (include/stereo_mi355x.h: smx_filter_speckles, smx_fill_invalid).

Region membership is unique, so the output does not depend on the labelling algorithm: every expected value comes from
the CPU reference (tests/postprocess_ref.py) and is compared bit for bit.  The injected-blob scene is the one behavioural
test."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import postprocess_ref as ref                       # noqa: E402
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


def check_both(cd, d, max_speckle_size, max_diff=1.0, invalid=-1.0, what=""):
    """filter_speckles and fill_invalid of d against the reference, out of place and in place."""
    t = torch.from_numpy(np.ascontiguousarray(d, np.float32)).cuda()
    exp_s = ref.filter_speckles(d, max_speckle_size, max_diff, invalid)
    got = cd.filter_speckles(t, max_speckle_size=max_speckle_size, max_diff=max_diff, invalid_disparity=invalid)
    assert_bitwise(got, exp_s, f"{what} speckles")
    exp_f = ref.fill_invalid(d, invalid)
    assert_bitwise(cd.fill_invalid(t, invalid_disparity=invalid), exp_f, f"{what} fill")
    assert_bitwise(t, d, f"{what} input untouched")
    t2 = t.clone()
    cd.filter_speckles(t2, max_speckle_size=max_speckle_size, max_diff=max_diff, invalid_disparity=invalid, out=t2)
    assert_bitwise(t2, exp_s, f"{what} speckles in place")
    cd.fill_invalid(t, invalid_disparity=invalid, out=t)
    assert_bitwise(t, exp_f, f"{what} fill in place")
    return exp_s


def random_map(rng, shape, invalid=-1.0, special_frac=0.15):
    """Integer levels plus a little noise, so that max_diff = 1 forms regions of many sizes, with the specials sprinkled
    in: NaN (with a payload), +-inf, the invalid value and -0.0."""
    d = (rng.integers(0, 5, shape) * 1.5 + rng.uniform(-0.3, 0.3, shape)).astype(np.float32)
    payload = np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]
    specials = np.array([np.nan, payload, np.inf, -np.inf, invalid, -0.0, 0.0], np.float32)
    mask = rng.random(shape) < special_frac
    d[mask] = rng.choice(specials, int(mask.sum()))
    return d


# ----------------------------------------------------------------------------- 1. random maps, sizes, limits
@pytest.mark.parametrize("n,H,W", [(1, 1, 1), (1, 1, 300), (1, 300, 1), (2, 37, 61), (1, 64, 64), (3, 33, 95),
                                   (1, 3, 5000)])
def test_random_maps(cd, n, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    d = random_map(rng, (n, H, W))
    for size in (0, 1, 3, 12, H * W):
        check_both(cd, d, size, what=f"{n}x{H}x{W} size {size}")
    check_both(cd, d[0], 5, max_diff=0.25, invalid=7.0, what="[H,W] map, other max_diff and marker")


def test_negative_zero_against_zero_marker(cd):
    rng = np.random.default_rng(5)
    d = random_map(rng, (2, 40, 70), invalid=0.0, special_frac=0.3)
    d[rng.random(d.shape) < 0.1] = -0.0
    exp = check_both(cd, d, 4, invalid=0.0, what="marker 0.0")
    assert (bits(exp) == np.float32(-0.0).view(np.uint32)).any()          # -0.0 copied as it is


# ----------------------------------------------------------------------------- 2. shapes that stress the labelling
def test_constant_map_is_one_region(cd):
    d = np.full((2, 150, 300), 3.25, np.float32)
    t = torch.from_numpy(d).cuda()
    assert_bitwise(cd.filter_speckles(t, max_speckle_size=150 * 300 - 1), d, "kept at size - 1")
    assert_bitwise(cd.filter_speckles(t, max_speckle_size=150 * 300), np.full_like(d, -1.0), "removed at size")


def test_checkerboard_every_pixel_its_own_region(cd):
    H, W = 70, 130
    d = np.where((np.arange(H)[:, None] + np.arange(W)[None]) % 2 == 0, 0.0, 10.0).astype(np.float32)
    t = torch.from_numpy(d).cuda()
    assert_bitwise(cd.filter_speckles(t, max_speckle_size=1), np.full_like(d, -1.0), "size 1 removed")
    check_both(cd, d, 0, what="checkerboard size 0")
    check_both(cd, d, 2, max_diff=20.0, what="checkerboard linked")


def serpentine(H, W, step):
    """A one-pixel-wide path of value 2 on a non-valid background: rows 0, step, 2 step, ... joined alternately at the
    right and the left edge.  Every row crosses every tile border; the joins cross the row-tile borders."""
    d = np.full((H, W), -1.0, np.float32)
    rows = list(range(0, H, step))
    for k, x in enumerate(rows):
        d[x] = 2.0
        if k + 1 < len(rows):
            y = W - 1 if k % 2 == 0 else 0
            d[x:rows[k + 1] + 1, y] = 2.0
    return d


def spiral(N):
    """A one-pixel-wide square spiral of value 4 from the corner inwards, one non-valid pixel between its arms."""
    d = np.full((N, N), -1.0, np.float32)
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    x = y = k = 0
    d[0, 0] = 4.0

    def free(i, j):
        return 0 <= i < N and 0 <= j < N and d[i, j] != 4.0

    while True:
        for _ in range(2):                                # straight on, else turn right once
            dx, dy = dirs[k]
            ahead2 = (x + 2 * dx, y + 2 * dy)
            if free(x + dx, y + dy) and (free(*ahead2) or not (0 <= ahead2[0] < N and 0 <= ahead2[1] < N)):
                x, y = x + dx, y + dy
                d[x, y] = 4.0
                break
            k = (k + 1) % 4
        else:
            return d


@pytest.mark.parametrize("case", ["serpentine", "serpentine_T", "spiral"])
def test_long_paths_across_tiles(cd, case):
    if case == "spiral":
        d = spiral(101)
    else:
        d = serpentine(97, 211, 3)
        if case == "serpentine_T":
            d = np.ascontiguousarray(d.T)
    sizes = ref.region_sizes(d, 1.0, -1.0)
    path = int(sizes.max())
    assert path > 1000 and (sizes[d == d.max()] == path).all(), "the path is one region"
    for size in (path - 1, path):
        check_both(cd, d, size, what=f"{case} size {size}")


def test_maps_do_not_join_across_boundaries(cd):
    """Map i's bottom row equals map i + 1's top row: linked if the maps were one image, separate regions here."""
    n, H, W = 4, 20, 50
    d = np.full((n, H, W), -1.0, np.float32)
    for i in range(n):
        d[i, 0] = 1.0                                     # top row: a region of W pixels
        d[i, H - 1] = 1.0                                 # bottom row: another one
    exp = check_both(cd, d, W, what="rows at the map edges")
    assert np.all(exp == -1.0)                            # joined across maps they would be 2W > W
    check_both(cd, d, W - 1, what="kept")


# ----------------------------------------------------------------------------- 3. workspace, graphs
def test_workspace_contents_do_not_matter(cd):
    from cuda_depth import _native as N
    rng = np.random.default_rng(11)
    n, H, W = 2, 45, 77
    d = random_map(rng, (n, H, W))
    t = torch.from_numpy(d).cuda()
    nbytes = int(N.LIB.smx_postprocess_workspace_bytes(n, H, W))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for _ in range(2):                                    # 0xFF first, then whatever the first call left
        o1, o2 = torch.empty_like(t), torch.empty_like(t)
        N.check(N.LIB.smx_filter_speckles(0, n, H, W, t.data_ptr(), o1.data_ptr(), 6, 1.0, -1.0, ws.data_ptr(), nbytes,
                                          stream))
        N.check(N.LIB.smx_fill_invalid(0, n, H, W, t.data_ptr(), o2.data_ptr(), -1.0, ws.data_ptr(), nbytes, stream))
        outs.append((o1, o2))
    for o1, o2 in outs:
        assert_bitwise(o1, ref.filter_speckles(d, 6), "speckles")
        assert_bitwise(o2, ref.fill_invalid(d), "fill")


def test_both_calls_inside_a_captured_graph(cd):
    from cuda_depth import _native as N
    rng = np.random.default_rng(12)
    n, H, W = 3, 64, 150
    d = random_map(rng, (n, H, W))
    t = torch.from_numpy(d).cuda()
    nbytes = int(N.LIB.smx_postprocess_workspace_bytes(n, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    mid, out = torch.empty_like(t), torch.empty_like(t)
    want = cd.fill_invalid(cd.filter_speckles(t, max_speckle_size=8)).clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        N.check(N.LIB.smx_filter_speckles(0, n, H, W, t.data_ptr(), mid.data_ptr(), 8, 1.0, -1.0, ws.data_ptr(), nbytes,
                                          cs))
        N.check(N.LIB.smx_fill_invalid(0, n, H, W, mid.data_ptr(), out.data_ptr(), -1.0, ws.data_ptr(), nbytes, cs))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert_bitwise(out, ref.fill_invalid(ref.filter_speckles(d, 8)), "replay")


def test_python_entries_reject_bad_tensors(cd):
    t = torch.zeros((2, 4, 8), device="cuda")
    with pytest.raises(RuntimeError, match="float32"):
        cd.filter_speckles(t.double(), max_speckle_size=2)
    with pytest.raises(RuntimeError, match=r"\[H,W\] or \[n,H,W\]"):
        cd.fill_invalid(t[None])
    with pytest.raises(RuntimeError, match="out must be float32"):
        cd.fill_invalid(t, out=t[0])
    buf = torch.zeros(2 * 4 * 8 + 4, device="cuda")
    with pytest.raises(RuntimeError, match="other than as the same buffer"):
        cd.filter_speckles(buf[:64].view(2, 4, 8), max_speckle_size=2, out=buf[4:].view(2, 4, 8))


# ----------------------------------------------------------------------------- 4. end to end, behaviour, pipeline
@pytest.mark.skipif(not os.path.exists(REAL), reason="tests/golden/real/real_crop_c2.npz not present")
def test_real_crop_lr_then_speckles_then_fill(cd):
    z = np.load(REAL)
    L, R = z["left_rgb"].astype(np.float32), z["right_rgb"].astype(np.float32)
    dmin, dmax = (int(v) for v in z["disparity_range"])
    H, W = L.shape[1:]
    cfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=2, min_disparity=dmin, max_disparity=dmax)
    sm = cd.StereoMatching(cfg, max_batch=2)
    lr = sm.compute_disparity_map_batch_lr(torch.from_numpy(L[None]).cuda(), torch.from_numpy(R[None]).cuda())[0]
    lr_host = lr.cpu().numpy()
    spk = cd.filter_speckles(lr, max_speckle_size=100, max_diff=1.0)
    filled = cd.fill_invalid(spk)
    exp_spk = ref.filter_speckles(lr_host, 100, 1.0, -1.0)
    assert_bitwise(spk, exp_spk, "real crop speckles")
    assert_bitwise(filled, ref.fill_invalid(exp_spk), "real crop fill")
    removed = int(((lr_host != -1.0) & (exp_spk == -1.0)).sum())
    print(f"real crop: {int((lr_host == -1.0).sum())} pixels invalid after the LR check, {removed} more removed as "
          f"speckles, {int((bits(filled) == np.float32(-1.0).view(np.uint32)).sum())} left invalid after the fill")
    assert removed > 0 and bool(torch.isfinite(filled).all()) and not bool((filled == -1.0).any())


def test_injected_blobs_are_removed_and_surfaces_kept(cd):
    """A synthetic scene's LR-checked map with blobs of 1, 4, 9 and 20 pixels at disparities far from their
    surroundings: the filter at 20 removes every blob pixel and keeps every pixel of every region above 20 pixels
    (the large surfaces); the fill then leaves no invalid pixel."""
    H, W, D, K = 96, 192, 32, 2
    l, r, _ = syn.make_pair(H, W, D, K, 3)
    cfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
    sm = cd.StereoMatching(cfg, max_batch=2)
    lr = sm.compute_disparity_map_batch_lr(torch.from_numpy(l[None]).cuda(), torch.from_numpy(r[None]).cuda())[0]
    d = lr.cpu().numpy().copy()
    blobs = [(10, 60, 1, 1), (30, 100, 2, 2), (60, 40, 3, 3), (75, 150, 4, 5)]
    blob_mask = np.zeros((H, W), bool)
    for x, y, h, w in blobs:
        d[x - 1:x + h + 1, y - 1:y + w + 1] = -1.0                        # a non-valid moat around each blob
        d[x:x + h, y:y + w] = 200.0
        blob_mask[x:x + h, y:y + w] = True
    sizes = ref.region_sizes(d, 1.0, -1.0)
    t = torch.from_numpy(d).cuda()
    out = cd.filter_speckles(t, max_speckle_size=20)
    got = out.cpu().numpy()
    assert_bitwise(got, ref.filter_speckles(d, 20), "scene")
    assert np.all(got[blob_mask] == -1.0)
    big = sizes > 20
    assert big.sum() > 0.5 * H * W, big.mean()
    assert_bitwise(got[big], d[big], "large surfaces kept")
    filled = cd.fill_invalid(out)
    assert not bool((filled == -1.0).any())


def _pipeline_pair(H, W, dmin, dmax, seed=5):
    return syn.random_rgb_pair(H, W, dmax + 1, 2, seed, dmin=dmin)


def test_pipeline_options_equal_the_standalone_chain(cd):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, dmin, dmax = 64, 128, 8, 39
    L, R = _pipeline_pair(H, W, dmin, dmax)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    cfg = dict(image_shape=(H, W), min_disparity=dmin, max_disparity=dmax, invalid_disparity=-7.0)
    lr_map = DepthEstimationPipeline(DepthEstimationPipelineConfig(**cfg, left_right_check=True)).process(
        tl, tr).disparity_map.clone()
    for lr in (True, False):
        base = lr_map if lr else DepthEstimationPipeline(DepthEstimationPipelineConfig(**cfg)).process(
            tl, tr).disparity_map.clone()
        for size, fill in ((10, False), (0, True), (10, True)):
            pipe = DepthEstimationPipeline(DepthEstimationPipelineConfig(**cfg, left_right_check=lr),
                                           speckle_max_size=size, speckle_max_diff=0.5, fill_invalid=fill)
            got = pipe.process(tl, tr).disparity_map
            want = base.clone()
            if size:
                want = cd.filter_speckles(want, max_speckle_size=size, max_diff=0.5, invalid_disparity=-7.0)
            if fill:
                want = cd.fill_invalid(want, invalid_disparity=-7.0)
            assert_bitwise(got, want, f"lr {lr} size {size} fill {fill}")
            got2 = pipe.process(tl, tr).disparity_map                     # the workspace is reused
            assert_bitwise(got2, want, f"second frame, lr {lr} size {size} fill {fill}")


def test_pipeline_defaults_return_the_plain_map(cd, oracle_omp):
    from oracle_lib import OracleConfig
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, dmin, dmax = 64, 128, 8, 39
    L, R = _pipeline_pair(H, W, dmin, dmax)
    pipe = DepthEstimationPipeline(DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=dmin,
                                                                 max_disparity=dmax))
    got = pipe.process(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()).disparity_map
    ocfg = OracleConfig(height=H, width=W, downscale_factor=2, min_disparity=dmin, max_disparity=dmax)
    assert_bitwise(got, oracle_omp.run(ocfg, L, R), "pipeline with default options")
    assert pipe._stereo_matching._post_workspace is None                  # nothing was allocated or run
