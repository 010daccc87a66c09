"""Left-right consistency check on the device (include/stereo_mi355x.h: smx_compute_lr_*, smx_lr_check).

Every expected value comes from the CPU oracle and the NumPy twin of the rule (lr_ref.lr_rule):
  D_L = oracle(L, R),  D_R = flip(oracle(flip R, flip L)),  out = rule(D_L, D_R)
and is compared bit for bit.  The occlusion scene at the end is the one behavioural test (thresholds in its docstring)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stereo_synthetic as syn                      # noqa: E402
from oracle_lib import OracleConfig                 # noqa: E402
from parity_inputs import float_pair, odd_disparity_pair   # noqa: E402
from lr_ref import lr_rule                          # noqa: E402


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def flip(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a[..., ::-1])


def bits(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bitwise(got, expect, what):
    g, e = bits(got), bits(expect)
    bad = np.argwhere(g != e)
    assert bad.size == 0, f"{what}: {len(bad)} pixels differ, first at {tuple(bad[0])}"


def oracle_lr(oracle, ocfg, L, R, max_diff=1.0, invalid=-1.0):
    """(checked left map, right-view map) for one pair, from the oracle."""
    dl = oracle.run(ocfg, L, R)
    dr = flip(oracle.run(ocfg, flip(R), flip(L)))
    return lr_rule(dl, dr, max_diff, invalid), dr


# ----------------------------------------------------------------------------- 1. the standalone check
def _random_maps(rng, n, H, W):
    """Left maps with the rule's edge values sprinkled in, and right maps built so that roughly half of the pixels
    pass (D_R at the gathered position within +-1.5 of D_L)."""
    dl = rng.uniform(-2.0, 0.6 * W, (n, H, W)).astype(np.float32)
    specials = np.array([np.nan, np.inf, -np.inf, 0.5, -0.5, -0.6, 2.5, 1.5, 0.0, 3.0], np.float32)
    mask = rng.random((n, H, W)) < 0.15
    dl[mask] = rng.choice(specials, int(mask.sum()))
    dl[..., 0] = 0.0                                 # t == Y == 0
    dl[..., 1] = 1.5                                 # t == 2 > Y
    dr = rng.uniform(-2.0, 0.6 * W, (n, H, W)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        t = np.floor(dl + np.float32(0.5))
        Y = np.arange(W)
        ok = np.isfinite(t) & (t >= 0) & (t <= Y)
    yr = Y - np.where(ok, t, 0).astype(np.int64)
    near = (dl + rng.uniform(-1.5, 1.5, dl.shape).astype(np.float32)).astype(np.float32)
    for i, x, y in np.argwhere(ok & (rng.random(dl.shape) < 0.7)):
        dr[i, x, yr[i, x, y]] = near[i, x, y]
    exact = np.argwhere(ok)[:: 7]                    # |diff| == max_diff exactly
    for i, x, y in exact:
        dr[i, x, yr[i, x, y]] = dl[i, x, y] - np.float32(1.0) if np.isfinite(dl[i, x, y]) else dr[i, x, yr[i, x, y]]
    dr[rng.random(dr.shape) < 0.03] = np.nan
    return dl, dr


@pytest.mark.parametrize("n,H,W", [(3, 5, 37), (2, 4, 64), (1, 2, 4500)])    # odd W / float4 rows / wider than the LDS row
def test_standalone_check_matches_the_rule(cd, n, H, W):
    rng = np.random.default_rng(W)
    dl, dr = _random_maps(rng, n, H, W)
    expect = lr_rule(dl, dr, 1.0, -1.0)
    tl, tr = torch.from_numpy(dl).cuda(), torch.from_numpy(dr).cuda()
    assert_bitwise(cd.left_right_check(tl, tr), expect, "out")
    assert_bitwise(cd.left_right_check(tl[0], tr[0], max_diff=0.25, invalid_disparity=-9.0),
                   lr_rule(dl[0], dr[0], 0.25, -9.0), "[H,W], other max_diff / marker")
    cd.left_right_check(tl, tr, out=tl)                                  # in place
    assert_bitwise(tl, expect, "in place")
    valid = np.isfinite(expect) & (expect != -1.0)
    assert 0.2 < valid.mean() < 0.9, valid.mean()                       # both outcomes are exercised


def test_standalone_check_rejects_bad_arguments(cd):
    t = torch.zeros((2, 4, 8), device="cuda")
    with pytest.raises(RuntimeError, match="same shape|one shape"):
        cd.left_right_check(t, t[0])
    with pytest.raises(RuntimeError, match="max_diff"):
        cd.left_right_check(t, t.clone(), max_diff=-1.0)
    with pytest.raises(RuntimeError, match="invalid_disparity"):
        cd.left_right_check(t, t.clone(), invalid_disparity=float("nan"))
    with pytest.raises(RuntimeError, match="must not overlap right_disp"):
        cd.left_right_check(t.clone(), t, out=t)                         # out == right_disp


# ----------------------------------------------------------------------------- 2. the four engine entries
def _engine(cd, H, W, K, dmin, dmax, max_batch, **kw):
    cfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=dmin, max_disparity=dmax)
    fp = kw.pop("fp_convention", "source")
    ocfg = OracleConfig(height=H, width=W, downscale_factor=K, min_disparity=dmin, max_disparity=dmax,
                        fp_convention=cd._native.FP_CONVENTIONS[fp])
    return cd.StereoMatching(cfg, max_batch=max_batch, fp_convention=fp, **kw), ocfg


# id, H, W, K, dmin, dmax, kind ("gray", "gray_u8", "float", "rgb", "rgb_u8"), extra engine options
ENTRY_CASES = [
    ("K2_gray_f32", 40, 64, 2, 0, 15, "gray", {}),                  # on the grid: AUTO -> fast kernel
    ("K1_gray_u8", 32, 48, 1, 0, 11, "gray_u8", {}),
    ("K4_W_not_multiple", 36, 50, 4, 0, 15, "gray", {}),             # W % K != 0
    ("K2_odd_W_u8", 34, 61, 2, 0, 15, "gray_u8", {}),                # W % K != 0
    ("K2_dmin_capture", 48, 96, 2, 16, 47, "gray", {}),              # min_disparity > 0: the capture route
    ("K2_offgrid_f32", 40, 72, 2, 0, 19, "float", {}),               # exact-order route
    ("K2_rgb_f32", 40, 64, 2, 0, 15, "rgb", {}),
    ("K2_rgb_u8", 40, 64, 2, 0, 15, "rgb_u8", {}),
    ("K2_rgb_fma_first_dmin", 40, 80, 2, 10, 33, "rgb", dict(fp_convention="fma_first")),
]


def _pair_inputs(kind, H, W, D, K, i, dmin=0):
    if kind == "float":
        return float_pair(H, W, D, seed=20 + i)
    if kind in ("rgb", "rgb_u8"):
        return syn.random_rgb_pair(H, W, D, K, 40 + i, dmin=dmin)
    if i % 2:
        return odd_disparity_pair(H, W, D, seed=30 + i)
    l, r, _ = syn.make_pair(H, W, D, K, 50 + i, dmin=dmin)
    return l, r


def _batch(kind, n, H, W, D, K, dmin=0):
    ls, rs = zip(*[_pair_inputs(kind, H, W, D, K, i, dmin) for i in range(n)])
    L, R = np.stack(ls).astype(np.float32), np.stack(rs).astype(np.float32)
    if kind.endswith("u8"):
        return L, R, torch.from_numpy(L.astype(np.uint8)).cuda(), torch.from_numpy(R.astype(np.uint8)).cuda()
    return L, R, torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()


@pytest.mark.parametrize("case", ENTRY_CASES, ids=[c[0] for c in ENTRY_CASES])
def test_lr_entries_match_oracle(cd, oracle_omp, case):
    _, H, W, K, dmin, dmax, kind, extra = case
    n = 2
    sm, ocfg = _engine(cd, H, W, K, dmin, dmax, 2 * n, **extra)
    L, R, tl, tr = _batch(kind, n, H, W, dmax + 1, K, dmin)
    right_out = torch.full((n, H, W), 7.0, device="cuda")
    out = sm.compute_disparity_map_batch_lr(tl, tr, right_out=right_out, max_diff=1.0, invalid_disparity=-1.0)
    out_np, rout_np = out.cpu().numpy(), right_out.cpu().numpy()
    for i in range(n):
        exp, dr = oracle_lr(oracle_omp, ocfg, L[i], R[i])
        assert_bitwise(rout_np[i], dr, f"right_out pair {i}")
        assert_bitwise(out_np[i], exp, f"out pair {i}")
    # right_out = NULL form, another max_diff / marker, caller's out
    out2 = torch.empty((n, H, W), device="cuda")
    sm.compute_disparity_map_batch_lr(tl, tr, out2, max_diff=0.5, invalid_disparity=-5.0)
    for i in range(n):
        exp, _ = oracle_lr(oracle_omp, ocfg, L[i], R[i], 0.5, -5.0)
        assert_bitwise(out2[i], exp, f"out (right_out NULL) pair {i}")


# ----------------------------------------------------------------------------- 3. batch sizes, errors
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("extra", [0, 1])
def test_batch_sizes(cd, oracle_omp, n, extra):
    H, W, K, D = 32, 56, 2, 16
    sm, ocfg = _engine(cd, H, W, K, 0, D - 1, 2 * n + extra)
    L, R, tl, tr = _batch("gray", n, H, W, D, K)
    out = sm.compute_disparity_map_batch_lr(tl, tr).cpu().numpy()
    for i in range(n):
        assert_bitwise(out[i], oracle_lr(oracle_omp, ocfg, L[i], R[i])[0], f"n={n} pair {i}")
    L2, R2, tl2, tr2 = _batch("gray", n + 1, H, W, D, K)
    with pytest.raises(RuntimeError, match=r"max_batch // 2"):
        sm.compute_disparity_map_batch_lr(tl2, tr2)


def test_engine_stream_and_argument_errors(cd):
    from cuda_depth import _native as N
    H, W = 32, 56
    sm, _ = _engine(cd, H, W, 2, 0, 15, 4)
    _, _, tl, tr = _batch("gray", 2, H, W, 16, 2)
    out = torch.empty((2, H, W), device="cuda")
    rc = N.LIB.smx_compute_lr_gray_batch(sm._handle, 2, tl.data_ptr(), tr.data_ptr(), out.data_ptr(), None,
                                         1.0, -1.0, N.STREAM_ENGINE)
    assert rc == -5 and "SMX_STREAM_ENGINE" in N.last_error()
    rc = N.LIB.smx_compute_lr_gray_batch(sm._handle, 3, tl.data_ptr(), tr.data_ptr(), out.data_ptr(), None,
                                         1.0, -1.0, None)
    assert rc == -1 and "mirrored problem" in N.last_error() and "2n = 6" in N.last_error()
    rc = N.LIB.smx_compute_lr_gray_batch(sm._handle, 2, tl.data_ptr(), tr.data_ptr(), tl.data_ptr(), None,
                                         1.0, -1.0, None)
    assert rc == -1 and "must not overlap" in N.last_error()
    rc = N.LIB.smx_compute_lr_gray_batch(sm._handle, 2, tl.data_ptr(), tr.data_ptr(), out.data_ptr(), out.data_ptr(),
                                         1.0, -1.0, None)
    assert rc == -1 and "must not overlap" in N.last_error()
    with pytest.raises(RuntimeError, match="max_diff"):
        sm.compute_disparity_map_batch_lr(tl, tr, max_diff=float("inf"))


# ----------------------------------------------------------------------------- 4. the mirrored half's intermediates
def test_wta_of_the_mirrored_pairs(cd, oracle_omp):
    from cuda_depth import _native as N
    H, W, K, D, n = 40, 64, 2, 16, 2
    sm, ocfg = _engine(cd, H, W, K, 0, D - 1, 2 * n)
    L, R, tl, tr = _batch("gray_u8", n, H, W, D, K)
    sm.compute_disparity_map_batch_lr(tl, tr)
    for i in range(n):
        _, im = oracle_omp.run(ocfg, flip(R[i]), flip(L[i]), intermediates=True)
        assert_bitwise(sm.intermediate(N.STAGE_WTA, n + i), im["wta"], f"mirrored WTA pair {i}")
        _, im_l = oracle_omp.run(ocfg, L[i], R[i], intermediates=True)
        assert_bitwise(sm.intermediate(N.STAGE_WTA, i), im_l["wta"], f"WTA pair {i}")


# ----------------------------------------------------------------------------- 5. no state leak
@pytest.mark.parametrize("kind", ["gray", "rgb_u8"])
def test_plain_calls_unchanged_by_lr_calls(cd, kind):
    H, W, K, D, n = 40, 64, 2, 16, 3
    sm, _ = _engine(cd, H, W, K, 0, D - 1, 2 * n)
    _, _, tl, tr = _batch(kind, n, H, W, D, K)
    before = sm.compute_disparity_map_batch(tl, tr).clone()
    single = (sm.compute_disparity_map_gray(tl[0], tr[0]) if kind == "gray" else sm.compute_disparity_map(tl[0], tr[0])).clone()
    for _ in range(3):
        sm.compute_disparity_map_batch_lr(tl, tr)
    assert_bitwise(sm.compute_disparity_map_batch(tl, tr), before, "batch after LR calls")
    after = sm.compute_disparity_map_gray(tl[0], tr[0]) if kind == "gray" else sm.compute_disparity_map(tl[0], tr[0])
    assert_bitwise(after, single, "single after LR calls")
    # an LR call of a larger format regrows the scratch; the smaller format gives the same bits afterwards
    lr_before = sm.compute_disparity_map_batch_lr(tl, tr).clone()
    _, _, tlr, trr = _batch("rgb", 1, H, W, D, K)
    sm.compute_disparity_map_batch_lr(tlr, trr)
    assert_bitwise(sm.compute_disparity_map_batch_lr(tl, tr), lr_before, "LR call after the scratch grew")


# ----------------------------------------------------------------------------- 6. an occlusion scene
def _occlusion_scene(H, W, d_bg, d_fg, y0, y1, x0, x1, seed=3):
    """A background plane at disparity d_bg and a nearer rectangle (columns [y0, y1), rows [x0, x1)) at d_fg, both with
    uint8-valued noise texture, rendered into both views; the right view is z-buffered (the rectangle hides the
    background behind it).  Left pixel (x, y) of a surface at disparity d shows up at right column y - d.
    Returns (left, right, occluded mask, X, Y)."""
    rng = np.random.default_rng(seed)
    bg = rng.integers(0, 256, (H, W + d_bg + 1)).astype(np.float32)
    fg = rng.integers(0, 256, (H, W + d_fg + 1)).astype(np.float32)
    Y = np.arange(W)[None, :].repeat(H, 0)
    X = np.arange(H)[:, None].repeat(W, 1)
    rows = (X >= x0) & (X < x1)
    in_rect_l = rows & (Y >= y0) & (Y < y1)
    left = np.where(in_rect_l, np.take_along_axis(fg, Y, 1), np.take_along_axis(bg, Y, 1))
    in_rect_r = rows & (Y + d_fg >= y0) & (Y + d_fg < y1)
    right = np.where(in_rect_r, np.take_along_axis(fg, Y + d_fg, 1), np.take_along_axis(bg, Y + d_bg, 1))
    # background pixels of the left view whose right-view position the rectangle covers
    occluded = rows & ~in_rect_l & (Y - d_bg + d_fg >= y0) & (Y - d_bg + d_fg < y1)
    return left.astype(np.float32), right.astype(np.float32), occluded, X, Y


def test_occlusion_scene(cd, oracle_omp):
    """Background at disparity 24, a rectangle at 40 (a 16-column occluded strip left of it), min_disparity 16, K = 2,
    max_diff 1.  Bitwise against the oracle + rule first; then the behaviour, with thresholds set from the first run on
    an MI355X (the same numbers as the CPU oracle: the map is bit-identical) and kept well below it:
      * occluded strip: 0.896 invalid measured, >= 0.75 asserted (the remaining pixels lie within a window of the
        rectangle's edge, where the 21-wide aggregation windows of both views see the rectangle);
      * the band Y < min_disparity: every pixel is invalid except where D_L == 0.  The reference's vertical fill writes 0
        into the full-resolution rows of pooled row 0 below its first row (k_fill.h, x == 0), in both views, and a
        disparity of 0 points back to itself (0.990 of the band measured, row 1 being the exception);
      * background at least 24 columns from the rectangle's edges and from the band: 0.807 valid measured, >= 0.7
        asserted.  It is not ~1 because the map of a flat plane at K = 2 scatters by up to ~1.5 pixels around the truth
        (0.75 of those pixels are within 0.5), in both views: a few % then differ by more than max_diff."""
    H, W, K, dmin, dmax = 96, 192, 2, 16, 63
    d_bg, d_fg, y0, y1, x0, x1 = 24, 40, 100, 150, 24, 72
    L, R, occ, X, Y = _occlusion_scene(H, W, d_bg, d_fg, y0, y1, x0, x1)
    sm, ocfg = _engine(cd, H, W, K, dmin, dmax, 2)
    out = sm.compute_disparity_map_batch_lr(torch.from_numpy(L[None]).cuda(), torch.from_numpy(R[None]).cuda())[0]
    out = out.cpu().numpy()
    exp, _ = oracle_lr(oracle_omp, ocfg, L, R)
    assert_bitwise(out, exp, "scene")
    dl = oracle_omp.run(ocfg, L, R)
    invalid = out == np.float32(-1.0)
    occ_frac = invalid[occ].mean()
    rect_zone = (X >= x0 - 24) & (X < x1 + 24) & (Y >= y0 - (d_fg - d_bg) - 24) & (Y < y1 + 24)
    far_bg = ~rect_zone & (Y >= dmin + 24)
    bg_valid = (~invalid[far_bg]).mean()
    print(f"occlusion scene: occluded strip invalid {occ_frac:.3f}, band invalid {invalid[:, :dmin].mean():.3f}, "
          f"far background valid {bg_valid:.3f}")
    assert occ_frac >= 0.75, occ_frac
    assert (invalid[:, :dmin] | (dl[:, :dmin] == 0)).all()
    assert invalid[:, :dmin].mean() >= 0.95
    assert bg_valid >= 0.7, bg_valid


# ----------------------------------------------------------------------------- 7. the pipeline
def test_pipeline_left_right_check(cd, oracle_omp):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    from pipeline.point_cloud import disparity_to_depth_and_points
    H, W, dmin, dmax = 64, 128, 8, 39
    config = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=dmin, max_disparity=dmax,
                                           invalid_disparity=-7.0, left_right_check=True, lr_max_diff=1.0)
    pipe = DepthEstimationPipeline(config)
    L, R = syn.random_rgb_pair(H, W, dmax + 1, 2, 5, dmin=dmin)
    res = pipe.process(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())
    ocfg = OracleConfig(height=H, width=W, downscale_factor=2, min_disparity=dmin, max_disparity=dmax)
    exp, _ = oracle_lr(oracle_omp, ocfg, L, R, 1.0, -7.0)
    got = res.disparity_map.cpu().numpy()
    assert_bitwise(got, exp, "pipeline map")
    n_valid = int((exp != np.float32(-7.0)).sum())
    assert 0 < n_valid < H * W
    _, points = disparity_to_depth_and_points(res.disparity_map, 700.0, 0.5, config.invalid_disparity)
    assert points.shape[0] == n_valid
    # without the check the same pipeline returns the plain map (no invalid pixels)
    plain = DepthEstimationPipeline(DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=dmin,
                                                                  max_disparity=dmax, invalid_disparity=-7.0))
    assert_bitwise(plain.process(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()).disparity_map,
                   oracle_omp.run(ocfg, L, R), "pipeline without the check")
