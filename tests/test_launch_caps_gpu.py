"""The map entries past the caps of their launchers' grids, bit for bit against their NumPy references.

Every engine-free entry caps a grid dimension and strides over the rest ("grid-stride beyond" in the tu_*.hip launchers);
each of those loops carries a barrier or LDS state from one trip to the next.  The caps are crossed with many tiny maps.
The sizes are in tests/scale_cases.py, and tests/test_scale_geometry_cpu.py checks against the kernel sources that every
case still crosses its cap.

    case                              loop on a second trip
    test_confidence_past_the_map_cap  k_confidence: m += gridDim.y, with right and guide (three barriers a trip), and bare
    test_temporal_past_the_map_cap    k_temporal: m += gridDim.y over three frames, state planes and guide ping-pong
    test_sgm_past_the_census_and_selection_caps
                                      k_sgm_census: z += gridDim.y (left and right images); k_sgm_right_wta and
                                      k_sgm_select: p += waves
    test_sgm_wide_range_past_the_census_cap
                                      k_sgm_census again, ahead of the four-disparities-per-lane kernels
    test_median_past_the_tile_cap     k_median: tile += gridDim.x, whole-map mode and holes mode
    test_wls_past_the_line_caps       k_wls_rows: line0 += gridDim.x * WLS_LINES; k_wls_cols: line += gridDim.x * 64
                                      (maps of 1x2 and 2x1 past both caps, maps of 33x1 past the rows cap)
    test_rectification_past_the_chunk_cap
                                      k_remap: ipt > REMAP_IPT images per thread, a last chunk of one pair
    test_lr_pack_strides              k_lr_pack: straight halves in 16-byte chunks and in elements, mirrored halves
    test_mirrored_lr_check_on_rows_wider_than_lds
                                      k_lr_check<MIRRORED, no LDS>, float4 rows and scalar rows
    test_track_past_the_triple_cap    k_track_accum: f += gridDim.y, and k_track_solve: f += gridDim.x, three iterations
                                      at two strides, with a lost triple's `continue` between tracked ones

How 10^5 to 10^8 maps get a reference: TILE_PERIOD = 7 distinct maps (pairs, streams) drawn from the generators of the
entry's own test module, their expectation from the entry's reference, and map i of the call = distinct map i % 7, tiled
on the device.  Every output, state plane and workspace starts as a sentinel (a NaN payload no kernel produces), and all
elements are compared as bits.  Two conditions make a wrong trip visible, whichever map it lands on: the 7 expectations
differ pairwise (asserted here, on the reference data), and 7 divides none of the loop strides (asserted over the
strides that tests/test_scale_geometry_cpu.py computes from the sources).  A trip that skips a map leaves sentinels, one
that lands one map off writes another map's values."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import confidence_ref                               # noqa: E402
import median_ref                                   # noqa: E402
import rectify_ref                                  # noqa: E402
import scale_cases as sc                            # noqa: E402
import sgm_ref                                      # noqa: E402
import stereo_synthetic as syn                      # noqa: E402
import temporal_ref                                 # noqa: E402
import wls_ref                                      # noqa: E402
import test_confidence_gpu as t_conf                # noqa: E402  (the generators of each entry's own tests)
import test_median_gpu as t_med                     # noqa: E402
import test_rectify_gpu as t_rect                   # noqa: E402
import test_sgm_gpu as t_sgm                        # noqa: E402
import test_temporal_gpu as t_temp                  # noqa: E402
import test_track_gpu as t_track                    # noqa: E402
import test_wls_gpu as t_wls                        # noqa: E402
import track_cases as trk                           # noqa: E402
from lr_ref import lr_rule                          # noqa: E402
from oracle_lib import OracleConfig                 # noqa: E402

P = sc.TILE_PERIOD
SENTINEL_BITS = 0x7FD5A5A5                          # a quiet NaN with a payload: no kernel here produces it
SENTINEL_BYTE = 0xA5
INVALID = -1.0


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


# ---- tiling, sentinels and the comparison ------------------------------------------------------------------------------

def tile_dev(distinct, n):
    """[n, ...] on the device: element i is distinct[i % len(distinct)] (repeat plus a tail, without a temporary)."""
    b = torch.from_numpy(np.ascontiguousarray(distinct)).cuda()
    q, r = divmod(n, b.shape[0])
    out = torch.empty((n,) + tuple(b.shape[1:]), dtype=b.dtype, device="cuda")
    out[:q * b.shape[0]].view((q,) + tuple(b.shape)).copy_(b)
    out[q * b.shape[0]:].copy_(b[:r])
    return out


def sentinel(shape, dtype=torch.float32):
    if dtype == torch.uint8:
        return torch.full(shape, SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
    if dtype == torch.float64:                                   # the sentinel word twice: a NaN as a double too
        return torch.full(tuple(shape[:-1]) + (2 * shape[-1],), SENTINEL_BITS, dtype=torch.int32, device="cuda").view(dtype)
    words = torch.full(shape, SENTINEL_BITS, dtype=torch.int32, device="cuda")
    return words if dtype == torch.int32 else words.view(torch.float32)


def as_bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def assert_tiled(got, distinct_expected, what):
    """got[i] == distinct_expected[i % P] for every i, bit for bit, compared on the device."""
    exp = np.ascontiguousarray(distinct_expected)
    assert tuple(got.shape[1:]) == exp.shape[1:] and str(got.dtype).endswith(str(exp.dtype)), (what, got.shape, exp.shape)
    g, e = as_bits(got), as_bits(tile_dev(exp, got.shape[0]))
    if torch.equal(g, e):
        return
    bad = (g != e).reshape(g.shape[0], -1)
    flat = int(bad.reshape(-1).nonzero()[0])
    i, k = divmod(flat, bad.shape[1])
    gv, ev = int(g.reshape(g.shape[0], -1)[i, k]), int(e.reshape(g.shape[0], -1)[i, k])
    mark = {torch.uint8: SENTINEL_BYTE, torch.float64: SENTINEL_BITS << 32 | SENTINEL_BITS}.get(got.dtype, SENTINEL_BITS)
    marks, mask = int((g == mark).sum()), (1 << 8 * g.element_size()) - 1
    raise AssertionError(f"{what}: {int(bad.sum())} elements of {int(bad.any(1).sum())} maps differ, first at map {i} "
                         f"(distinct map {i % exp.shape[0]}) element {k}: got {gv & mask:#x}, expected "
                         f"{ev & mask:#x}; {marks} elements still hold the sentinel")


def assert_distinct(distinct_expected, what):
    """The tiling's first condition: the expectations of the distinct maps differ pairwise (as bits)."""
    rows = [np.ascontiguousarray(a).tobytes() for a in distinct_expected]
    assert len(rows) == P and len(set(rows)) == P, f"{what}: the {P} distinct expectations are not pairwise different"


def assert_bitwise(got, expect, what):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    g, e = np.ascontiguousarray(g, np.float32).view(np.uint32), np.ascontiguousarray(expect, np.float32).view(np.uint32)
    assert g.shape == e.shape, f"{what}: shape {g.shape} != {e.shape}"
    bad = np.argwhere(g != e)
    assert bad.size == 0, (f"{what}: {len(bad)} values differ, first at {tuple(bad[0])}: got {g[tuple(bad[0])]:#x}, "
                           f"expected {e[tuple(bad[0])]:#x}; {int((g == SENTINEL_BITS).sum())} hold the sentinel")


# ---- 1. confidence -------------------------------------------------------------------------------------------------------

CONF_PARAMS = dict(radius=sc.MAP_RADIUS, lr_scale=0.75, texture_scale=6.0)


def confidence_distinct():
    """The distinct (left, right, guide) maps and their expectations with both operands and with neither."""
    _, H, W = sc.CONF_CAP_SHAPE
    rng = np.random.default_rng(9001)
    d, r, g = t_conf.random_map(rng, (P, H, W)), t_conf.random_map(rng, (P, H, W)), t_conf.random_guide(rng, (P, H, W))
    # the generator's disparities (0..12) point outside rows of 5 pixels: fold the valid ones into -0.7..3, then make the
    # right-view map agree within the LR scale at most of the positions the left pixels point at
    with np.errstate(invalid="ignore"):
        d = np.where(median_ref.valid_mask(d, INVALID), np.fmod(d, np.float32(3.0)), d).astype(np.float32)
        t = np.floor(d + np.float32(0.5))
        ok = np.isfinite(t) & (t >= 0) & (t <= np.arange(W))
    for i, x, y in np.argwhere(ok & (rng.random(d.shape) < 0.8)):
        r[i, x, y - int(t[i, x, y])] = d[i, x, y] + np.float32(rng.uniform(-0.7, 0.7))
    full = confidence_ref.confidence_map(d, r, g, invalid_disparity=INVALID, **CONF_PARAMS)
    bare = confidence_ref.confidence_map(d, None, None, invalid_disparity=INVALID, **CONF_PARAMS)
    return d, r, g, full, bare


def test_confidence_past_the_map_cap(cd):
    n, H, W = sc.CONF_CAP_SHAPE
    d, r, g, full, bare = confidence_distinct()
    assert_distinct(full, "confidence with right and guide")
    assert_distinct(bare, "confidence without right and guide")
    assert np.isnan(d).any() and np.isnan(g).any(), "the distinct maps carry the specials"
    td, tr, tg = tile_dev(d, n), tile_dev(r, n), tile_dev(g, n)
    out = sentinel((n, H, W))
    cd.confidence_map(td, tr, tg, invalid_disparity=INVALID, out=out, **CONF_PARAMS)
    assert_tiled(out, full, "confidence with right and guide")
    out = sentinel((n, H, W))
    cd.confidence_map(td, invalid_disparity=INVALID, out=out)
    assert_tiled(out, bare, "confidence without right and guide")
    assert_tiled(td, d, "left untouched")


# ---- 2. temporal filter --------------------------------------------------------------------------------------------------

TEMP_PARAMS = dict(t_temp.PARAMS, motion_radius=sc.MAP_RADIUS)


def temporal_distinct():
    """The distinct streams' frames and, per frame, (out, state_disp, state_weight) and the masks of the three branches
    the frame's pixels took where a history existed: blended with it, restarted against it, held it."""
    _, H, W = sc.TEMPORAL_CAP_SHAPE
    seq = t_temp.frames(np.random.default_rng(9002), (P, H, W), sc.TEMPORAL_FRAMES)
    r = temporal_ref.TemporalRef((P, H, W), **TEMP_PARAMS)
    steps = []
    p = r.params
    for d, c, g in seq:
        with np.errstate(invalid="ignore", over="ignore"):
            dv = median_ref.valid_mask(d, p["invalid_disparity"])
            a = (r.A * np.float32(p["decay"])).astype(np.float32)
            still = temporal_ref.static_mask(g, r.G, p["motion_radius"], p["motion_threshold"])
            had = (a > 0) & median_ref.valid_mask(r.D, p["invalid_disparity"])
            hist = had & still
            agree = dv & hist & (np.abs((d - r.D).astype(np.float32)) <= np.float32(p["max_diff"]))
            branches = dict(average=agree, reset=dv & had & ~agree, hold=~dv & hist & (a >= np.float32(p["min_weight"])))
        out = r.apply(d, g, c)
        steps.append((out, r.D.copy(), r.A.copy(), branches))
    return seq, steps


def test_temporal_past_the_map_cap(cd):
    n, H, W = sc.TEMPORAL_CAP_SHAPE
    seq, steps = temporal_distinct()
    for f, (out, D, A, _) in enumerate(steps):
        assert_distinct(out, f"frame {f}: out")
        assert_distinct(A, f"frame {f}: state_weight")
    for name in ("average", "reset", "hold"):
        assert steps[-1][3][name].any(), f"no pixel of the last frame takes the {name} branch"
    filt = cd.TemporalFilter(n, H, W, **TEMP_PARAMS)
    for f, ((d, c, g), (out, D, A, _)) in enumerate(zip(seq, steps)):
        nxt = filt._guides[1 - filt._prev]                        # the plane this call's guide_out is
        nxt.copy_(sentinel((n, H, W)))
        got = sentinel((n, H, W))
        filt.apply(tile_dev(d, n), tile_dev(g, n), confidence=tile_dev(c, n), out=got)
        assert_tiled(got, out, f"frame {f}: out")
        sd, sw = filt.state
        assert_tiled(sd, D, f"frame {f}: state_disp")
        assert_tiled(sw, A, f"frame {f}: state_weight")
        assert_tiled(nxt, g, f"frame {f}: guide_out")
    del filt
    torch.cuda.empty_cache()


# ---- 3. SGM --------------------------------------------------------------------------------------------------------------

def sgm_distinct(case, seed):
    """The distinct u8 gray pairs of an SGM case and their expected (out, gray_out, right_out)."""
    _, H, W, dmin, D = case
    left, right = t_sgm.frames(P, 1, H, W, "u8", seed, D=min(D, 16))
    opt = sc.SGM_CAP_OPTIONS
    out, gray = sgm_ref.sgm_ref(left, right, dmin, D, paths=opt["paths"], uniqueness=opt["uniqueness"],
                                lr_max_diff=opt["lr_max_diff"], invalid_disparity=INVALID)
    right_map = t_conf._sgm_expect(left, right, dmin, D, opt["paths"], 10, 120, INVALID)
    return left, right, out, gray, right_map


def run_sgm_case(cd, case, seed):
    n, H, W, dmin, D = case
    left, right, out, gray, right_map = sgm_distinct(case, seed)
    for name, e in (("out", out), ("gray_out", gray), ("right_out", right_map)):
        assert_distinct(e, f"sgm {name}")
    assert (out == INVALID).any() and (out != INVALID).any(), "valid and invalid pixels"
    sgm = cd.StereoSGM(dmin, dmin + D - 1, invalid_disparity=INVALID, **sc.SGM_CAP_OPTIONS)
    sgm.workspace(n, H, W, torch.device("cuda", torch.cuda.current_device())).fill_(SENTINEL_BYTE)
    tl, tr = tile_dev(left, n), tile_dev(right, n)
    o, g, ro = sentinel((n, H, W)), sentinel((n, H, W)), sentinel((n, H, W))
    sgm.compute(tl, tr, out=o, gray_out=g, right_out=ro)
    assert_tiled(g, gray, "sgm gray_out")
    assert_tiled(ro, right_map, "sgm right_out")
    assert_tiled(o, out, "sgm out")
    del sgm
    torch.cuda.empty_cache()


def test_sgm_past_the_census_and_selection_caps(cd):
    run_sgm_case(cd, sc.SGM_CAP_CASE, 9003)


def test_sgm_wide_range_past_the_census_cap(cd):
    run_sgm_case(cd, sc.SGM_CAP_WIDE_CASE, 9004)


# ---- 4. weighted median ---------------------------------------------------------------------------------------------------

def window_total(d, g, x, y, radius, rw, sw):
    """T of pixel (x, y) of one map: the summed weight of the valid samples of its window (the rule of the header)."""
    H, W = d.shape
    T = 0
    for qx in range(max(0, x - radius), min(H, x + radius + 1)):
        for qy in range(max(0, y - radius), min(W, y + radius + 1)):
            if median_ref.valid_mask(d[qx, qy], INVALID):
                k = int(median_ref.range_index(g[x, y], g[qx, qy]))
                T += int(sw[abs(qx - x) * (radius + 1) + abs(qy - y)]) * int(rw[k])
    return T


def median_distinct(cd):
    """The distinct (map, guide, holes), the tables and the expectations of both modes."""
    _, H, W = sc.MEDIAN_CAP_SHAPE
    rng = np.random.default_rng(9005)
    d, g = t_med.random_map(rng, (P, H, W)), t_med.random_guide(rng, (P, H, W))
    d[3, :, :2] = INVALID                           # pixel (0, 0) of map 3: no valid sample in its window
    h = t_med.holes_of(rng, d)
    rw, sw = cd.median_weight_tables(sc.MEDIAN_CAP_RADIUS, *sc.MEDIAN_CAP_SIGMAS)
    whole = median_ref.weighted_median(d, g, sc.MEDIAN_CAP_RADIUS, rw, sw, invalid_disparity=INVALID)
    holes = median_ref.weighted_median(d, g, sc.MEDIAN_CAP_RADIUS, rw, sw, holes=h, invalid_disparity=INVALID)
    return d, g, h, rw, sw, whole, holes


def test_median_past_the_tile_cap(cd):
    n, H, W = sc.MEDIAN_CAP_SHAPE
    d, g, h, rw, sw, whole, holes = median_distinct(cd)
    assert_distinct(whole, "median of the whole map")
    assert_distinct(holes, "median of the holes")
    hole = ~median_ref.valid_mask(h, INVALID)
    assert hole.any(axis=(1, 2)).any() and not hole.all(), "a map with a hole, and pixels that are none"
    empty = [(i, x, y) for i, x, y in np.argwhere(hole)
             if window_total(d[i], g[i], x, y, sc.MEDIAN_CAP_RADIUS, rw, sw) == 0]
    assert empty, "no filtered pixel has a window total of 0"
    assert (whole.view(np.uint32) != d.view(np.uint32)).any(), "the filter changes a value"
    sigma_color, sigma_space = sc.MEDIAN_CAP_SIGMAS
    kw = dict(radius=sc.MEDIAN_CAP_RADIUS, sigma_color=sigma_color, sigma_space=sigma_space, invalid_disparity=INVALID)
    td, tg = tile_dev(d, n), tile_dev(g, n)
    out = sentinel((n, H, W))
    cd.weighted_median(td, tg, out=out, **kw)
    assert_tiled(out, whole, "median of the whole map")
    out = sentinel((n, H, W))
    cd.weighted_median(td, tg, holes=tile_dev(h, n), out=out, **kw)
    assert_tiled(out, holes, "median of the holes")
    assert_tiled(td, d, "in untouched")


# ---- 5. WLS --------------------------------------------------------------------------------------------------------------

WLS_LAMBDA, WLS_SIGMA, WLS_MIN_WEIGHT = 500.0, 4.0, 1e-3


def wls_distinct(cd, H, W, seed):
    rng = np.random.default_rng(seed)
    d, g = t_wls.random_map(rng, (P, H, W)), t_wls.random_guide(rng, (P, H, W), nan_frac=0.05)
    c = t_wls.random_conf(rng, (P, H, W))
    lam, rw = cd.wls_tables(WLS_LAMBDA, WLS_SIGMA, sc.WLS_CAP_ITERATIONS, 0.25)
    want = wls_ref.wls_filter(d, g, lam, rw, confidence=c, min_weight=WLS_MIN_WEIGHT, invalid_disparity=INVALID)
    return d, g, c, lam, rw, want


@pytest.mark.parametrize("shape", sc.WLS_CAP_SHAPES, ids=[f"{h}x{w}" for _, h, w in sc.WLS_CAP_SHAPES])
def test_wls_past_the_line_caps(cd, shape):
    """Through the C entry, so that the workspace (the planes U, V and E that one launch hands to the next) starts as
    sentinels like every output: the Python entry allocates its own."""
    from cuda_depth import _native as N
    n, H, W = shape
    d, g, c, lam, rw, want = wls_distinct(cd, H, W, 9006 + H)
    assert_distinct(want, f"wls {H}x{W}")
    assert (want == INVALID).any() and (want != INVALID).any(), "pixels with and without weight"
    assert (want[:, 0, 0] != want[:, -1, -1]).any(), "the first and the last pixel of a map differ"
    try:
        ws = torch.full((int(N.LIB.smx_wls_workspace_bytes(n, H, W)),), SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
        td, tg, tc = tile_dev(d, n), tile_dev(g, n), tile_dev(c, n)
        out = sentinel((n, H, W))
        t_wls.run(td, tg, lam, rw, conf=tc, out=out, min_weight=WLS_MIN_WEIGHT, invalid=INVALID, workspace=ws)
        del ws, tg, tc
        assert_tiled(out, want, f"wls {H}x{W}")
        assert_tiled(td, d, "in untouched")
    finally:
        ws = td = tg = tc = out = None
        torch.cuda.empty_cache()


# ---- 6. rectification ----------------------------------------------------------------------------------------------------

def remap_distinct(dtype, C, border, seed=9010):
    """The distinct raw pairs, the two maps and the expected rectified pairs of one run."""
    _, Hi, Wi, Ho, Wo = sc.REMAP_CAP_CASE
    rng = np.random.default_rng(seed + C)
    npdt = np.uint8 if dtype == "u8" else np.float32
    L, R = t_rect.random_images(rng, P, C, Hi, Wi, npdt), t_rect.random_images(rng, P, C, Hi, Wi, npdt)
    qL, qR = t_rect.random_qmap(rng, Ho, Wo, Hi, Wi), t_rect.random_qmap(rng, Ho, Wo, Hi, Wi)
    for q in (qL, qR):                              # the generator aims mostly outside a 2 x 3 input: pull most taps inside
        inner = np.stack([rng.integers(-20, Wi * 32, (Ho, Wo)), rng.integers(-20, Hi * 32, (Ho, Wo))], -1).astype(np.int32)
        keep = rng.random((Ho, Wo)) < 0.2
        q[~keep] = inner[~keep]
    bv = 201.0 if dtype == "u8" else -3.75
    mode = rectify_ref.CONSTANT if border == "constant" else rectify_ref.REPLICATE
    return L, R, qL, qR, bv, rectify_ref.remap(L, qL, mode, bv), rectify_ref.remap(R, qR, mode, bv)


@pytest.mark.parametrize("dtype,C,border,both", sc.REMAP_CAP_RUNS,
                         ids=[f"{d}-C{c}-{b}-{'pair' if p else 'left'}" for d, c, b, p in sc.REMAP_CAP_RUNS])
def test_rectification_past_the_chunk_cap(cd, dtype, C, border, both):
    n, Hi, Wi, Ho, Wo = sc.REMAP_CAP_CASE
    L, R, qL, qR, bv, want_l, want_r = remap_distinct(dtype, C, border)
    assert_distinct(want_l, "rectified left")
    assert_distinct(want_r, "rectified right")
    for q in (qL, qR):
        inside = rectify_ref.taps(q, Hi, Wi, rectify_ref.CONSTANT)[2]
        assert inside.any() and not inside.all(), "the maps must mix taps inside the input and border taps"
    rect = cd.StereoRectification(qL, qR, (Hi, Wi), (Ho, Wo), border_mode=border, border_value=bv)
    tdt = torch.uint8 if dtype == "u8" else torch.float32
    tl = tile_dev(L, n)
    lo, ro = sentinel((n, C, Ho, Wo), tdt), sentinel((n, C, Ho, Wo), tdt)
    if both:
        rect.rectify(tl, tile_dev(R, n), out=(lo, ro))
        assert_tiled(ro, want_r, "rectified right")
    else:
        rect.rectify(tl, out=lo)
        assert bool((as_bits(ro) == (SENTINEL_BYTE if dtype == "u8" else SENTINEL_BITS)).all()), "right output written"
    assert_tiled(lo, want_l, "rectified left")
    assert_tiled(tl, L, "left input untouched")


# ---- 7. the LR pack and 8. the mirrored LR check without LDS ------------------------------------------------------------

def flip(a):
    return np.ascontiguousarray(a[..., ::-1])


def oracle_lr(oracle, ocfg, L, R):
    dl = oracle.run(ocfg, L, R)
    dr = flip(oracle.run(ocfg, flip(R), flip(L)))
    return lr_rule(dl, dr, 1.0, INVALID), dr


LR_DISTINCT = 2                                     # distinct C2 pairs of the pack cases: pair i is distinct pair i % 2


@pytest.fixture(scope="module")
def c2_lr_pairs(oracle_omp):
    """The distinct C2 pairs (integer-valued gray, so the uint8 and float32 entries see the same frames) and their
    (checked left map, right-view map) from the oracle and the rule, computed once for the pack cases."""
    H, W, K, D = sc.C2_H, sc.C2_W, sc.LR_PACK_K, sc.LR_PACK_D
    L, R = syn.make_batch(LR_DISTINCT, H, W, D, K, 40)
    L, R = np.ascontiguousarray(L, np.float32), np.ascontiguousarray(R, np.float32)
    assert np.array_equal(L, np.rint(L)) and L.min() >= 0 and L.max() <= 255
    ocfg = OracleConfig(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
    want = [oracle_lr(oracle_omp, ocfg, L[i], R[i]) for i in range(LR_DISTINCT)]
    assert not np.array_equal(want[0][0], want[1][0]) and not np.array_equal(want[0][1], want[1][1])
    return L, R, want


def lr_engine(cd, H, W, K, D, n):
    cfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
    return cd.StereoMatching(cfg, max_batch=2 * n)


@pytest.mark.parametrize("n,dtype", sc.LR_PACK_CASES, ids=[f"{n}-{d}" for n, d in sc.LR_PACK_CASES])
def test_lr_pack_strides(cd, c2_lr_pairs, n, dtype):
    """The engine's packed inputs are scratch of its own: a first call on the inverted frames leaves it holding other
    values than the checked call writes, so an element the pack skips cannot pass as written."""
    H, W = sc.C2_H, sc.C2_W
    L, R, want = c2_lr_pairs
    idx = np.arange(n) % LR_DISTINCT
    tdt = torch.uint8 if dtype == "u8" else torch.float32
    tl, tr = torch.from_numpy(L[idx]).cuda().to(tdt), torch.from_numpy(R[idx]).cuda().to(tdt)
    sm = lr_engine(cd, H, W, sc.LR_PACK_K, sc.LR_PACK_D, n)
    sm.compute_disparity_map_batch_lr(255 - tl, 255 - tr)
    out, right_out = sentinel((n, H, W)), sentinel((n, H, W))
    sm.compute_disparity_map_batch_lr(tl, tr, out, right_out=right_out, max_diff=1.0, invalid_disparity=INVALID)
    got, got_r = out.cpu().numpy(), right_out.cpu().numpy()
    for i in range(n):
        assert_bitwise(got_r[i], want[idx[i]][1], f"right_out pair {i}")
        assert_bitwise(got[i], want[idx[i]][0], f"out pair {i}")
    del sm
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n,H,W,K,D", sc.LR_WIDE_CASES, ids=[f"W{c[2]}" for c in sc.LR_WIDE_CASES])
def test_mirrored_lr_check_on_rows_wider_than_lds(cd, oracle_omp, n, H, W, K, D):
    l, r, _ = syn.make_pair(H, W, D, K, 60 + W % 7)
    L, R = np.ascontiguousarray(l, np.float32)[None], np.ascontiguousarray(r, np.float32)[None]
    ocfg = OracleConfig(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
    want, want_r = oracle_lr(oracle_omp, ocfg, L[0], R[0])
    valid = want != INVALID
    assert 0.05 < valid.mean() < 0.999, f"both outcomes of the check must occur ({valid.mean():.3f} valid)"
    sm = lr_engine(cd, H, W, K, D, n)
    out, right_out = sentinel((n, H, W)), sentinel((n, H, W))
    sm.compute_disparity_map_batch_lr(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), out, right_out=right_out,
                                      max_diff=1.0, invalid_disparity=INVALID)
    assert_bitwise(right_out[0], want_r, "right_out")
    assert_bitwise(out[0], want, "out")


# ---- 9. camera tracking --------------------------------------------------------------------------------------------------

def track_distinct():
    """The distinct triples' operands (frames, model views and their poses, start poses) and the twin's four outputs."""
    _, shape, model_shape = sc.TRACK_CAP_CASE
    margin = trk.run_margin(sc.TRACK_CAP_SCHEDULE)                # the frames scaled_expected tracks
    frames = [trk.scaled_frame(shape, k, view, margin)[0] for view, k, _ in sc.TRACK_CAP_TRIPLES]
    models = [trk.scaled_model(view, model_shape, misses) for view, _, misses in sc.TRACK_CAP_TRIPLES]
    want = [trk.scaled_expected(shape, sc.TRACK_CAP_SCHEDULE, k, view, model_shape, misses,
                               min_inliers=sc.TRACK_CAP_MIN_INLIERS) for view, k, misses in sc.TRACK_CAP_TRIPLES]
    ops = dict(disp=np.stack(frames), depth=np.stack([m["depth"] for m in models]),
               normals=np.stack([m["normals"] for m in models]), c2w=np.stack([m["c2w"] for m in models]),
               w2c=np.stack([m["w2c"] for m in models]),
               pose_in=np.stack([trk.start_pose(view) for view, _, _ in sc.TRACK_CAP_TRIPLES]))
    outs = dict(pose_out=np.stack([w["pose"] for w in want]), info=np.stack([w["info"] for w in want]).astype(np.int32),
                rms=np.array([w["rms"] for w in want], np.float32), sums=np.stack([w["sums"] for w in want]))
    return ops, outs, trk.scaled_q(shape, margin), models[0]["Qm"], models[0]["Pm"]


def test_track_past_the_triple_cap(cd):
    """Through the C entry, so that the outputs and the workspace (the triples' state and partial sums, which one launch
    hands to the next) start as sentinels."""
    from cuda_depth import _native as N
    n, shape, model_shape = sc.TRACK_CAP_CASE
    ops, outs, Q, Qm, Pm = track_distinct()
    for name, e in outs.items():
        assert_distinct(e, f"track {name}")
    lost = outs["info"][:, 0] != 0
    assert [bool(v) for v in lost] == [m for _, _, m in sc.TRACK_CAP_TRIPLES] and lost.any() and not lost.all()
    iterations = sum(k for _, k in sc.TRACK_CAP_SCHEDULE)
    assert (outs["info"][~lost, 1] == iterations).all() and (outs["info"][lost, 1] == 1).all(), "a tracked triple runs on"
    assert (outs["info"][~lost, 2] >= sc.TRACK_CAP_MIN_INLIERS).all()
    tiled = {k: tile_dev(v, n) for k, v in ops.items()}
    got = dict(pose_out=sentinel((n, 3, 4)), info=sentinel((n, 4), torch.int32), rms=sentinel((n,)),
               sums=sentinel((n, 30), torch.float64))
    ws_bytes = int(N.LIB.smx_track_camera_workspace_bytes(n, *shape))
    assert ws_bytes > 0
    ws = torch.full((ws_bytes,), SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
    call = t_track.Direct.of(n, shape, model_shape, Q, Qm, Pm, sc.TRACK_CAP_SCHEDULE, ws=ws, **tiled, **got)
    assert call.call(min_inliers=sc.TRACK_CAP_MIN_INLIERS) == 0, call.native.last_error()
    torch.cuda.synchronize()
    for name, e in outs.items():
        assert_tiled(got[name], e, f"track {name}")
    assert_tiled(tiled["disp"], ops["disp"], "disp untouched")
    assert_tiled(tiled["pose_in"], ops["pose_in"], "pose_in untouched")
