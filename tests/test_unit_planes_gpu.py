"""The pooled planes in grid units (k_prologue.h -> MatchParams::Lu / Ru) and the fast kernels' staging from them
(k_match_fast.h: fast_stage_units) against the oracle, bit for bit.

The prologue writes every pooled pixel a second time as (unsigned short)(K^2 * pooled) into rows of round_up(w + 3, 4)
columns whose last three repeat the first three; the fast kernels and the capture kernel copy their tiles from those rows four
columns per lane and row.  Shapes (pooled sizes), chosen for where that can go wrong:
  * w mod 4 = 1, 2, 3, 0 (169 .. 172): the apron and the last lane's group; w = 169 also leaves the second workgroup column
    one pixel column, and its left tile wraps on both sides;
  * h = 49 and 53: a partial last band, cyclic row wrap above and below;
  * ranges of 1, 2, 67, 68 and 131 pooled disparities: the right tile's first column takes every alignment mod 4; 67 fills
    pitch 256, 68 takes pitch 288 with ONE column in the second group of 256, 131 fills pitch 320;
  * odd full-resolution W and H at K = 2: the generic prologue; K = 1, 2, 4 and the u8 entry: the other prologues;
  * min_disparity > 0: the capture kernel; a range wider than the image: the right tile wraps more than once.
Every shape runs as a single frame (latency shape: the waves of a workgroup share one window) and as the smallest
engine-stream call that takes the throughput shape.  Further calls: batches of 1, 2 and 9; RGB entries (AUTO: their pooled
values are off the grid, the planes are written and not used); an AUTO batch whose middle pair is off the grid; the stacked
bands on the lanes; and FAST_GRID forced on off-grid input at K = 1, where the unit of the grid is one gray level and the
truncated planes are exactly the planes of the truncated images, and at K = 2 / 4 on a pair shifted by 0.3, whose truncated
units are those of the same pair shifted by 0.25 (which is on the grid)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stereo_synthetic as syn                      # noqa: E402
import test_gpu_parity as parity                    # noqa: E402

WG_COLS, UNIT_ROWS = 168, 24                        # k_match_fast.h: FA_VALID * FA_WAVES, FA_TH


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


@pytest.fixture(scope="module")
def cus(cd):
    cfg = cd.StereoMatchingConfiguration(height=64, width=96, min_disparity=0, max_disparity=15)
    return cd.StereoMatching(cfg).route_info()["compute_units"]


def _throughput_pairs(h, w, cus):
    """The smallest engine-stream call in the throughput shape (match_fast_plan: one workgroup of 24-row bands per CU)."""
    return -(-cus // (-(-w // WG_COLS) * -(-h // UNIT_ROWS)))


def _distinct(H, W, D, K, dmin=0):
    """A banded, a scene-like and a noise pair, uint8-valued."""
    return [syn.make_pair(H, W, D, K, 90, dmin=dmin)[:2], syn.make_slanted_pair(H, W, D, K, 91)[:2], syn.make_noise_pair(H, W, 92)]


_ORACLE = {}


def _oracle_runs(oracle, ocfg, key, pairs):
    """(map, intermediates) of every distinct pair, computed once per shape and shared by the cases that use it."""
    if key not in _ORACLE:
        _ORACLE[key] = [oracle.run(ocfg, l, r, intermediates=True, volumes=True) for l, r in pairs]
    return _ORACLE[key]


def _call(cd, cfg, tl, tr, n, engine_streams, match_mode="auto"):
    from cuda_depth import _native as N
    sm = cd.StereoMatching(cfg, max_batch=n, match_mode=match_mode, overlap_min_pairs=-1)
    out = sm.compute_disparity_map_batch(tl, tr, engine_streams=engine_streams)
    if engine_streams:
        sm.join()
    torch.cuda.synchronize()
    stages = {k: torch.stack([sm.intermediate(st, i) for i in range(n)]) for k, st in
              (("wta", N.STAGE_WTA), ("costs", N.STAGE_MBM_COSTS), ("refined", N.STAGE_REFINED), ("down_left", N.STAGE_DOWN_LEFT),
               ("down_right", N.STAGE_DOWN_RIGHT))}
    stages["out"] = out.clone()
    return sm, stages


def _tensors(pairs, idx, u8):
    tl, tr = (torch.from_numpy(np.stack([p[k] for p in pairs])).cuda() for k in (0, 1))
    if u8:
        tl, tr = tl.to(torch.uint8), tr.to(torch.uint8)
    return tl[idx].contiguous(), tr[idx].contiguous()


SHAPES = [
    # name, u8 entry, K, H, W, min_disparity, max_disparity   ->   pooled h x w, pooled range
    ("w169_h49_r131_f32_k2", False, 2, 98, 338, 0, 261),       # 49 x 169, 131: pitch 320 filled
    ("w170_h53_r68_u8_k2", True, 2, 106, 340, 0, 135),         # 53 x 170, 68: pitch 288, one column in the second group
    ("w171_h49_r67_f32_k1", False, 1, 49, 171, 0, 66),         # 49 x 171, 67: pitch 256 filled
    ("w172_h53_r2_u8_k4", True, 4, 212, 688, 0, 7),            # 53 x 172, 2: the K = 4 prologue
    ("w169_h49_r1_f32_k2", False, 2, 98, 338, 0, 1),           # 49 x 169, 1
    ("odd_W_and_H_w170_h49_r67_f32_k2", False, 2, 97, 339, 0, 133),   # generic prologue at K = 2
    ("w172_h53_r68_f32_k4", False, 4, 212, 688, 0, 271),       # the K = 4 prologue, f32 entry
    ("range_wider_than_the_image_w40_r100_k1", False, 1, 30, 40, 0, 99),
    ("min_disparity_w171_h53_k2", False, 2, 106, 342, 8, 47),  # pooled 4 .. 23: the capture kernel
    ("min_disparity_w169_h49_u8_k1", True, 1, 49, 169, 5, 71),  # pooled 5 .. 71 (67 disparities)
]


@pytest.mark.parametrize("batch", ["single", "throughput"])
@pytest.mark.parametrize("name,u8,K,H,W,dmin,dmax", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes_against_the_oracle(cd, oracle_omp, monkeypatch, cus, name, u8, K, H, W, dmin, dmax, batch):
    monkeypatch.delenv("SMX_FAST_STACK", raising=False)
    h, w = -(-H // K), -(-W // K)
    cfg, ocfg = parity._cfgs(cd, H, W, K, dmin, dmax)
    pairs = _distinct(H, W, dmax + 1, K, dmin)
    refs = _oracle_runs(oracle_omp, ocfg, name, pairs)
    n = len(pairs) if batch == "single" else max(len(pairs), _throughput_pairs(h, w, cus))
    idx = torch.arange(n, device="cuda") % len(pairs)
    tl, tr = _tensors(pairs, idx, u8)
    if batch == "single":
        for i in range(n):
            sm, got = _call(cd, cfg, tl[i:i + 1], tr[i:i + 1], 1, False)
            assert sm.last_match_mode() in ("auto", "fast_grid"), sm.last_match_mode()
            assert sm.match_geometry(1)["kernel"].startswith("fast"), sm.match_geometry(1)
            parity._check({k: v[0].cpu().numpy() for k, v in got.items()}, refs[i][0], refs[i][1], dmin // K)
        return
    sm, got = _call(cd, cfg, tl, tr, n, True)
    geo = sm.match_geometry(n)
    assert geo["kernel"] == "fast_window", geo
    for j in list(range(len(pairs))) + [n - 1]:
        i = j % len(pairs)
        parity._check({k: v[j].cpu().numpy() for k, v in got.items()}, refs[i][0], refs[i][1], dmin // K)
    want = torch.from_numpy(np.stack([r[0] for r in refs])).cuda()[idx]
    differing = (got["out"] != want).flatten(1).any(dim=1).nonzero().flatten().tolist()
    assert not differing, f"pairs {differing[:20]} of {n} differ from the oracle's map of their distinct pair"


BATCH_SHAPE = (2, 98, 338, 133)                       # K, H, W, max_disparity: 49 x 169 pooled, 67 disparities


@pytest.mark.parametrize("n", [1, 2, 9])
def test_small_batches_on_a_callers_stream(cd, oracle_omp, n):
    """The latency shapes: 8-, 10- and 12-row bands, by what the call's workgroups make of the chip."""
    K, H, W, dmax = BATCH_SHAPE
    cfg, ocfg = parity._cfgs(cd, H, W, K, 0, dmax)
    pairs = _distinct(H, W, dmax + 1, K)
    refs = _oracle_runs(oracle_omp, ocfg, "batch_shape", pairs)
    idx = torch.arange(n, device="cuda") % len(pairs)
    tl, tr = _tensors(pairs, idx, False)
    sm, got = _call(cd, cfg, tl, tr, n, False)
    assert sm.match_geometry(n)["kernel"].startswith("fast"), sm.match_geometry(n)
    for j in range(n):
        i = j % len(pairs)
        parity._check({k: v[j].cpu().numpy() for k, v in got.items()}, refs[i][0], refs[i][1], 0)


def test_auto_batch_of_three_with_the_middle_pair_off_the_grid(cd, oracle_omp):
    """The off-grid pair's planes hold truncated values and must not be used (the gate sends it to the exact-order kernel); its
    neighbours in the buffers stay exact."""
    K, H, W, dmax = BATCH_SHAPE
    cfg, ocfg = parity._cfgs(cd, H, W, K, 0, dmax)
    pairs = _distinct(H, W, dmax + 1, K)
    refs = _oracle_runs(oracle_omp, ocfg, "batch_shape", pairs)
    left_off = (pairs[1][0] + np.float32(0.3)).astype(np.float32)
    ref_off = oracle_omp.run(ocfg, left_off, pairs[1][1], intermediates=True, volumes=True)
    tl, tr = _tensors(pairs, torch.arange(3, device="cuda"), False)
    tl[1] = torch.from_numpy(left_off).cuda()
    sm, got = _call(cd, cfg, tl, tr, 3, False)
    assert sm.last_match_mode() == "auto"
    for j in range(3):
        ref_out, ref = ref_off if j == 1 else refs[j]
        parity._check({k: v[j].cpu().numpy() for k, v in got.items()}, ref_out, ref, 0)


def test_forced_fast_grid_off_the_grid_truncates_at_k1(cd):
    """match_mode = "fast_grid" on off-grid input keeps what the f32 staging computed: (unsigned short)(K^2 * pooled).  At
    K = 1 the pooled image is the image, so the aggregation of the off-grid pair is the aggregation of its truncated images:
    the WTA map and the three cost planes are equal bit for bit (step 6 reads the gray itself and differs)."""
    H, W, dmax = 49, 171, 66
    cfg, _ = parity._cfgs(cd, H, W, 1, 0, dmax)
    (l, r), = _distinct(H, W, dmax + 1, 1)[1:2]
    l_off, r_off = (l * np.float32(0.97) + np.float32(0.3)).astype(np.float32), (r * np.float32(0.99) + np.float32(0.6)).astype(np.float32)
    assert np.any(l_off != np.floor(l_off)) and l_off.min() >= 0 and r_off.max() < 256
    a = parity._run_hip(cd, cfg, l_off, r_off, "fast_grid")
    b = parity._run_hip(cd, cfg, np.floor(l_off), np.floor(r_off), "fast_grid")
    assert a["mode"] == b["mode"] == "fast_grid" and a["flag"] != 0 and b["flag"] == 0
    assert np.array_equal(a["wta"], b["wta"]) and np.array_equal(a["costs"], b["costs"])


@pytest.mark.parametrize("batch", ["single", "throughput"])
@pytest.mark.parametrize("K", [2, 4])
def test_forced_fast_grid_off_the_grid_keeps_the_truncated_units(cd, cus, monkeypatch, K, batch):
    """The same through k_prologue_k2 / _k4, whose unit is 4 / 16 per gray level.  With S = K^2 * pooled of an integer-valued
    pair: + 0.3 on every pixel gives K^2 * pooled = S + 1.2 (K = 2) or S + 4.8 (K = 4) up to float32 rounding far below the
    fraction, off the grid, and truncates to S + 1 / S + 4; + 0.25 on every pixel is exact, stays on the grid and gives S + 1 /
    S + 4 as it stands.  Forced FAST_GRID must therefore aggregate both pairs alike: WTA map and cost planes bit for bit.  A
    staging that rounded, or a prologue that wrote another value than the f32 staging computed, would differ.  Single frame
    (latency shape) and the smallest engine-stream call of the throughput shape."""
    monkeypatch.delenv("SMX_FAST_STACK", raising=False)
    h, w, Dd = 49, 169, 67
    H, W, dmax = h * K, w * K, Dd * K - 1
    cfg, _ = parity._cfgs(cd, H, W, K, 0, dmax)
    l, r = (np.minimum(a, np.float32(254)) for a in syn.make_slanted_pair(H, W, dmax + 1, K, 93)[:2])
    n = 1 if batch == "single" else _throughput_pairs(h, w, cus)
    got = {}
    for name, off in (("off", np.float32(0.3)), ("on", np.float32(0.25))):
        tl, tr = (torch.from_numpy((a + off).astype(np.float32)).cuda()[None].expand(n, H, W).contiguous() for a in (l, r))
        sm, st = _call(cd, cfg, tl, tr, n, batch != "single", match_mode="fast_grid")
        assert sm.last_match_mode() == "fast_grid" and sm.match_geometry(n)["kernel"] == ("fast_split" if n == 1 else "fast_window")
        got[name] = st
    for k in ("wta", "costs"):
        assert torch.equal(got["off"][k], got["on"][k]), f"{k}: the off-grid pair's units are not the truncated ones"
    assert not torch.equal(got["off"]["down_left"], got["on"]["down_left"])


RGB = [("k1", 1, 49, 169), ("k2_odd_W", 2, 98, 339), ("k4", 4, 212, 684)]


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("name,K,H,W", RGB, ids=[c[0] for c in RGB])
def test_rgb_entries(cd, oracle_omp, name, K, H, W, u8):
    """Every RGB prologue writes the planes too (their pooled values are off the grid: AUTO takes the exact-order routes)."""
    from cuda_depth import _native as N
    dmax = 24 * K - 1
    cfg, ocfg = parity._cfgs(cd, H, W, K, 0, dmax)
    left, right = syn.random_rgb_pair(H, W, dmax + 1, K, 3)
    ref_out, ref = oracle_omp.run(ocfg, left, right, intermediates=True, volumes=True)
    sm = cd.StereoMatching(cfg)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    if u8:
        tl, tr = tl.to(torch.uint8), tr.to(torch.uint8)
    out = sm.compute_disparity_map(tl, tr)
    torch.cuda.synchronize()
    im = {"out": out.cpu().numpy()}
    for k, st in (("wta", N.STAGE_WTA), ("costs", N.STAGE_MBM_COSTS), ("refined", N.STAGE_REFINED), ("down_left", N.STAGE_DOWN_LEFT),
                  ("down_right", N.STAGE_DOWN_RIGHT), ("gray_left", N.STAGE_GRAY_LEFT), ("gray_right", N.STAGE_GRAY_RIGHT)):
        im[k] = sm.intermediate(st).cpu().numpy()
    parity._check(im, ref_out, ref, 0)


def test_stacked_bands_on_the_lanes(cd, oracle_omp, monkeypatch, cus):
    """A 110 x 420 image at K = 2 (55 x 210 pooled) as one engine-stream call in the stacked form: 70-row tiles, left and
    right staged together, the second pass of each half on the tile that is already there."""
    K, H, W, dmax = 2, 110, 420, 127
    h, w = H // K, W // K
    cfg, ocfg = parity._cfgs(cd, H, W, K, 0, dmax)
    pairs = _distinct(H, W, dmax + 1, K)
    refs = _oracle_runs(oracle_omp, ocfg, "stacked", pairs)
    n = _throughput_pairs(h, w, cus)
    idx = torch.arange(n, device="cuda") % len(pairs)
    tl, tr = _tensors(pairs, idx, True)
    monkeypatch.setenv("SMX_FAST_STACK", "1")                    # read once, in smx_create
    sm, got = _call(cd, cfg, tl, tr, n, True)
    geo = sm.match_geometry(n)
    assert geo["kernel"] == "fast_window" and geo["band_rows"] == 48 and geo["rows_marched"] == 70, geo
    for j in list(range(len(pairs))) + [n - 1]:
        i = j % len(pairs)
        parity._check({k: v[j].cpu().numpy() for k, v in got.items()}, refs[i][0], refs[i][1], 0)
    want = torch.from_numpy(np.stack([r[0] for r in refs])).cuda()[idx]
    differing = (got["out"] != want).flatten(1).any(dim=1).nonzero().flatten().tolist()
    assert not differing, f"pairs {differing[:20]} of {n} differ from the oracle's map of their distinct pair"
