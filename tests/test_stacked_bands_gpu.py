"""The stacked bands of the throughput aggregation kernel (k_match_fast.h: FA_STACK) against the oracle.

On the stream lanes a sparse-form launch of the throughput shape marches two 24-row unit bands in one go: pass 1 runs over
48 output rows (70 marched ones), and the store block, the needed-set table and the sparse second pass -- all written for
at most 32 band rows -- run once per 24-row half on the tile that is already staged.  Every case is one engine-stream call
large enough for the throughput shape on this device; smx_get_match_geometry must report 48-row bands for it.  The planner
stacks only where that marches fewer rows, which none of the small shapes A, B and C below does (A: 2 x 70 rows against 2 x 54
of 32-row bands): those run with the form forced (SMX_FAST_STACK=1); shape D is stacked by the rule itself.  The final
map, the WTA index and the three cost planes of every distinct pair are compared bit for bit with the oracle
(multi_block_matching_cost_aggregation.cu:54-88, wta_disparity_selection.cu:22-30, secondary_matching.cu:28-31), and the
whole batch bit for bit with an engine that has the form forbidden (SMX_FAST_STACK=0).

Shapes, chosen for what the halves can get wrong (pooled sizes):
  A  57 x 190, 64 disparities: two workgroup columns, the second with one active wave of 22 columns; the second band is
     partial (9 rows: a first half of 9 rows, an empty second half).  At K = 1, 2, 4 and 8: the three packed-sum forms.
  B  30 x 190: one band, the first half full, the second with 6 rows.
  C  98 x 190, 33 disparities (an unpaired last disparity): two full bands and a tail of 2 rows.
  D  96 x 190: two full bands, 2 x 70 marched rows against 4 x 49 -- planned by the rule, nothing forced.
Limits of the form, each forced unless the rule stacks by itself (H73): the ranges 67 (the LDS cap), 66, 65 (one needed word
alone in the second 64-word ballot group), 32 (a one-group table), 3 and 2 (both neighbours the same disparity) at shape A;
the widths 168 (no idle wave), 169 (a workgroup column of one pixel column), 43 (wave 1 owns one column) and 100 at 57 rows;
the heights 24 (second half empty), 25 (one row), 48, 49 (a second band of one row) and 73 at width 100; K = 4 and K = 8 at 25 x 100.
Content: banded, scene-like and noise pairs (noise fills the needed sets of both halves), tiled over the batch.  One more
call is an AUTO batch of f32 gray with one off-grid pair (the gated launches), one is split over both lanes (both shape D)."""
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
    wgs = -(-w // WG_COLS) * -(-h // UNIT_ROWS)
    return -(-cus // wgs)


def _distinct(H, W, D, K):
    """Two banded, two scene-like and two noise pairs, uint8-valued."""
    return ([syn.make_pair(H, W, D, K, 70 + i)[:2] for i in range(2)] + [syn.make_slanted_pair(H, W, D, K, 70 + i)[:2] for i in range(2)] +
            [syn.make_noise_pair(H, W, 70 + i) for i in range(2)])


_ORACLE = {}


def _oracle_runs(oracle, ocfg, key, pairs):
    """(map, intermediates) of every distinct pair, computed once per shape and shared by the cases that use it."""
    if key not in _ORACLE:
        _ORACLE[key] = [oracle.run(ocfg, l, r, intermediates=True, volumes=True) for l, r in pairs]
    return _ORACLE[key]


def _call(cd, cfg, tl, tr, n, stack, monkeypatch, overlap_min_pairs=-1, match_mode="auto"):
    from cuda_depth import _native as N
    if stack is None:
        monkeypatch.delenv("SMX_FAST_STACK", raising=False)
    else:
        monkeypatch.setenv("SMX_FAST_STACK", stack)                 # read once, in smx_create
    sm = cd.StereoMatching(cfg, max_batch=n, match_mode=match_mode, overlap_min_pairs=overlap_min_pairs)
    out = sm.compute_disparity_map_batch(tl, tr, engine_streams=True)
    sm.join()
    torch.cuda.synchronize()
    geo = sm.match_geometry(n)
    stages = {k: torch.stack([sm.intermediate(st, i) for i in range(n)]) for k, st in
              (("wta", N.STAGE_WTA), ("costs", N.STAGE_MBM_COSTS), ("refined", N.STAGE_REFINED), ("down_left", N.STAGE_DOWN_LEFT),
               ("down_right", N.STAGE_DOWN_RIGHT))}
    stages["out"] = out.clone()
    return geo, stages


CASES = [
    # name, K, pooled h, pooled w, pooled disparities, SMX_FAST_STACK of the stacked engine
    ("A_k2", 2, 57, 190, 64, "1"),
    ("A_k1", 1, 57, 190, 64, "1"),
    ("A_k4", 4, 57, 190, 64, "1"),
    ("A_k8", 8, 57, 190, 64, "1"),
    ("B_one_partial_band", 2, 30, 190, 64, "1"),
    ("C_odd_range", 2, 98, 190, 33, "1"),
    ("D_by_rule", 2, 96, 190, 64, None),
    # the limits of the form (shape A's 57 x 190 unless said otherwise; six distinct pairs each)
    ("R67_lds_cap", 2, 57, 190, 67, "1"),            # the largest instantiation (fast_stacked_raise_lds_caps): 68 table words
    ("R66", 2, 57, 190, 66, "1"),
    ("R65_lone_word_in_group_2", 2, 57, 190, 65, "1"),   # needed word 64 alone in the second ballot group: a pending partner crosses groups
    ("R32_one_group", 2, 57, 190, 32, "1"),
    ("R3", 2, 57, 190, 3, "1"),
    ("R2_both_neighbours_one_march", 2, 57, 190, 2, "1"),     # dn == dp: both cost planes come from one march
    ("W168_no_idle_wave", 2, 57, 168, 64, "1"),      # one full workgroup column
    ("W169_one_pixel_column", 2, 57, 169, 64, "1"),  # the second workgroup column owns one pixel column
    ("W43_wave_1_one_column", 2, 57, 43, 64, "1"),
    ("W100", 2, 57, 100, 64, "1"),
    ("H24_second_half_empty", 2, 24, 100, 64, "1"),
    ("H25_second_half_one_row", 2, 25, 100, 64, "1"),
    ("H48", 2, 48, 100, 64, "1"),
    ("H49_second_band_one_row", 2, 49, 100, 64, "1"),
    ("H73_by_rule", 2, 73, 100, 64, None),           # 2 x 70 marched rows against 3 x 49 of 27-row bands: the rule stacks
    ("H25_k4", 4, 25, 100, 64, "1"),                 # the other packed-sum forms through a one-row half
    ("H25_k8", 8, 25, 100, 64, "1"),
]
D_SHAPE = (2, 96, 190, 64)


@pytest.mark.parametrize("name,K,h,w,Dd,stack", CASES, ids=[c[0] for c in CASES])
def test_stacked_call_against_the_oracle_and_the_plain_bands(cd, oracle_omp, monkeypatch, cus, name, K, h, w, Dd, stack):
    H, W, D = h * K, w * K, Dd * K
    n = _throughput_pairs(h, w, cus)
    cfg, ocfg = parity._cfgs(cd, H, W, K, 0, D - 1)
    pairs = _distinct(H, W, D, K)
    idx = torch.arange(n, device="cuda") % len(pairs)
    tl, tr = (torch.from_numpy(np.stack([p[k] for p in pairs])).to(torch.uint8).cuda()[idx].contiguous() for k in (0, 1))
    geo, got = _call(cd, cfg, tl, tr, n, stack, monkeypatch)
    assert geo["kernel"] == "fast_window" and geo["band_rows"] == 48 and geo["rows_marched"] == 70, geo
    geo0, plain = _call(cd, cfg, tl, tr, n, "0", monkeypatch)
    assert geo0["kernel"] == "fast_window" and geo0["band_rows"] in (24, 27, 32), geo0
    if name == "H73_by_rule":                        # match_fast_plan: `rows_stack < ceil(h / th) * (th + 22)`
        assert geo0["band_rows"] == 27 and -(-h // 48) * 70 == 140 < -(-h // 27) * 49 == 147, geo0
    for k in got:
        assert torch.equal(got[k], plain[k]), f"{name}: {k} differs from the engine with the stacked bands forbidden"
    for i, (ref_out, ref) in enumerate(_oracle_runs(oracle_omp, ocfg, (K, h, w, Dd), pairs)):
        for j in (i, i + len(pairs) * ((n - 1 - i) // len(pairs))):  # the pair's first and last copy in the batch
            assert int(idx[j]) == i
            parity._check({k: v[j].cpu().numpy() for k, v in got.items()}, ref_out, ref, 0)


def test_auto_batch_with_an_off_grid_pair_takes_the_gated_stacked_launch(cd, oracle_omp, monkeypatch, cus):
    """f32 gray, AUTO: the fast launch is gated on the device-side grid flag; the off-grid pair is the exact-order kernel's."""
    K, h, w, Dd = D_SHAPE
    H, W, D = h * K, w * K, Dd * K
    n = _throughput_pairs(h, w, cus)
    cfg, ocfg = parity._cfgs(cd, H, W, K, 0, D - 1)
    pairs = _distinct(H, W, D, K)
    monkeypatch.delenv("SMX_FAST_STACK", raising=False)
    refs = _oracle_runs(oracle_omp, ocfg, (K, h, w, Dd), pairs)
    off = n // 2 + 1                                                 # one pair moved off the grid (not integer-valued)
    left_off = (pairs[off % len(pairs)][0] + np.float32(0.3)).astype(np.float32)
    ref_off = oracle_omp.run(ocfg, left_off, pairs[off % len(pairs)][1])
    idx = torch.arange(n, device="cuda") % len(pairs)
    tl, tr = (torch.from_numpy(np.stack([p[k] for p in pairs])).cuda()[idx].contiguous() for k in (0, 1))
    tl[off] = torch.from_numpy(left_off).cuda()
    sm = cd.StereoMatching(cfg, max_batch=n, overlap_min_pairs=-1)
    sm.profile_begin(1)
    out = sm.compute_disparity_map_batch(tl, tr, engine_streams=True)
    sm.join()
    prof = sm.profile_end()
    torch.cuda.synchronize()
    assert sm.last_match_mode() == "auto" and (prof["match_fast"][1], prof["match_exact"][1]) == (1, 1), (sm.last_match_mode(), prof)
    geo = sm.match_geometry(n)
    assert geo["kernel"] == "fast_window" and geo["band_rows"] == 48, geo
    got = out.cpu().numpy()
    for j in range(n):
        want = ref_off if j == off else refs[j % len(pairs)][0]
        assert np.array_equal(got[j], want), f"pair {j} of {n} ({'off' if j == off else 'on'} the grid) differs from the oracle"


def test_call_split_over_both_lanes(cd, oracle_omp, monkeypatch, cus):
    """Twice the pairs with overlap_min_pairs = 2: each lane launches a stacked half, side by side."""
    K, h, w, Dd = D_SHAPE
    H, W, D = h * K, w * K, Dd * K
    n = 2 * _throughput_pairs(h, w, cus)
    cfg, ocfg = parity._cfgs(cd, H, W, K, 0, D - 1)
    pairs = _distinct(H, W, D, K)
    idx = torch.arange(n, device="cuda") % len(pairs)
    tl, tr = (torch.from_numpy(np.stack([p[k] for p in pairs])).to(torch.uint8).cuda()[idx].contiguous() for k in (0, 1))
    geo, got = _call(cd, cfg, tl, tr, n, None, monkeypatch, overlap_min_pairs=2)
    assert geo["kernel"] == "fast_window" and geo["band_rows"] == 48, geo
    want = torch.from_numpy(np.stack([r[0] for r in _oracle_runs(oracle_omp, ocfg, (K, h, w, Dd), pairs)])).cuda()[idx]
    differing = (got["out"] != want).flatten(1).any(dim=1).nonzero().flatten().tolist()
    assert not differing, f"pairs {differing[:20]} of {n} differ from the oracle's map of their distinct pair"
