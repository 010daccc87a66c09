"""The model of the sparse fast kernel's density report (tests/fast_density_ref.py) on hand-made winner maps, and the inputs
of tests/test_fast_density_gpu.py against the conditions that make that test able to fail -- from the oracle alone, no GPU.

The conditions, for every GPU case (printed per case: marches, windows, ratio and the margins; run with -s to see them):
  1. windows * ceil(Dd / 2) <= 900 for what one distinct pair contributes to a lane's sample, so that one march too many or too
     few in that pair's windows moves the ratio by more than 0.0011, twice the half-unit of the three-decimal print.  (Per
     distinct pair, not per sample: a launch samples up to four pairs, and at 96 x 190 / 64 one pair alone is 20 windows x
     32 = 640.  The kernel is deterministic, so every sampled copy of a pair carries the same miscount and a batch of identical
     pairs moves by 1 / 640 however many copies are sampled; the literal figure of the whole sample is printed beside it.)
  2. In every case that names a window height, the model at R = 24, 27 and 32 differs pairwise by more than 0.002 -- for the
     three cases that run the same shape on three contents (plain_*, stacked_forced_*) in at least one of the contents, which
     is the case's verdict on the height: scene-like content at 96 x 190 / 64 gives 197 / 20 at 24 and at 27 rows alike.
     Every one of R = 24, 27, 32 and the stacked 24 has a case.
  3. Mixed content: the model over the sampled pairs differs by more than 0.005 from the model over all pairs and from the model
     over the pairs b % (stride + 1) == 0.
n depends on the device's compute units; the conditions are checked for 256 (MI355X) and, where n matters (3), again by the GPU
test for the device at hand."""
import itertools

import numpy as np
import pytest

import fast_density_ref as fd
from oracle_lib import OracleConfig

CUS = 256                   # MI355X


# ---- the model on hand-made maps ------------------------------------------------------------------------------------------------

def _const(h, w, a):
    return np.full((h, w), a, np.int32)


@pytest.mark.parametrize("a", [1, 5, 30, 62])
def test_constant_map_is_one_march_per_window(a):
    m, win, r = fd.report([_const(48, 84, a)], 64, 24, 67, [0])
    assert (m, win) == (4, 4) and r == np.float32(4) / (np.float32(4) * np.float32(32))


def test_winner_zero_wraps_to_the_last_disparity_and_back():
    assert fd.needed_set(_const(3, 3, 0), 64).tolist() == [1, 63]
    assert fd.needed_set(_const(3, 3, 63), 64).tolist() == [0, 62]
    # ... which at 140 disparities lie in two chunks of 131: one march each
    assert fd.report([_const(24, 42, 0)], 140, 24, 131, [0])[:2] == (2, 1)
    assert fd.report([_const(24, 42, 139)], 140, 24, 131, [0])[:2] == (2, 1)


def test_two_disparities_need_one_march():
    for a in (0, 1):
        assert fd.needed_set(_const(2, 2, a), 2).tolist() == [1 - a]
        m, win, r = fd.report([_const(24, 42, a)], 2, 24, 67, [0])
        assert (m, win, float(r)) == (1, 1, 1.0)


def test_needed_set_across_a_chunk_boundary_marches_twice():
    """140 disparities in chunks of 131: needed {130, 131} lie in two right tiles -- two marches, not one."""
    assert fd.chunk_counts(np.array([130, 131]), 140, 131) == [1, 1]
    assert fd.marches_of_needed([130, 131], 140, 131) == 2
    assert fd.marches_of_needed([130, 131], 140, 140) == 1                       # (the same two in one chunk: one march)
    assert fd.window_marches_throughput(np.array([[131]]), 140, 131) == 2        # winner 131: needed {130, 132}
    assert fd.window_marches_throughput(np.array([[129, 132]]), 140, 131) == 1 + 1   # {128, 130} and {131, 133}


def test_partial_last_window_counts_and_an_empty_one_does_not():
    a = _const(57, 100, 7)
    assert fd.report([a], 64, 24, 67, [0])[:2] == (9, 9)            # 3 unit bands x 3 column windows (the third: 16 columns)
    assert fd.report([a], 64, 27, 67, [0])[:2] == (9, 9)            # 27 + 27 + 3 rows
    assert fd.report([a], 64, 32, 67, [0])[:2] == (6, 6)
    a[48:, 84:] = 20                                                 # only the partial corner window differs
    assert fd.report([a], 64, 24, 67, [0])[:2] == (9, 9)
    a[47, 83] = 20                                                   # ... and now its three neighbours hold two winners too
    assert fd.report([a], 64, 24, 67, [0])[:2] == (9 + 1, 9)


def test_latency_dealing_with_an_odd_count():
    # 19 needed disparities: waves 0 and 1 get two pairs and one pair + one, the others one pair: 10 marches, as
    # ceil(19 / 2); written out as the kernel deals them
    a = np.arange(1, 37, 2, dtype=np.int32)[None, :]                 # winners 1, 3, .., 35: needed 0, 2, .., 36
    assert len(fd.needed_set(a, 64)) == 19
    assert fd.window_marches_latency(a, 64, 193) == 10
    assert fd.window_marches_latency(a, 64, 193, nw=1) == 10
    # across two chunks the dealing starts again: 10 + 9 needed -> 5 + 5
    assert fd.window_marches_latency(a, 64, 19) == 5 + 5
    # every 16th workgroup: 17 x 2 workgroups, linear ids 0, 16, 32
    m, win, _ = fd.report([_const(24, 17 * 42, 9)], 64, 12, 193, [0], "latency")
    assert (m, win) == (3, 3)


def test_stride_rule():
    assert [fd.sample_stride(n) for n in (4, 5, 8, 9, 32)] == [1, 2, 2, 3, 8]
    assert fd.sampled_pairs(4) == [0, 1, 2, 3]
    assert fd.sampled_pairs(5) == [0, 2, 4]
    assert fd.sampled_pairs(8) == [0, 2, 4, 6]
    assert fd.sampled_pairs(9) == [0, 3, 6]
    assert fd.sampled_pairs(32) == [0, 8, 16, 24]


def test_two_lane_mean():
    maps = [_const(24, 42, 3)] * 3 + [np.arange(24 * 42, dtype=np.int32).reshape(24, 42) % 64] * 2
    per_lane, obs = fd.call_report(lambda j: maps[j], 5, 2, 64, 24, 67)           # lanes of 3 and 2 pairs
    assert fd.lane_ranges(5, 2) == [(0, 3), (3, 2)]
    assert [r[:2] for r in per_lane] == [(3, 3), (64, 2)]
    assert obs == np.float32((np.float32(3) / np.float32(96) + np.float32(1.0)) / np.float32(2))
    assert fd.observation([np.float32(0.1), np.float32(0.3)]) == np.float32((np.float32(0.1) + np.float32(0.3)) / np.float32(2))


# ---- the GPU test's inputs --------------------------------------------------------------------------------------------------------

_WTA = {}


def wta_of(oracle, K, h, w, Dd, content):
    """The oracle's pooled winner indices of a named pair, once per distinct pair."""
    key = (K, h, w, Dd, content)
    if key not in _WTA:
        H, W, D = h * K, w * K, Dd * K
        cfg = OracleConfig(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
        l, r = fd.make_content(content, H, W, D, K)
        _WTA[key] = oracle.run(cfg, l, r, intermediates=True)[1]["wta_index"].copy()
    return _WTA[key]


def _case_model(oracle, case, n, rows, pick=None):
    tiles = [wta_of(oracle, case["K"], case["h"], case["w"], case["Dd"], c) for c in case["tiles"]]
    return fd.call_report(lambda j: tiles[j % len(tiles)], n, case["lanes"], case["Dd"], rows, fd.tall_nd(case["Dd"]), pick=pick)


def _pairwise_margin(vals):
    return min(abs(float(a) - float(b)) for a, b in itertools.combinations(vals, 2))


def height_margins(oracle, case, n):
    by_rows = {R: _case_model(oracle, case, n, R)[1] for R in fd.PLAIN_ROWS}
    return by_rows, _pairwise_margin(by_rows.values())


def sampling_margins(oracle, case, n, rows):
    """Condition 3: (model, model over all pairs, model over b % (stride + 1) == 0)."""
    right = _case_model(oracle, case, n, rows)[1]
    everyone = _case_model(oracle, case, n, rows, pick=lambda nl: list(range(nl)))[1]
    off_by_one = _case_model(oracle, case, n, rows, pick=lambda nl: fd.sampled_pairs(nl, fd.sample_stride(nl) + 1))[1]
    return right, everyone, off_by_one


@pytest.mark.parametrize("case", fd.CASES, ids=[c["name"] for c in fd.CASES])
def test_gpu_case_can_tell_a_wrong_report(oracle_omp, case):
    n = fd.case_pairs(case, CUS)
    rows = fd.case_model_rows(case)
    per_lane, obs = _case_model(oracle_omp, case, n, rows)
    pass1 = (case["Dd"] + 1) // 2
    line = f"{case['name']}: n {n}, R {rows}:"
    for k, (m, win, r) in enumerate(per_lane):
        nl = fd.lane_ranges(n, case["lanes"])[k][1]
        sampled = fd.sampled_pairs(nl)
        # condition 1, per distinct pair of the lane's sample
        per_pair = max(fd.report([wta_of(oracle_omp, case["K"], case["h"], case["w"], case["Dd"], c)], case["Dd"], rows,
                                 fd.tall_nd(case["Dd"]), [0])[1] for c in case["tiles"])
        line += f" lane {k}: {m}/{win} = {float(r):.4f} (sample of {len(sampled)}: windows x pass 1 = {win * pass1}, per pair {per_pair * pass1})"
        assert per_pair * pass1 <= 900, line
    line += f" -> {float(obs):.4f}"
    if case["height"]:
        by_rows, margin = height_margins(oracle_omp, case, n)
        line += " | by height " + ", ".join(f"{R}: {float(v):.4f}" for R, v in by_rows.items()) + f", margin {margin:.4f}"
        group = [c for c in fd.CASES if case["group"] and c["group"] == case["group"]]
        best = max([margin] + [height_margins(oracle_omp, c, n)[1] for c in group])
        assert best > 0.002, line
    if case["mixed"]:
        right, everyone, off_by_one = sampling_margins(oracle_omp, case, n, rows)
        line += f" | all pairs {float(everyone):.4f}, stride + 1 {float(off_by_one):.4f}"
        assert abs(float(right) - float(everyone)) > 0.005 and abs(float(right) - float(off_by_one)) > 0.005, line
    print(line)


def test_every_window_height_has_a_case():
    heights = {("stacked" if c["rows"] == fd.FA_STACK_TH else "plain", fd.case_model_rows(c)) for c in fd.CASES if c["height"]}
    assert heights >= {("plain", 24), ("plain", 27), ("plain", 32), ("stacked", 24)}, heights


def test_plain_and_stacked_models_differ_where_the_plain_plan_is_taller(oracle_omp):
    """54 x 190: the plain plan marches 27-row bands, the stacked form reports from 24-row windows -- the stacked case must be
    modelled with the unit band, the plain plan's height gives another value.  (At 96 x 190 / 64 both are 24 rows: a 32-row
    tile of pitch 256 does not fit a CU three times, so the plan keeps 4 x 46 marched rows.)"""
    plain, stacked = fd.CASES_BY_NAME["plain_27_rows"], fd.CASES_BY_NAME["stacked_where_plain_is_27"]
    assert (plain["h"], plain["w"], plain["Dd"], plain["tiles"]) == (stacked["h"], stacked["w"], stacked["Dd"], stacked["tiles"])
    assert fd.plain_band_rows(plain["h"], plain["Dd"]) == 27 and fd.plain_band_rows(96, 64) == 24
    a = wta_of(oracle_omp, 2, plain["h"], plain["w"], plain["Dd"], plain["tiles"][0])
    at24, at27 = (fd.report([a], plain["Dd"], R, 67, [0])[2] for R in (24, 27))
    print(f"scene-like 54 x 190 / 64: stacked {float(at24):.4f}, plain {float(at27):.4f}")
    assert abs(float(at24) - float(at27)) > 0.002


def test_table_of_the_notes(oracle_omp):
    """NOTES.md, "Density report against its model": one pair of each content class at 96 x 190 / 64, by window height."""
    want = {"band": ((26, 20), (37, 20), (32, 15)), "slant": ((197, 20), (197, 20), (182, 15)),
            "noise": ((597, 20), (592, 20), (469, 15)), "flat": ((20, 20), (20, 20), (15, 15))}
    for content, row in want.items():
        a = wta_of(oracle_omp, 2, 96, 190, 64, content)
        got = tuple(fd.report([a], 64, R, 67, [0])[:2] for R in fd.PLAIN_ROWS)
        print(content, " ".join(f"{m}/{w} = {float(fd.ratio_f32(m, w, 64)):.4f}" for m, w in got))
        assert got == row, (content, got)


def test_latency_shape_at_256_compute_units(oracle_omp):
    """The single latency frame: every 16th workgroup reports, so the sample stays small (condition 1, literally)."""
    assert fd.latency_shape(CUS) == (187, 621)
    h, w = fd.latency_shape(CUS)
    a = wta_of(oracle_omp, 2, h, w, fd.LATENCY_DD, fd.LATENCY_CONTENT)
    m, win, r = fd.report([a], fd.LATENCY_DD, fd.FA_TH_SMALL_TALL, fd.small_nd(fd.LATENCY_DD), [0], "latency")
    print(f"latency {h} x {w}: {m}/{win} = {float(r):.4f}")
    assert win == 15 and win * ((fd.LATENCY_DD + 1) // 2) <= 900
