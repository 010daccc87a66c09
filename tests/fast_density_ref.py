"""Model of the density report of the sparse fast kernel (k_match_fast.h: fast_stats_report), numpy only.

The sparse form of k_match_fast adds [marches of its second pass : 40][windows : 24] to a counter of its stream lane, from a
sample of the launch; the call's fill kernel (k_fill.h: fill_publish_fast_stats) publishes marches / (windows * ceil(Dd / 2)).
Both numbers are exact functions of the winner map and the launch geometry:

  * a window is FA_VALID = 42 pooled columns by `band_rows` rows (the unit band of 24 rows in the stacked form, whose
    fast_stacked_tail reports once per unit band that holds image rows); a partial last window counts, an empty one does not;
  * the needed set of a window is the union over its pixels of (a + 1) mod Dd and (a - 1) mod Dd of the winner a (the
    dup_left dedup skips only marks that a left neighbour makes anyway: the set is the same);
  * the second pass walks the needed disparities of one right-tile chunk [d0, d0 + nd) at a time and marches them two by
    two: ceil(|needed in chunk| / 2) marches per chunk (an odd one out marches alone: `if (pend >= 0) march(pend, pend)`);
  * latency shape (12-row bands): the FA_DS_WAVES = 8 waves of a workgroup share one window and take the needed disparities
    pair by pair in turn, `(seen >> 1) % NW == wv`; every wave reports its own marches, wave 0 the window; only workgroups
    with (blk.x + gridDim.x * blk.y) % 16 == 0 report;
  * of a launch of n pairs those with b % stride == 0 report, stride = (n + 3) / 4 if n > 4 else 1 (smx_plan.h: plan_range);
  * a call split over both stream lanes is two launches, pairs [0, n0) and [n0, n) with n0 = (n + 1) / 2 (smx_engine.hip:
    enqueue); the engine's observation is the float32 mean of the lanes' ratios (smx_route.h: ContentSwitch::observe).

The second half of the module names the inputs and the calls of tests/test_fast_density_gpu.py, so that
tests/test_fast_density_cpu.py can check from the oracle alone that those inputs can tell a wrong report from a right one."""
import numpy as np

import stereo_synthetic as syn

FA_VALID = 42               # k_match_fast.h: FA_VALID, output columns of a wave
FA_WAVES = 4                # k_match_fast.h: FA_WAVES, column windows of a throughput-shape workgroup
FA_WGCOLS = 190             # k_match_fast.h: FA_WGCOLS, staged left columns (4 * 42 + 2 * 11)
FA_TH = 24                  # k_match_fast.h: FA_TH, the unit band
FA_STACK_TH = 48            # k_match_fast.h: FA_STACK_TH
FA_TH_SMALL = 8             # k_match_fast.h: FA_TH_SMALL
FA_TH_SMALL_TALL = 12       # k_match_fast.h: FA_TH_SMALL_TALL
FA_DS_WAVES = 8             # k_match_fast.h: FA_DS_WAVES, waves of a latency-shape workgroup
FA_STAT_WG_STRIDE_DS = 16   # k_match_fast.h: FA_STAT_WG_STRIDE_DS
PLAIN_ROWS = (24, 27, 32)   # k_match_fast.h: match_fast_plan, `cand`


def tall_pitch(Dd):
    """k_match_fast.h: fast_tall_pitch (FA_WIDE_FROM = 67, FA_MID_UPTO = 99)."""
    return 256 if Dd <= 67 else (288 if Dd <= 99 else 320)


def tall_nd(Dd):
    """Disparities per right-tile chunk of the throughput shape: ND = PR - FA_WGCOLS + 1 = 67 / 99 / 131."""
    return tall_pitch(Dd) - FA_WGCOLS + 1


def small_nd(Dd):
    """... of the latency shape: ND = PR - 64 + 1 with PR = 320 above 193 disparities (fast_small_wide), else 256."""
    return (320 if Dd > 193 else 256) - 64 + 1


def sample_stride(n):
    """smx_plan.h: plan_range, `p.stride`."""
    return (n + 3) // 4 if n > 4 else 1


def sampled_pairs(n, stride=None):
    """Launch-local indices of the pairs that report (k_match_fast.h: fast_stats_report, `b % p.fast_stride != 0`)."""
    stride = sample_stride(n) if stride is None else stride
    return [b for b in range(n) if b % stride == 0]


def needed_set(a, Dd):
    """Disparities the second pass revisits for the winners `a` of one window: pad_index(a + 1), pad_index(a - 1)."""
    a = np.asarray(a, np.int64).ravel()
    return np.unique(np.concatenate([(a + 1) % Dd, (a - 1) % Dd]))


def chunk_counts(needed, Dd, nd):
    """Needed disparities per right-tile chunk [d0, d0 + nd)."""
    return [int(((needed >= d0) & (needed < d0 + nd)).sum()) for d0 in range(0, Dd, nd)]


def marches_of_needed(needed, Dd, nd):
    """Throughput shape: the needed disparities of each chunk two by two (a pair never spans two right tiles)."""
    return sum((c + 1) // 2 for c in chunk_counts(np.asarray(needed), Dd, nd))


def window_marches_throughput(a, Dd, nd):
    return marches_of_needed(needed_set(a, Dd), Dd, nd)


def window_marches_latency(a, Dd, nd, nw=FA_DS_WAVES):
    """As the kernel deals them: the needed disparity of rank `seen` in its chunk is wave (seen >> 1) % nw's; every wave
    marches its own share two by two."""
    total = 0
    for c in chunk_counts(needed_set(a, Dd), Dd, nd):
        share = [0] * nw
        for seen in range(c):
            share[(seen >> 1) % nw] += 1
        total += sum((s + 1) // 2 for s in share)
    return total


def ratio_f32(marches, windows, Dd):
    """k_fill.h: fill_publish_fast_stats, in float32 as there."""
    return np.float32(marches) / (np.float32(windows) * np.float32((Dd + 1) // 2))


def report(wtas, Dd, band_rows, nd, sampled, shape="throughput"):
    """(marches, windows, ratio) of ONE launch.  wtas: winner maps [h, w] indexed by the launch-local pair index (a list, or
    a function of the index); sampled: the pairs that report; shape: "throughput" (every wave its own window of 42 columns by
    band_rows rows) or "latency" (one window per workgroup, every 16th workgroup)."""
    get = wtas if callable(wtas) else (lambda b: wtas[b])
    marches = windows = 0
    for b in sampled:
        a = np.asarray(get(b))
        h, w = a.shape
        gx, gy = -(-w // FA_VALID), -(-h // band_rows)
        for y in range(gy):
            for x in range(gx):
                if shape == "latency" and (x + gx * y) % FA_STAT_WG_STRIDE_DS != 0:
                    continue
                win = a[y * band_rows:(y + 1) * band_rows, x * FA_VALID:(x + 1) * FA_VALID]
                if win.size == 0:
                    continue
                windows += 1
                marches += (window_marches_latency if shape == "latency" else window_marches_throughput)(win, Dd, nd)
    return marches, windows, ratio_f32(marches, windows, Dd)


def lane_ranges(n, lanes):
    """(first pair, pairs) of the launches of a call (smx_engine.hip: enqueue, `n0 = split ? (n + 1) / 2 : n`)."""
    if lanes == 1:
        return [(0, n)]
    n0 = (n + 1) // 2
    return [(0, n0), (n0, n - n0)]


def observation(ratios):
    """smx_route.h: ContentSwitch::observe -- the float32 mean of the fresh reports."""
    s = np.float32(0)
    for r in ratios:
        s = np.float32(s + np.float32(r))
    return np.float32(s / np.float32(len(ratios)))


def call_report(wta_of_pair, n, lanes, Dd, band_rows, nd, shape="throughput", pick=None):
    """The observation of one call of n pairs: per lane (marches, windows, ratio), and their mean.  wta_of_pair: winner map
    of the call's pair j.  pick(n_lane) -> launch-local sampled indices (default: the kernel's rule)."""
    pick = pick or sampled_pairs
    per_lane = [report(lambda b, first=first: wta_of_pair(first + b), Dd, band_rows, nd, pick(nl), shape)
                for first, nl in lane_ranges(n, lanes)]
    return per_lane, observation([r[2] for r in per_lane])


# ---- the calls of tests/test_fast_density_gpu.py ---------------------------------------------------------------------------

def throughput_pairs(h, w, cus, on_lanes):
    """The smallest call in the throughput shape (k_match_fast.h: match_fast_plan, `pl.small = 8 * wgs_tall < (on_lanes ?
    8 : 13) * cus`): one workgroup of unit bands per CU on the stream lanes, 1.625 on a caller's stream."""
    wgs = -(-w // (FA_VALID * FA_WAVES)) * -(-h // FA_TH)
    return -(-(8 if on_lanes else 13) * cus // (8 * wgs))


def tall_lds_bytes(th, Dd):
    """k_match_fast.h: fast_lds_bytes of the throughput shape -- the two u16 tiles of th + 22 rows (left pitch FA_PL = 192), the
    four waves' needed-set tables (fast_bitwords) and their exchange rows (FA_XCH_FLOATS = 2 * 2 * 76 floats)."""
    bitwords = 2 if Dd > 64 * 32 else (Dd + 1) & ~1
    return (th + 22) * (192 + tall_pitch(Dd)) * 2 + FA_WAVES * bitwords * 4 + FA_WAVES * 304 * 4


def plain_band_rows(h, Dd):
    """k_match_fast.h: match_fast_plan's choice among 24 / 27 / 32 rows: the fewest marched rows, 32-row bands weighted by
    1.06 and a tile that does not fit three times into a CU's 160 KB of LDS (1280-byte granules) by 1.3."""
    best, best_rows = 24, None
    for th in PLAIN_ROWS:
        three = 3 * (-(-tall_lds_bytes(th, Dd) // 1280) * 1280) <= 160 * 1024
        rows = -(-h // th) * (th + 22) * (106 if th == 32 else 100) * (100 if three else 130)
        if best_rows is None or rows < best_rows:
            best, best_rows = th, rows
    return best


def latency_shape(cus, max_h=200, max_w=640):
    """A pooled size whose single-pair call takes the split kernel at 12-row bands (match_fast_plan: `wg_small > cus &&
    wg_tall <= cus`), or None."""
    def fits(h, w):
        windows = -(-w // FA_VALID)
        small = 8 * (-(-w // (FA_VALID * FA_WAVES)) * -(-h // FA_TH)) < 13 * cus
        return small and windows * -(-h // FA_TH_SMALL) > cus and windows * -(-h // FA_TH_SMALL_TALL) <= cus
    if fits(187, 621):
        return 187, 621
    for h in range(max_h - 1, 24, -1):                 # (odd sizes first: partial last bands and windows)
        for w in range(max_w - 1, 42, -1):
            if fits(h, w) and h % FA_TH_SMALL_TALL and w % FA_VALID:
                return h, w
    return None


FLAT_SHIFT = 20             # pooled disparity of the `flat` pair


def make_content(name, H, W, D, K):
    """(left, right) of a named content class, uint8-valued float32.  band / slant / noise: the synthetic pairs of index 70
    (a trailing apostrophe: 71); flat: one cyclic shift, every winner the same."""
    index = 71 if name.endswith("'") else 70
    base = name.rstrip("'")
    if base == "band":
        return syn.make_pair(H, W, D, K, index)[:2]
    if base == "slant":
        return syn.make_slanted_pair(H, W, D, K, index)[:2]
    if base == "noise":
        return syn.make_noise_pair(H, W, index)
    if base == "flat":
        left = syn.make_pair(H, W, D, K, 72)[0]
        return left, np.roll(left, -min(FLAT_SHIFT, max(D // K - 2, 0)) * K, axis=1).copy()
    raise KeyError(name)


MIXED = ("band", "slant", "noise", "flat", "band'", "slant'")

# name: K, pooled h, w, Dd; tiles: the distinct pairs the batch tiles (idx = j % len); stack: SMX_FAST_STACK (None: unset);
# streams: engine streams (the lanes) or the caller's stream; lanes: 1, or 2 (twice the pairs, overlap_min_pairs = 2);
# rows: the band_rows match_geometry must report (None: one of 24 / 27 / 32, the plan's choice); height: whether the case
# names a window height that its values must tell from the other two (condition 2; not where every height gives one value);
# group: cases that run one shape on several contents and answer condition 2 together
def _case(name, h, w, Dd, tiles, stack, streams, lanes=1, rows=None, K=2, height=True, mixed=False, group=None):
    return dict(name=name, K=K, h=h, w=w, Dd=Dd, tiles=tuple(tiles), stack=stack, streams=streams, lanes=lanes, rows=rows,
                height=height, mixed=mixed, group=group)


CASES = (
    [_case(f"plain_{c}", 96, 190, 64, [c], "0", False, group="plain") for c in ("band", "slant", "noise")] +
    [_case(f"stacked_forced_{c}", 96, 190, 64, [c], "1", False, rows=48, group="stacked_forced") for c in ("band", "slant", "noise")] +
    [_case("stacked_by_rule_one_lane", 96, 190, 64, ["band"], None, True, rows=48),
     _case("stacked_by_rule_two_lanes", 96, 190, 64, ["band"], None, True, lanes=2, rows=48),
     _case("plain_27_rows", 54, 190, 64, ["slant"], "0", False),
     _case("stacked_where_plain_is_27", 54, 190, 64, ["slant"], "1", True, rows=48),
     _case("plain_32_rows", 30, 190, 64, ["noise"], "0", False),
     _case("partial_half_57", 57, 190, 64, ["slant"], "1", True, rows=48),
     _case("partial_half_30", 30, 190, 64, ["noise"], "1", True, rows=48),
     _case("idle_wave_48x100", 48, 100, 64, ["noise"], "1", True, rows=48),
     _case("mixed_plain", 96, 190, 64, MIXED, "0", False, mixed=True),
     _case("mixed_stacked", 96, 190, 64, MIXED, "1", False, rows=48, mixed=True),
     # both lanes sample different tiles: the observation is the mean of two different ratios
     _case("mixed_two_lanes", 96, 190, 64, MIXED, None, True, lanes=2, rows=48, mixed=True),
     _case("range_67", 57, 190, 67, ["noise"], "1", True, rows=48),
     _case("range_33", 57, 190, 33, ["noise"], "1", True, rows=48),
     # two disparities: both neighbours of winner 0 are disparity 1 and both of winner 1 disparity 0 -- one march per window
     # against one march of pass 1, whatever the window height: the report is 1.0 and names no height
     _case("range_2", 57, 190, 2, ["noise"], "1", True, rows=48, height=False),
     _case("range_140_plain", 48, 190, 140, ["slant"], "1", True)])
CASES_BY_NAME = {c["name"]: c for c in CASES}
LATENCY_CONTENT = "slant"
LATENCY_DD = 64


def case_pairs(case, cus):
    """Pairs of a case's call on a device of `cus` compute units."""
    return case["lanes"] * throughput_pairs(case["h"], case["w"], cus, case["streams"])


def case_model_rows(case, reported_rows=None):
    """Window height of the case's model: the unit band where the stacked form runs, else the plan's band."""
    if case["rows"] == FA_STACK_TH:
        return FA_TH
    return plain_band_rows(case["h"], case["Dd"]) if reported_rows is None else reported_rows
