"""Model of the second pass of the stacked bands (k_match_fast.h: fast_stacked_tail), numpy only.

A stacked launch of the throughput aggregation kernel marches two 24-row unit bands in one go; a wave owns a window of
FA_VALID = 42 pooled columns by 48 rows.  Behind pass 1 every pixel needs AGG at (a + 1) mod Dd and (a - 1) mod Dd of its
winner a, and the second pass marches exactly the disparities that some pixel of the window needs.  From the oracle's winner
map alone this module derives, per window:

  * the three classes of needed disparities -- read by pixels of both unit bands, of the upper one only, of the lower one
    only (the tail keeps one table word per disparity and unit band: a word is non-zero iff the unit band needs it);
  * the tile rows the per-band tail marched (fast_stacked_tail_halves: per unit band its needed disparities two by two,
    TU + 22 = 46 rows a march) and the rows the joint tail marches: pairs of "both" over the whole staged tile (2 TU + 22 =
    70 rows), pairs of "upper" / "lower" over 46, and what is left by the rule of fast_tail_leftover;
  * the marches themselves with their row masks (which the CPU test uses to show that an input reaches every march form).

The rule is restated here (leftover_code, leftover_rows, rows_joint, rows_halves) and pinned to the header's own
__host__ __device__ functions by tests/stacked_tail_harness.cpp.  The report of the sparse form is NOT modelled here: it
kept its meaning (marches of a per-band second pass) and tests/fast_density_ref.py is its model.

The second half names the inputs of tests/test_stacked_tail_gpu.py.

    python tests/stacked_tail_ref.py [pair indices]     class counts and rows on the benchmark's pairs (needs the oracle)"""
import os
import sys

import numpy as np

FA_VALID = 42               # k_match_fast.h: FA_VALID, output columns of a wave
FA_TH = 24                  # k_match_fast.h: FA_TH, the unit band (TU)
FA_STACK_TH = 48            # k_match_fast.h: FA_STACK_TH
ROWS_HALF = FA_TH + 22      # tile rows of a march over one unit band
ROWS_FULL = FA_STACK_TH + 22    # ... over the whole staged tile

# k_match_fast.h: enum FastTailLeftover
FT_NONE, FT_FULL_BB, FT_FULL_BU, FT_FULL_BL, FT_FULL_UL, FT_HALVES, FT_UPPER, FT_LOWER = range(8)


def leftover_code(both, upper, lower):
    """k_match_fast.h: fast_tail_leftover -- how the odd ones out of the three classes are marched."""
    if both:
        return (FT_HALVES if lower else FT_FULL_BU) if upper else (FT_FULL_BL if lower else FT_FULL_BB)
    return (FT_FULL_UL if lower else FT_UPPER) if upper else (FT_LOWER if lower else FT_NONE)


def leftover_rows(code, tu=FA_TH):
    """k_match_fast.h: fast_tail_leftover_rows."""
    if code == FT_NONE:
        return 0
    if code in (FT_UPPER, FT_LOWER):
        return tu + 22
    return 2 * (tu + 22) if code == FT_HALVES else 2 * tu + 22


def rows_joint(nb, nu, nl, tu=FA_TH):
    """k_match_fast.h: fast_tail_rows -- tile rows the joint tail marches for a window with nb / nu / nl needed disparities."""
    return (nb // 2) * (2 * tu + 22) + (nu // 2 + nl // 2) * (tu + 22) + leftover_rows(leftover_code(nb & 1, nu & 1, nl & 1), tu)


def rows_halves(nb, nu, nl, tu=FA_TH):
    """k_match_fast.h: fast_tail_rows_halves -- ... the per-band tail marched."""
    return ((nb + nu + 1) // 2 + (nb + nl + 1) // 2) * (tu + 22)


def row_words(a, Dd):
    """The table of one unit band: word[d] has bit o set iff a pixel of row o needs disparity d.  a: winners [rows, cols]."""
    words = [0] * Dd
    a = np.asarray(a, np.int64)
    for o in range(a.shape[0]):
        for d in set(((a[o] + 1) % Dd).tolist()) | set(((a[o] - 1) % Dd).tolist()):
            words[d] |= 1 << o
    return words


def window_tables(win, Dd):
    """(upper words, lower words) of a window of up to 48 rows."""
    win = np.asarray(win)
    return row_words(win[:FA_TH], Dd), row_words(win[FA_TH:FA_STACK_TH], Dd)


def classes(wu, wl):
    """Needed disparities in ascending order: (both, upper only, lower only)."""
    both = [d for d in range(len(wu)) if wu[d] and wl[d]]
    upper = [d for d in range(len(wu)) if wu[d] and not wl[d]]
    lower = [d for d in range(len(wu)) if wl[d] and not wu[d]]
    return both, upper, lower


def marches(wu, wl):
    """The marches of the joint tail for one window, as the kernel's walk deals them: a list of (kind, da, db, rows_lo,
    rows_hi) with kind "full" / "upper" / "lower"; a full march's mask is upper | lower << 24 split into two 32-bit words, a
    half march's the 24 bits of its unit band in rows_lo.  Pairs within a class in ascending order, then the leftover rule."""
    out = []
    pend = {"b": None, "u": None, "l": None}
    for d in range(len(wu)):
        ru, rl = wu[d], wl[d]
        if not (ru or rl):
            continue
        c = "b" if ru and rl else ("u" if ru else "l")
        if pend[c] is None:
            pend[c] = d
            continue
        e, pend[c] = pend[c], None
        if c == "b":
            out.append(_full(e, d, wu[e] | ru, wl[e] | rl))
        elif c == "u":
            out.append(("upper", e, d, wu[e] | ru, 0))
        else:
            out.append(("lower", e, d, wl[e] | rl, 0))
    b, u, l = pend["b"], pend["u"], pend["l"]
    code = leftover_code(b is not None, u is not None, l is not None)
    if code == FT_FULL_BB:
        out.append(_full(b, b, wu[b], wl[b]))
    elif code == FT_FULL_BU:
        out.append(_full(b, u, wu[b] | wu[u], wl[b]))
    elif code == FT_FULL_BL:
        out.append(_full(b, l, wu[b], wl[b] | wl[l]))
    elif code == FT_FULL_UL:
        out.append(_full(u, l, wu[u], wl[l]))
    elif code == FT_HALVES:
        out.append(("upper", b, u, wu[b] | wu[u], 0))
        out.append(("lower", b, l, wl[b] | wl[l], 0))
    elif code == FT_UPPER:
        out.append(("upper", u, u, wu[u], 0))
    elif code == FT_LOWER:
        out.append(("lower", l, l, wl[l], 0))
    return out, code


def _full(da, db, ru, rl):
    mask = ru | (rl << FA_TH)
    return ("full", da, db, mask & 0xffffffff, mask >> 32)


def rows_of_marches(ms):
    return sum(ROWS_FULL if m[0] == "full" else ROWS_HALF for m in ms)


def windows(a):
    """(band, window, winners [<= 48, <= 42]) of every wave window of a stacked launch that holds pixels."""
    a = np.asarray(a)
    h, w = a.shape
    for y in range(-(-h // FA_STACK_TH)):
        for x in range(-(-w // FA_VALID)):
            yield y, x, a[y * FA_STACK_TH:(y + 1) * FA_STACK_TH, x * FA_VALID:(x + 1) * FA_VALID]


def map_summary(a, Dd):
    """Totals over all windows of a winner map: class counts, rows of either tail, leftover codes, march forms."""
    s = dict(windows=0, both=0, upper=0, lower=0, rows_halves=0, rows_joint=0, codes=[0] * 8, full=0, half=0)
    for _, _, win in windows(a):
        wu, wl = window_tables(win, Dd)
        b, u, l = classes(wu, wl)
        ms, code = marches(wu, wl)
        assert rows_of_marches(ms) == rows_joint(len(b), len(u), len(l))
        s["windows"] += 1
        s["both"] += len(b)
        s["upper"] += len(u)
        s["lower"] += len(l)
        s["rows_halves"] += rows_halves(len(b), len(u), len(l))
        s["rows_joint"] += rows_joint(len(b), len(u), len(l))
        s["codes"][code] += 1
        s["full"] += sum(m[0] == "full" for m in ms)
        s["half"] += sum(m[0] != "full" for m in ms)
    return s


# ---- the inputs of tests/test_stacked_tail_gpu.py ---------------------------------------------------------------------------

SEAM = FA_TH                # first row of the lower unit band


def _texture(H, W, seed):
    """uint8-valued texture, 3 x 3 box-blurred and re-rounded (as stereo_synthetic.make_pair's left image)."""
    rng = np.random.default_rng(seed)
    tex = rng.integers(0, 256, (H, W)).astype(np.float64)
    acc = np.zeros_like(tex)
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            acc += np.roll(tex, (i, j), axis=(0, 1))
    return np.rint(acc / 9.0)


def pair_of_rows(h, w, K, d_rows, seed):
    """(left, right), uint8-valued float32 [h K, w K]: pooled row y of the right image is the left one shifted by the pooled
    disparity d_rows[y] (cyclic: R[x][y] = L[x][(y + K d) mod W], stereo_synthetic's convention)."""
    H, W = h * K, w * K
    left = _texture(H, W, seed)
    g = np.repeat(np.asarray(d_rows, np.int64) * K, K)[:, None]
    cols = (np.arange(W)[None, :] + g) % W
    return left.astype(np.float32), np.take_along_axis(left, cols, axis=1).astype(np.float32)


CONTENTS = ("plane", "seam_step", "step_above", "step_below", "ramp", "plane_0", "plane_last", "noise")


def make_content(name, h, w, Dd, K):
    """The contents the issue of the joint tail names.  Disparities are pooled; a step goes from a quarter to three quarters
    of the range."""
    lo, hi, mid = Dd // 4, (3 * Dd) // 4, Dd // 2
    y = np.arange(h)
    seed = 4100 + CONTENTS.index(name)
    if name == "plane":                      # fronto-parallel: both unit bands need the same two disparities
        return pair_of_rows(h, w, K, np.full(h, mid), seed)
    if name in ("seam_step", "step_above", "step_below"):    # a disparity step on the seam row / one row above / one below
        at = SEAM + {"seam_step": 0, "step_above": -1, "step_below": 1}[name]
        return pair_of_rows(h, w, K, np.where(y % FA_STACK_TH < at, lo, hi), seed)
    if name == "ramp":                       # every row its own disparity
        return pair_of_rows(h, w, K, y % Dd, seed)
    if name == "plane_0":
        return pair_of_rows(h, w, K, np.zeros(h, np.int64), seed)
    if name == "plane_last":
        return pair_of_rows(h, w, K, np.full(h, Dd - 1), seed)
    if name == "noise":                      # uniform noise: every disparity needed by both unit bands
        rng = np.random.default_rng(seed)
        return (rng.integers(0, 256, (h * K, w * K)).astype(np.float32), rng.integers(0, 256, (h * K, w * K)).astype(np.float32))
    raise KeyError(name)


# name: K, pooled h, w, Dd.  `lacks`: what the shape cannot hold, by its geometry (tests/test_stacked_tail_cpu.py asserts the
# rest, and that these are indeed absent):
#   lower    the lower unit band holds no image row: every needed disparity is "upper only"
#   hi_rows  the lower unit band holds at most rows 24 .. 29: no row mask reaches bit 32
def _case(name, K, h, w, Dd, lacks=()):
    return dict(name=name, K=K, h=h, w=w, Dd=Dd, lacks=tuple(lacks))


CASES = [
    _case("48x190_prefix", 2, 48, 190, 64),
    _case("30x190_lower_6_rows", 2, 30, 190, 64, lacks=("hi_rows",)),
    _case("24x190_lower_empty", 2, 24, 190, 64, lacks=("lower", "hi_rows")),
    _case("54x190_second_band_6_rows", 2, 54, 190, 64),
    _case("48x64_one_partial_window", 2, 48, 64, 64),
    _case("48x190_range_67", 2, 48, 190, 67),
    _case("48x190_range_33", 2, 48, 190, 33),
    _case("48x190_range_2", 2, 48, 190, 2),      # both neighbours of winner a are 1 - a: one march fills both cost planes
    _case("48x190_k4_sliding", 4, 48, 190, 64),
]
CASES_BY_NAME = {c["name"]: c for c in CASES}
REPORT_CASES = ("48x190_prefix", "30x190_lower_6_rows", "48x190_range_33")     # ... whose density report is checked as well


def case_pairs(case):
    """(left, right) of every content of a case."""
    return [make_content(c, case["h"], case["w"], case["Dd"], case["K"]) for c in CONTENTS]


_ORACLE = {}


def oracle_runs(oracle, ocfg, case):
    """[(left, right, map, intermediates)] of a case's contents: the oracle runs once per distinct pair and process."""
    if case["name"] not in _ORACLE:
        _ORACLE[case["name"]] = [(l, r) + tuple(oracle.run(ocfg, l, r, intermediates=True, volumes=True)) for l, r in case_pairs(case)]
    return _ORACLE[case["name"]]


def throughput_pairs(h, w, cus):
    """The smallest engine-stream call in the throughput shape (match_fast_plan: one workgroup of 24-row bands per CU)."""
    return -(-cus // (-(-w // (FA_VALID * 4)) * -(-h // FA_TH)))


if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(ROOT, "stereo-depth_amd"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import oracle_lib
    import stereo_synthetic as syn
    H, W, D, K = 375, 1242, 128, 2
    oracle = oracle_lib.get(parallel=True)
    ocfg = oracle_lib.OracleConfig(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
    total = None
    for i in [int(v) for v in sys.argv[1:]] or [0, 1, 2, 3, 17, 63]:
        left, right, _ = syn.make_pair(H, W, D, K, i)
        _, im = oracle.run(ocfg, left, right, intermediates=True)
        s = map_summary(im["wta_index"], D // K)
        print(f"pair {i}: windows {s['windows']}, both {s['both']}, upper only {s['upper']}, lower only {s['lower']}; second-pass rows "
              f"{s['rows_halves']} -> {s['rows_joint']} ({100.0 * (s['rows_halves'] - s['rows_joint']) / s['rows_halves']:.1f} % fewer); "
              f"marches full {s['full']}, half {s['half']}; leftover codes {s['codes']}")
        total = s if total is None else {k: ([a + b for a, b in zip(total[k], s[k])] if k == "codes" else total[k] + s[k]) for k in s}
    pass1 = total["windows"] * ((D // K + 1) // 2) * ROWS_FULL
    print(f"all: both {total['both']}, upper only {total['upper']}, lower only {total['lower']} in {total['windows']} windows; second-pass rows "
          f"{total['rows_halves']} -> {total['rows_joint']} ({100.0 * (total['rows_halves'] - total['rows_joint']) / total['rows_halves']:.1f} % fewer), "
          f"against {pass1} rows of pass 1: {100.0 * (total['rows_halves'] - total['rows_joint']) / (pass1 + total['rows_halves']):.2f} % of all marched rows")
