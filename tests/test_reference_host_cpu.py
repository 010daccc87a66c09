"""The oracle against the REFERENCE'S OWN TEXT, run on the host (no GPU anywhere in this file).

oracle/build_ref.py compiles the reference's sources with g++ against the stand-in headers of oracle/ref_host/ into
oracle/_ref/libref_host.so; tests/golden/from_reference/*.npz are its outputs on seeded inputs.  Two groups:

  against the committed files (always run): the C oracle and its NumPy twin, under floating-point convention 0, equal
  `out`, `gray_left`, `down_left`, `wta`, `refined` BIT FOR BIT inside the validity masks, and the masks are not empty;

  against the live library (skipped, with the reason, where oracle/_ref/libref_host.so has not been built -- it needs
  the reference tree): the files are current; the masks lie inside the set of pixels that does not depend on what
  uninitialised and out-of-bounds memory holds or on the order in which threads run; a real compiler's own contractions
  are among the conventions; the stand-in runtime's barrier and accessor behave; for the cases under non-default radii
  and threshold the oracle's aggregated cost volume equals the library's inside the pooled mask, and a seeded sweep of
  configurations over all six of those fields finds no masked value unstable or different.

Figures of the run that produced the committed files (share of pixels; "stable" = bit-identical in all 8 runs of poison
{0, NaN, +1e30, -1e30} x order {forward, reverse}; mask and stable are those of `out`):

    case                               mask   stable  stable but unmasked
    k1_48x64_d0_15_rgb_float           0.686  0.804   0.118
    k1_32x48_d5_20_gray_int            0.554  0.697   0.143
    k2_64x96_d0_31_rgb_int             0.544  0.684   0.139
    k2_64x96_d20_51_rgb_noise_float    0.530  0.684   0.154
    k2_96x160_d75_138_gray_float       0.620  0.780   0.160
    k3_72x96_d6_41_rgb_float           0.392  0.557   0.166
    k4_96x128_d8_71_rgb_int            0.390  0.565   0.175
    k2_65x96_d0_31_gray_int            0.231  0.318   0.087

The six cases under non-default ncc / sad radii, threshold and aggregation radii (name suffix
_r<ncc>_<sad>_<threshold>_<small>_<mid>_<large>); "before S8" is what the masks without safe rule S8 (stereo_oracle.h)
gave on the same runs: their share, the masked values of `out` that are unstable, and the stable masked values of
`refined` / `out` where the oracle differs from the reference:

    case                                         mask   stable  stable but unmasked   before S8
    k2_64x96_d0_31_rgb_float_r0_3_0_0_2_4        0.716  0.871   0.155                 the same mask
    k1_64x96_d4_27_gray_float_r1_8_11_3_8_12     0.716  0.814   0.098                 the same mask
    k3_72x108_d6_41_rgb_float_r1_5_5_6_6_6       0.593  0.704   0.111                 the same mask
    k2_96x160_d0_31_gray_float_r2_3_2_2_3_5      0.558  0.761   0.203                 0.732, 1722 unstable, 1 / 3 differ
    k1_64x96_d5_36_gray_float_r2_6_3_3_3_8       0.589  0.729   0.140                 0.807, 878 unstable, 311 / 271 differ
    k4_128x192_d8_71_gray_int_r3_4_8_0_1_4       0.498  0.672   0.174                 0.728, 3257 unstable, 103 / 1618 differ
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

import build_ref
import oracle_lib
import stereo_numpy
import stereo_synthetic as syn
import test_from_reference as tfr
from oracle_lib import OracleConfig, fp_mixed

DIR = os.path.join(os.path.dirname(__file__), "golden", "from_reference")
_spec = importlib.util.spec_from_file_location("make_from_reference", os.path.join(DIR, "make_from_reference.py"))
mfr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mfr)

CASES = list(mfr.CASES)
ALL_STAGES = ("out",) + mfr.STAGES
POISONS = (0.0, float("nan"), 1e30, -1e30)
NEW_CASES = list(mfr.ALL_FIELDS)          # produced under non-default values of the six fields after max_disparity
FLOAT_RGB = [n for n in mfr.DEFAULT_FIELDS if mfr.CASES[n][5] in ("rgb_float", "rgb_noise_float")]

live = pytest.mark.skipif(not build_ref.RefHost.built(),
                          reason="oracle/_ref/libref_host.so is not built (build() makes it where the reference tree exists)")
live_fma = pytest.mark.skipif(not (build_ref.RefHost.built() and build_ref.RefHost.built(fma=True)),
                              reason="oracle/_ref/libref_host_fma.so is not built (needs the reference tree and a CPU with FMA)")


@functools.lru_cache(maxsize=None)
def _file(name):
    with np.load(os.path.join(DIR, name + ".npz")) as z:
        return tfr._Case({k: z[k] for k in z.files})


@functools.lru_cache(maxsize=None)
def _ref(fma=False):
    return build_ref.RefHost(fma=fma)


@functools.lru_cache(maxsize=None)
def _eight_runs(name):
    return [mfr.generate(name, _ref(), poison=p, reverse=rev) for p in POISONS for rev in (False, True)]


def _cfg(name, conv=0):
    return tfr.oracle_config(mfr.config_of(name), conv)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mask_for(a, md, mf):
    return mf if a.shape == mf.shape else md


def _assert_bitwise(name, who, got, want, md, mf):
    for st in ALL_STAGES:
        m = _mask_for(want[st], md, mf)
        bad = (_bits(got[st]) != _bits(want[st])) & m
        if bad.any():
            first = tuple(int(v) for v in np.argwhere(bad)[0])
            pytest.fail(f"{name}: {who} differs from the reference in stage {st}: {int(bad.sum())} of {int(m.sum())} masked "
                        f"values, first at {first}: {got[st][first]!r} vs {want[st][first]!r}")


# ---- against the committed files -------------------------------------------------------------------------------------
def test_the_committed_files_are_the_eight_cases():
    """... and the six produced under non-default fields, whose `config` has all eleven entries."""
    assert len(mfr.DEFAULT_FIELDS) == 8 and len(NEW_CASES) == 6
    have = sorted(os.path.basename(f)[:-4] for f in tfr.FILES)
    assert have == sorted(CASES)
    for name in CASES:
        z = _file(name)
        assert {"left", "right", "config", "out"} | set(mfr.STAGES) <= set(z)
        assert np.array_equal(z["config"], mfr.config_of(name))
        assert z["config"].size == (11 if name in NEW_CASES else 5)
        assert z["left"].ndim == (3 if mfr.CASES[name][5].startswith("rgb") else 2)
        integer = bool(np.all(z["left"] == np.rint(z["left"])) and np.all(z["right"] == np.rint(z["right"])))
        assert integer == mfr.CASES[name][5].endswith("int"), name


@pytest.mark.parametrize("name", CASES)
def test_no_comparison_passes_on_an_empty_mask(oracle, name):
    md, mf = oracle.masks(_cfg(name))
    assert mf.mean() >= mfr.CASES[name][6], f"{name}: the full mask keeps {mf.mean():.3f} of the pixels"
    assert md.any()


@pytest.mark.parametrize("name", CASES)
def test_classify_lists_convention_0(oracle, name):
    matching, report, _, _ = tfr.classify(_file(name), oracle)
    assert 0 in matching, report


@pytest.mark.parametrize("name", CASES)
def test_oracle_equals_the_reference_bitwise_inside_the_masks(oracle, name):
    z, cfg = _file(name), _cfg(name)
    md, mf = oracle.masks(cfg)
    out, im = oracle.run(cfg, z["left"], z["right"], intermediates=True)
    _assert_bitwise(name, "the C oracle", dict(im, out=out), z, md, mf)


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_equals_the_reference_bitwise_inside_the_masks(oracle, name):
    z, cfg = _file(name), _cfg(name)
    md, mf = oracle.masks(cfg)
    out, im = stereo_numpy.run(cfg, z["left"], z["right"])
    _assert_bitwise(name, "the NumPy restatement", dict(im, out=out), z, md, mf)


def test_rule_s7_takes_the_pixels_whose_lookups_reach_undefined_costs(oracle):
    """dmin > 0: a pixel's Q5 lookups reach ceil(dmin / Dd) pixels back in row-major order, so a pixel is in the mask
    only if those lie where the aggregated costs are defined (S7).  A pixel's predecessors in its own row are defined
    when it is; those of the first columns are the previous row's tail, which never is (y + L > w).  So the mask is that
    of the same range starting at 0, without its first ceil(dmin / Dd) columns -- and dmin = 0 loses nothing.  (The
    cases at the reference's default radii; test_masks_for_ncc_radius_of_2_and_more_only_shrink has S7 under S8.)"""
    seen = set()
    for name in mfr.DEFAULT_FIELDS:
        cfg = _cfg(name)
        md, _ = oracle.masks(cfg)
        d = oracle.dims(cfg)
        back = -(-d.dmin // d.Dd) if d.dmin > 0 else 0
        seen.add(back)
        twin = _cfg(name)
        twin.min_disparity = 0
        md0, _ = oracle.masks(twin)
        assert md0[:, 0].any(), name
        assert np.array_equal(md, md0 & (np.arange(d.w)[None, :] >= back)), name
    assert seen == {0, 1, 2}


def test_a_mixed_convention_is_two_plain_ones(oracle):
    """SO_FP_MIXED(s, p): step 1 as under s, the parabola as under p -- C oracle and NumPy twin alike."""
    name = "k2_64x96_d20_51_rgb_noise_float"
    z = _file(name)
    runs = {c: oracle.run(_cfg(name, c), z["left"], z["right"], intermediates=True) for c in (2, 3, fp_mixed(3, 2), fp_mixed(3, 3))}
    mixed = runs[fp_mixed(3, 2)]
    assert np.array_equal(_bits(mixed[1]["gray_left"]), _bits(runs[3][1]["gray_left"]))
    assert not np.array_equal(_bits(mixed[1]["gray_left"]), _bits(runs[2][1]["gray_left"]))
    assert not np.array_equal(_bits(mixed[1]["refined"]), _bits(runs[3][1]["refined"]))       # the parabola is not 3's
    assert np.array_equal(_bits(runs[fp_mixed(3, 3)][0]), _bits(runs[3][0]))
    out, im = stereo_numpy.run(_cfg(name, fp_mixed(3, 2)), z["left"], z["right"])
    assert np.array_equal(_bits(out), _bits(mixed[0]))
    for st in mfr.STAGES:
        assert np.array_equal(_bits(im[st]), _bits(mixed[1][st])), st
    bad = _cfg(name, 6 | (1 << 3))
    with pytest.raises(RuntimeError):
        oracle.dims(bad)


# ---- the masks under ncc_patch_radius (safe rule S8) -----------------------------------------------------------------
def _masks_restated(cfg, d, s8):
    """so_validity_masks restated in NumPy: the formula of S1-S7 as it stood before S8 (s8=False), and with S8 in its
    closed form (s8=True: for r >= 2 the aggregated costs are defined only for L <= x, x + L + r <= h, L <= y,
    y + L + r <= w).  The C function derives S8 another way (it marks the cost rows and columns that pad_index sends
    out of the image and every window that reaches one), so the two check each other."""
    H, W, K, h, w = d.H, d.W, d.K, d.h, d.w
    r, R, L = cfg.ncc_patch_radius, cfg.sad_patch_radius, cfg.large_mbm_radius
    md = np.zeros((h, w), bool)
    if W % K == 0 and d.dmax + r <= w and L + r < h and L + r < w:
        x, y = np.arange(h)[:, None], np.arange(w)[None, :]
        row_taint = np.zeros(h, bool)
        if H % K:
            for i in range(-(L + r), L + r + 1):
                row_taint |= (np.arange(h) + i) % h == h - 1
        agg_ok = ~row_taint[:, None] & (x + L <= h) & (y + L <= w)
        if s8 and r >= 2:
            agg_ok &= (x >= L) & (x + L + r <= h) & (y >= L) & (y + L + r <= w)
        md = agg_ok & (x * K + R <= H) & (y * K + R + K <= W)
        pix = x * w + y
        if d.dmin > 0:
            md &= pix * d.Dd - d.dmin >= 0
            for b in range(1, -(-d.dmin // d.Dd) + 1):
                md &= agg_ok.ravel()[np.maximum(pix - b, 0)]       # pix - b >= 0 wherever md still holds
    mf = np.zeros((H, W), bool)
    c0 = np.arange(W) // K
    live = c0 * K + K < W
    c0, c1 = np.where(live, c0, 0), np.where(live, c0 + 1, 0)
    for X in range(H):
        x, i = divmod(X, K)
        if (x == 0 and i > 0) or (i > 0 and (K + 1) * x >= H):
            continue
        mf[X] = live & md[x, c0] & md[x, c1]
        if i > 0:
            mf[X] &= md[x - 1, c0] & md[x - 1, c1]
    return md, mf


def _mask_configs(n, ncc_values, seed):
    """Seeded configurations over all eleven fields, small enough that most masks are not empty and some are."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        K = int(rng.integers(1, 5))
        r = int(rng.choice(ncc_values))
        L = int(rng.integers(0, 13))
        h = int(rng.integers(max(8, L + r + 1), 2 * (L + r) + 30))
        w = int(rng.integers(max(8, L + r + 1), 2 * (L + r) + 40))
        H = h * K - (int(rng.integers(0, K)) if rng.random() < 0.3 else 0)
        W = w * K - (int(rng.integers(0, K)) if rng.random() < 0.1 else 0)
        dmin = int(rng.integers(0, 3 * K * 8)) if rng.random() < 0.5 else 0
        dmax = dmin + int(rng.integers(0, K * 16))
        yield OracleConfig(height=H, width=W, downscale_factor=K, min_disparity=dmin, max_disparity=dmax,
                           ncc_patch_radius=r, sad_patch_radius=int(rng.integers(0, 9)), threshold=int(rng.integers(0, 12)),
                           small_mbm_radius=int(rng.integers(0, L + 1)), mid_mbm_radius=int(rng.integers(0, L + 1)),
                           large_mbm_radius=L)


def test_masks_for_ncc_radius_up_to_1_are_what_they_were(oracle):
    """S8 is empty for ncc_patch_radius <= 1: over 120 seeded configurations the masks equal, pixel for pixel, the
    formula of S1-S7 restated in NumPy."""
    kept = empty = 0
    for cfg in _mask_configs(120, (0, 1), 8801):
        md, mf = oracle.masks(cfg)
        want_md, want_mf = _masks_restated(cfg, oracle.dims(cfg), s8=False)
        assert np.array_equal(md, want_md) and np.array_equal(mf, want_mf), cfg
        kept += bool(mf.any())
        empty += not md.any()
    assert kept >= 50 and empty >= 5, (kept, empty)


def test_masks_for_ncc_radius_of_2_and_more_only_shrink(oracle):
    """ncc_patch_radius >= 2: the masks equal the formula of S1-S7 with S8's closed form on the aggregated costs, lie
    inside the masks of S1-S7 alone, and lose something nearly wherever those kept anything (not always: the SAD radius
    or the S7 columns may have taken the same pixels already).  S7 under S8: with dmin > 0 the
    first ceil(dmin / Dd) kept columns go as well (their predecessors are columns < L, which S8 takes)."""
    kept = lost = with_back = 0
    for cfg in _mask_configs(120, (2, 3, 4, 5, 8), 8802):
        md, mf = oracle.masks(cfg)
        d = oracle.dims(cfg)
        want_md, want_mf = _masks_restated(cfg, d, s8=True)
        assert np.array_equal(md, want_md) and np.array_equal(mf, want_mf), cfg
        old_md, old_mf = _masks_restated(cfg, d, s8=False)
        assert not (md & ~old_md).any() and not (mf & ~old_mf).any(), cfg
        lost += bool((old_md & ~md).any())
        kept += bool(mf.any())
        if md.any() and d.dmin > 0:
            back = -(-d.dmin // d.Dd)
            assert int(np.flatnonzero(md.any(axis=0))[0]) == cfg.large_mbm_radius + back, cfg
            with_back += 1
    assert kept >= 50 and lost >= kept and with_back >= 10, (kept, lost, with_back)


# ---- against the live library ----------------------------------------------------------------------------------------
@live
@pytest.mark.parametrize("name", CASES)
def test_the_committed_files_are_current(name):
    z, fresh = _file(name), _eight_runs(name)[0]                   # poison 0, forward order
    assert set(z) == set(fresh)
    for k in fresh:
        assert z[k].dtype == fresh[k].dtype and np.array_equal(_bits(z[k]) if z[k].dtype == np.float32 else z[k],
                                                                _bits(fresh[k]) if z[k].dtype == np.float32 else fresh[k]), (name, k)


@live
@pytest.mark.parametrize("name", CASES)
def test_the_masks_lie_inside_the_stable_set(oracle, name):
    """The oracle's claim that the reference is DEFINED inside the masks: there no value may depend on what torch::empty
    left in memory (body, guard bands, shared memory) nor on the order of blocks and threads.  Not the converse: the
    masks are conservative, and by how much is printed (and tabulated in the module docstring and DESIGN.md section 5)."""
    runs = _eight_runs(name)
    md, mf = oracle.masks(_cfg(name))
    for st in ALL_STAGES:
        first = _bits(runs[0][st])
        stable = np.ones(first.shape, bool)
        for r in runs[1:]:
            stable &= _bits(r[st]) == first
        m = _mask_for(first, md, mf)
        print(f"{name} {st}: mask {m.mean():.3f} stable {stable.mean():.3f} stable-but-unmasked {(stable & ~m).mean():.3f}")
        escaped = m & ~stable
        assert not escaped.any(), (f"{name}: stage {st}: {int(escaped.sum())} masked values depend on uninitialised memory or "
                                   f"thread order, first at {tuple(int(v) for v in np.argwhere(escaped)[0])}")
    if mfr.CASES[name][5].startswith("gray"):
        assert np.array_equal(_bits(runs[0]["gray_left"]), _bits(runs[0]["left"]))


@live
@pytest.mark.parametrize("name", NEW_CASES)
def test_aggregated_costs_equal_the_reference_inside_the_pooled_mask(oracle, name):
    """The files hold no agg_volume (too large); live, the oracle's equals the reference's at every disparity of every
    pooled pixel of the pooled mask.  This is the buffer S8 is about: wta and refined can agree where costs differ."""
    fresh = mfr.generate(name, _ref(), volumes=True)
    cfg = _cfg(name)
    md, _ = oracle.masks(cfg)
    _, im = oracle.run(cfg, fresh["left"], fresh["right"], intermediates=True, volumes=True)
    bad = (_bits(im["agg_volume"]) != _bits(fresh["agg_volume"])).any(axis=2) & md
    assert md.any()
    assert not bad.any(), (f"{name}: the aggregated costs of {int(bad.sum())} of {int(md.sum())} masked pooled pixels differ, "
                           f"first at {tuple(int(v) for v in np.argwhere(bad)[0])}")


def _sweep_configs(n=18, seed=8803):
    """Seeded configurations over all six fields after max_disparity: ncc 0..4, sad 1..8, threshold 0..11, small and
    mid <= large in 2..12; K in 1..4, H % K != 0 and dmin > 0 sometimes; large + ncc below both pooled dimensions and
    dmax / K + ncc at most the pooled width; images of 40-130 pixels a side."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        K = int(rng.integers(1, 5))
        r = int(rng.integers(0, 5))
        side = 130 // K                                            # largest pooled side
        L = int(rng.integers(2, min(12, (side - 6) // 2 - r) + 1))
        ragged = K > 1 and rng.random() < 0.35                     # H % K != 0 taints the L + r rows around the last one
        dmin_p = int(rng.integers(1, 7)) if i % 2 else 0            # dmin > 0 in every other one
        dd_p = int(rng.integers(6, 17))
        h = int(rng.integers(max(2 * (L + r) + 6, -(-40 // K)), side + 1))
        w_low = max(2 * L + r + 8, dmin_p + dd_p + r, -(-40 // K))
        w = int(rng.integers(w_low, max(w_low, side) + 1))
        H = h * K - (int(rng.integers(1, K)) if ragged else 0)
        dmin = dmin_p * K + (int(rng.integers(0, K)) if dmin_p else 0)
        dmax = (dmin_p + dd_p - 1) * K + int(rng.integers(0, K))
        out.append((H, w * K, K, dmin, dmax, r, int(rng.integers(1, 9)), int(rng.integers(0, 12)),
                    int(rng.integers(0, L + 1)), int(rng.integers(0, L + 1)), L))
    return out


SWEEP = _sweep_configs()


def test_the_sweep_covers_what_it_says():
    assert len(SWEEP) >= 16
    assert {c[5] for c in SWEEP} == {0, 1, 2, 3, 4} and sum(c[5] >= 2 for c in SWEEP) >= 6
    assert {c[2] for c in SWEEP} == {1, 2, 3, 4}
    assert any(c[0] % c[2] for c in SWEEP) and sum(c[3] > 0 for c in SWEEP) == len(SWEEP) // 2
    for H, W, K, dmin, dmax, r, R, thr, small, mid, L in SWEEP:
        h, w = -(-H // K), W // K
        assert 37 <= H <= 130 and 40 <= W <= 136 and W % K == 0, (H, W)
        assert L + r < h and L + r < w and dmax // K + r <= w and small <= L and mid <= L and 2 <= L <= 12


@live
@pytest.mark.parametrize("config", SWEEP, ids=["-".join(str(v) for v in c) for c in SWEEP])
def test_sweep_of_all_six_fields_against_the_live_reference(oracle, config):
    """Four runs of the reference (poison 0, NaN, +1e30, -1e30; order forward, reverse, forward, reverse) on a seeded
    gray pair with fractional samples: inside the masks no value may move between the runs, and the oracle equals them
    bit for bit in out, down_left, wta, refined and, at the pooled mask, the whole aggregated cost volume."""
    cfg = tfr.oracle_config(config)
    H, W, K = config[:3]
    seed = SWEEP.index(config)
    l, r = syn.make_pair(H, W, config[4] + 1, K, 500 + seed, dmin=config[3])[:2]
    l, r = mfr._fraction(l, 1000 + seed), mfr._fraction(r, 2000 + seed)
    runs = [_ref().run(config, l, r, poison=p, reverse=rev) for p, rev in zip(POISONS, (False, True, False, True))]
    md, mf = oracle.masks(cfg)
    assert md.any() and mf.any(), "empty mask"
    out, im = oracle.run(cfg, l, r, intermediates=True, volumes=True)
    got = dict(im, out=out)
    for st in ("out", "down_left", "wta", "refined", "agg_volume"):
        first = _bits(runs[0][st])
        moved = np.zeros(first.shape, bool)
        for run in runs[1:]:
            moved |= _bits(run[st]) != first
        differs = _bits(got[st]) != first
        if st == "agg_volume":
            moved, differs = moved.any(axis=2), differs.any(axis=2)
        m = mf if st == "out" else md
        print(f"{config} {st}: mask {m.mean():.3f} stable {1 - moved.mean():.3f}")
        assert not (moved & m).any(), f"stage {st}: {int((moved & m).sum())} of {int(m.sum())} masked values depend on poison or order"
        assert not (differs & m).any(), f"stage {st}: {int((differs & m).sum())} of {int(m.sum())} masked values differ from the reference"


@live_fma
@pytest.mark.parametrize("name", FLOAT_RGB)
def test_a_real_compilers_contractions_are_among_the_conventions(oracle, name):
    """libref_host_fma.so is the reference's text under g++ -O2 -mfma -ffp-contract=fast: a real compiler choosing which
    products to fuse.  Some convention must reproduce it bit for bit.  gcc 11 fuses step 1 as FMA_OUTER and the parabola
    as FMA_SECOND, which no plain convention expresses: k2_64x96_d20_51_rgb_noise_float and k3_72x96_d6_41_rgb_float
    matched none of the six before SO_FP_MIXED existed (k1_48x64_d0_15_rgb_float matched FMA_OUTER: its parabola is
    insensitive).  This says nothing about nvcc's own choice."""
    assert len(FLOAT_RGB) == 3
    z = tfr._Case(mfr.generate(name, _ref(fma=True)))
    assert not np.array_equal(_bits(z["gray_left"]), _bits(_file(name)["gray_left"])), "the FMA build contracted nothing"
    matching, report, _, _ = tfr.classify(z, oracle)
    print(name, "FMA build follows", [oracle_lib.fp_name(c) for c in matching])
    assert matching, report


@live
@pytest.mark.parametrize("reverse", [False, True])
def test_runner_barrier_orders_shared_memory(reverse):
    """Every thread reads the slot its cyclic right-hand neighbour wrote before the barrier; threads past n leave before
    it.  With the barrier every value is the neighbour's; the same kernel WITHOUT the barrier reads unwritten (poison)
    slots, so this check cannot pass on a barrier that does nothing."""
    import ctypes as C
    lib = _ref().lib
    blocks, tx, ty, n, poison = 3, 4, 8, 27, -7.0
    per = tx * ty

    def run(with_barrier):
        out = np.zeros((blocks, per), np.float32)
        assert lib.ref_host_selfcheck_barrier(blocks, tx, ty, n, int(with_barrier), poison, int(reverse),
                                              out.ctypes.data_as(C.POINTER(C.c_float))) == 0
        return out

    want = np.full((blocks, per), poison, np.float32)
    for b in range(blocks):
        for t in range(n):
            want[b, t] = 1000 * (b + 1) + (t + 1) % n
    assert np.array_equal(run(True), want)
    racy = run(False)
    assert np.array_equal(racy[:, n:], want[:, n:])
    wrong = racy[:, :n] != want[:, :n]
    # forward: only the last thread finds its neighbour (slot 0) written; reverse: only thread n-1 (reads slot 0) does not
    assert int(wrong.sum()) == (blocks * (n - 1) if not reverse else blocks)
    assert np.all(racy[:, :n][wrong] == np.float32(poison))


@live
def test_accessor_wraps_a_negative_index_into_the_guard_band():
    lib = _ref().lib
    rows, cols = 5, 7
    assert lib.ref_host_selfcheck_read(rows, cols, 2, 3, 9.5) == 2 * cols + 3 + 1
    assert lib.ref_host_selfcheck_read(rows, cols, -1, 0, 9.5) == 9.5            # a whole row before the base: poison
    assert lib.ref_host_selfcheck_read(rows, cols, 0, -1, 9.5) == 9.5
    assert lib.ref_host_selfcheck_read(rows, cols, 1, -1, 9.5) == cols           # last element of row 0, as on the device
    assert lib.ref_host_selfcheck_read(rows, cols, rows, 0, 9.5) == 9.5          # the guard after the body
    assert np.isnan(lib.ref_host_selfcheck_read(rows, cols, -2, 1, float("nan")))
    assert lib.ref_host_selfcheck_types() == 7       # -1 >= size() in size_t; unsigned indices; size_t / int64_t sizes


def test_the_recipe_refuses_a_rewrite_that_misses():
    """A launch or a shared-memory declaration the rewrite does not match would be compiled away silently."""
    launch = "k<scalar_t><<<g, b>>>(x);"
    assert "<<<" not in build_ref.rewrite(launch, 1, 0, "t")
    assert "refhost::launch(refhost::launch_cfg(g, b, n * sizeof(scalar_t)), k<scalar_t>, x);" == \
        build_ref.rewrite("k<scalar_t><<<g, b, n * sizeof(scalar_t)>>>(x);", 1, 0, "t")
    for text, counts in ((launch, (2, 0)), (launch + launch, (1, 0)), ("k<<<g, b>>>(x);", (1, 0)), (launch, (1, 1)),
                         ("extern __shared__ float s[];", (0, 0)), ("extern __shared__ float s[4];", (0, 1))):
        with pytest.raises(RuntimeError):
            build_ref.rewrite(text, counts[0], counts[1], "t")
    assert build_ref.rewrite("extern __shared__ __align__(sizeof(T)) unsigned char raw[];", 0, 1, "t") == \
        "unsigned char* raw = static_cast<unsigned char*>(refhost::block_shared());"
