"""The oracle against the REFERENCE'S OWN TEXT, run on the host (no GPU anywhere in this file).

oracle/build_ref.py compiles the reference's sources with g++ against the stand-in headers of oracle/ref_host/ into
oracle/_ref/libref_host.so; tests/golden/from_reference/*.npz are its outputs on seeded inputs.  Two groups:

  against the committed files (always run): the C oracle and its NumPy twin, under floating-point convention 0, equal
  `out`, `gray_left`, `down_left`, `wta`, `refined` BIT FOR BIT inside the validity masks, and the masks are not empty;

  against the live library (skipped, with the reason, where oracle/_ref/libref_host.so has not been built -- it needs
  the reference tree): the files are current; the masks lie inside the set of pixels that does not depend on what
  uninitialised and out-of-bounds memory holds or on the order in which threads run; a real compiler's own contractions
  are among the conventions; the stand-in runtime's barrier and accessor behave.

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
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

import build_ref
import oracle_lib
import stereo_numpy
import test_from_reference as tfr
from oracle_lib import OracleConfig, fp_mixed

DIR = os.path.join(os.path.dirname(__file__), "golden", "from_reference")
_spec = importlib.util.spec_from_file_location("make_from_reference", os.path.join(DIR, "make_from_reference.py"))
mfr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mfr)

CASES = list(mfr.CASES)
ALL_STAGES = ("out",) + mfr.STAGES
POISONS = (0.0, float("nan"), 1e30, -1e30)
FLOAT_RGB = [n for n in CASES if mfr.CASES[n][5] in ("rgb_float", "rgb_noise_float")]

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
    H, W, K, dmin, dmax = mfr.CASES[name][:5]
    return OracleConfig(height=H, width=W, downscale_factor=K, min_disparity=dmin, max_disparity=dmax, fp_convention=conv)


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
    have = sorted(os.path.basename(f)[:-4] for f in tfr.FILES)
    assert have == sorted(CASES)
    for name in CASES:
        z = _file(name)
        assert {"left", "right", "config", "out"} | set(mfr.STAGES) <= set(z)
        assert np.array_equal(z["config"], mfr.config_of(name))
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
    of the same range starting at 0, without its first ceil(dmin / Dd) columns -- and dmin = 0 loses nothing."""
    seen = set()
    for name in CASES:
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
