"""Generates the committed outputs OF THE REFERENCE ITSELF (README.md here has the schema):

    python -c "import __graft_entry__ as g; g.build()"        # builds oracle/_ref/libref_host.so from the reference tree
    python tests/golden/from_reference/make_from_reference.py [case ...]      # every case, or the named ones

The reference's own sources, compiled for the host against oracle/ref_host/ (oracle/build_ref.py), run on seeded
synthetic inputs with poison 0 in forward order; `out` and the stage buffers `gray_left`, `down_left`, `wta`, `refined`
are saved.  Built with -ffp-contract=off, so every file follows floating-point convention 0 (stereo_oracle.h).
Outside the validity masks the stored values are whatever a zero-filled torch::empty and in-order threads give;
nothing compares them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "stereo-depth_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import stereo_synthetic as syn        # noqa: E402

STAGES = ("gray_left", "down_left", "wta", "refined")

# name: (H, W, K, min_disparity, max_disparity, input kind, smallest share of pixels the full mask must keep[,
#        (ncc_patch_radius, sad_patch_radius, threshold, small_mbm_radius, mid_mbm_radius, large_mbm_radius)])
# Without the last entry the six fields are the reference's defaults and the file's `config` has 5 entries; with it, 11.
CASES = {
    "k1_48x64_d0_15_rgb_float": (48, 64, 1, 0, 15, "rgb_float", 0.35),
    "k1_32x48_d5_20_gray_int": (32, 48, 1, 5, 20, "gray_int", 0.35),
    "k2_64x96_d0_31_rgb_int": (64, 96, 2, 0, 31, "rgb_int", 0.35),
    "k2_64x96_d20_51_rgb_noise_float": (64, 96, 2, 20, 51, "rgb_noise_float", 0.35),
    "k2_96x160_d75_138_gray_float": (96, 160, 2, 75, 138, "gray_float", 0.35),
    "k3_72x96_d6_41_rgb_float": (72, 96, 3, 6, 41, "rgb_float", 0.35),
    "k4_96x128_d8_71_rgb_int": (96, 128, 4, 8, 71, "rgb_int", 0.35),
    "k2_65x96_d0_31_gray_int": (65, 96, 2, 0, 31, "gray_int", 0.20),
}
DEFAULT_FIELDS = sorted(CASES)
# the six fields away from their defaults; ncc_patch_radius >= 2 in the last three (safe rule S8 of stereo_oracle.h)
CASES.update({
    "k2_64x96_d0_31_rgb_float_r0_3_0_0_2_4": (64, 96, 2, 0, 31, "rgb_float", 0.35, (0, 3, 0, 0, 2, 4)),
    "k1_64x96_d4_27_gray_float_r1_8_11_3_8_12": (64, 96, 1, 4, 27, "gray_float", 0.35, (1, 8, 11, 3, 8, 12)),
    "k3_72x108_d6_41_rgb_float_r1_5_5_6_6_6": (72, 108, 3, 6, 41, "rgb_float", 0.35, (1, 5, 5, 6, 6, 6)),
    "k2_96x160_d0_31_gray_float_r2_3_2_2_3_5": (96, 160, 2, 0, 31, "gray_float", 0.35, (2, 3, 2, 2, 3, 5)),
    "k1_64x96_d5_36_gray_float_r2_6_3_3_3_8": (64, 96, 1, 5, 36, "gray_float", 0.35, (2, 6, 3, 3, 3, 8)),
    "k4_128x192_d8_71_gray_int_r3_4_8_0_1_4": (128, 192, 4, 8, 71, "gray_int", 0.35, (3, 4, 8, 0, 1, 4)),
})
ALL_FIELDS = [n for n in CASES if n not in DEFAULT_FIELDS]
# input seeds: the first eight keep the ones they were generated with, the later cases follow in the order above
SEEDS = {n: i for i, n in enumerate(DEFAULT_FIELDS + ALL_FIELDS)}


def _fraction(a, seed):
    """Adds a seeded fraction in [-0.5, 0.5) and keeps [0, 255]: float32 values off every integer grid."""
    rng = np.random.default_rng(syn.BASE_SEED + 90_000 + seed)
    return np.clip(a.astype(np.float64) + rng.uniform(-0.5, 0.5, a.shape), 0.0, 255.0).astype(np.float32)


def build_inputs(name):
    H, W, K, dmin, dmax, kind = CASES[name][:6]
    seed = SEEDS[name]
    D = dmax + 1
    if kind.startswith("rgb_noise"):
        pairs = [syn.make_noise_pair(H, W, 10 * seed + c) for c in range(3)]
        l, r = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    elif kind.startswith("rgb"):
        l, r = syn.random_rgb_pair(H, W, D, K, seed, dmin=dmin)
    else:
        l, r, _ = syn.make_pair(H, W, D, K, seed, dmin=dmin)
    if kind.endswith("float"):
        l, r = _fraction(l, 2 * seed), _fraction(r, 2 * seed + 1)
    return np.ascontiguousarray(l, np.float32), np.ascontiguousarray(r, np.float32)


def config_of(name):
    """The `config` array of a case's file: 5 entries, or all 11 in the order of stereo_matching_configuration.hh."""
    c = CASES[name]
    return np.array(c[:5] + (c[7] if len(c) > 7 else ()), np.int32)


def generate(name, ref, poison=0.0, reverse=False, volumes=False):
    """One case through the host build of the reference: the arrays of the committed file (volumes=True adds the
    aggregated cost volume `agg_volume`, which is too large to store)."""
    l, r = build_inputs(name)
    got = ref.run(config_of(name), l, r, poison=poison, reverse=reverse)
    z = dict(left=l, right=r, config=config_of(name), out=got["out"])
    z.update({k: got[k] for k in STAGES + (("agg_volume",) if volumes else ())})
    return z


def main():
    import build_ref
    ref = build_ref.RefHost()
    for name in (sys.argv[1:] or CASES):
        z = generate(name, ref)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **z)
        print(name, z["out"].shape, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
