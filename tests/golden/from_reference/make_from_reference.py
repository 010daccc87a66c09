"""Generates the committed outputs OF THE REFERENCE ITSELF (README.md here has the schema):

    python -c "import __graft_entry__ as g; g.build()"        # builds oracle/_ref/libref_host.so from the reference tree
    python tests/golden/from_reference/make_from_reference.py

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

# name: (H, W, K, min_disparity, max_disparity, input kind, smallest share of pixels the full mask must keep)
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


def _fraction(a, seed):
    """Adds a seeded fraction in [-0.5, 0.5) and keeps [0, 255]: float32 values off every integer grid."""
    rng = np.random.default_rng(syn.BASE_SEED + 90_000 + seed)
    return np.clip(a.astype(np.float64) + rng.uniform(-0.5, 0.5, a.shape), 0.0, 255.0).astype(np.float32)


def build_inputs(name):
    H, W, K, dmin, dmax, kind, _ = CASES[name]
    seed = sorted(CASES).index(name)
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
    return np.array(CASES[name][:5], np.int32)


def generate(name, ref, poison=0.0, reverse=False):
    """One case through the host build of the reference: the arrays of the committed file."""
    l, r = build_inputs(name)
    got = ref.run(config_of(name), l, r, poison=poison, reverse=reverse)
    z = dict(left=l, right=r, config=config_of(name), out=got["out"])
    z.update({k: got[k] for k in STAGES})
    return z


def main():
    import build_ref
    ref = build_ref.RefHost()
    for name in CASES:
        z = generate(name, ref)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **z)
        print(name, z["out"].shape, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
