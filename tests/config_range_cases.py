"""The configuration-range cases shared by tests/test_config_range_cpu.py and tests/test_config_range_gpu.py.

smx_create accepts ncc_patch_radius up to 16, sad_patch_radius and large_mbm_radius up to 32 (as far as the 64 KB LDS tile
of the generic exact-order kernel allows), downscale_factor up to 64, any threshold and any disparity range; the other
parity files stay in a corner of that space.  This list walks the rest of it.  Every case names the code it is aimed at:

  chunks    k_match_exact.h with several right-tile chunks (the `for d0 ... += nd_max` loop: cbase, roff, the rcols_max
            pitch of a short last chunk), also on the volume route (WRITE_VOL);
  boundary  the largest radii whose tile fits, degenerate radii, one disparity;
  K         the generic prologue, the generic float step 6 and k_fill<false> / k_fill<true> beyond K in {1, 2, 3, 4, 8};
  step6     the generic float step 6 (`kt == 0`) at SAD radii up to 32, windows wider than the image, and the fills at the
            ends of the threshold's range;
  sweep     24 seeded random cases over all of it.

Plain data and seeded inputs: no torch, no GPU.  The CPU file keeps the list honest (the planner's facts per case from
tests/config_range_harness.cpp, the oracle against its NumPy twin, the non-vacuity conditions); the GPU file compares the
HIP path with the oracle on exactly these cases."""
import os
import subprocess
from dataclasses import dataclass, field, replace

import numpy as np

import stereo_synthetic as syn
from parity_inputs import odd_disparity_pair, float_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "config_range_harness.cpp")

DEFAULTS = dict(ncc_patch_radius=1, sad_patch_radius=5, threshold=5, small_mbm_radius=1, mid_mbm_radius=4, large_mbm_radius=10)


def R(rn, sad, thr, rs, rm, rl):
    """The six radius and threshold fields, in the order of the configuration struct."""
    return dict(ncc_patch_radius=rn, sad_patch_radius=sad, threshold=thr, small_mbm_radius=rs, mid_mbm_radius=rm,
                large_mbm_radius=rl)


@dataclass(frozen=True)
class Case:
    id: str
    H: int
    W: int
    K: int
    dmin: int                   # min_disparity / max_disparity at full resolution
    dmax: int
    extra: dict = field(default_factory=dict)      # configuration fields that differ from DEFAULTS
    kind: str = "odd"           # input builder: synthetic / odd / float / rgb / slanted / shifted / shifted_rgb
    seed: int = 1
    group: str = "boundary"     # chunks / boundary / K / step6 / sweep
    aims: tuple = ()            # "chunks": exact_nd < Dd; "step6": generic float step 6 that moves values; "K": generic K
    exact_nd: int = 0           # expected disparities per right-tile chunk (0: not stated)
    volume: bool = False        # expected on the volume route (aggregated volume materialised)
    columns: bool = False       # inputs(): the disparity levels lie in column bands (column_band_pair)

    @property
    def fields(self):
        return dict(DEFAULTS, **self.extra)

    def config_kwargs(self):
        return dict(height=self.H, width=self.W, downscale_factor=self.K, min_disparity=self.dmin, max_disparity=self.dmax,
                    **self.extra)

    @property
    def pooled(self):
        K = self.K
        return (self.H + K - 1) // K, (self.W + K - 1) // K, self.dmin // K, self.dmax // K - self.dmin // K + 1


# ----------------------------------------------------------------------------------------------------------------- inputs
def shifted_noise_pair(H, W, shifts, seed, noise=3):
    """A noise texture and, in horizontal bands of the right image, the same texture shifted cyclically by the band's
    constant, plus sensor noise; the last band of the right image is independent noise.  Integer-valued in 0..255.  With
    shifts that are no multiples of K the full-resolution winner of step 6 sits strictly between the candidates' ends
    on most pixels, so step 6 moves them; in the noise band no disparity is better than another, so the arg-max lands
    anywhere in the range whatever the radii."""
    rng = np.random.default_rng(90_000 + seed)
    left = rng.integers(0, 256, (H, W)).astype(np.float64)
    acc = np.zeros_like(left)
    for j in (-1, 0, 1):
        acc += np.roll(left, j, axis=1)
    left = np.rint(acc / 3.0)
    right = rng.integers(0, 256, (H, W)).astype(np.float64)
    edges = np.linspace(0, H, len(shifts) + 2).astype(int)
    for b, shift in enumerate(shifts):
        right[edges[b]:edges[b + 1]] = np.roll(left, -int(shift), axis=1)[edges[b]:edges[b + 1]]
    right[:edges[-2]] = np.clip(right[:edges[-2]] + rng.integers(-noise, noise + 1, (edges[-2], W)), 0, 255)
    return left.astype(np.float32), right.astype(np.float32)


def band_levels(case):
    """min(4, Dd) true disparities at full resolution, spread over the range: pooled disparity d as d * K + 1 for K >= 3
    (nearest to d after pooling, and no multiple of K), d * K otherwise; only those inside [min_disparity, max_disparity]
    where that leaves enough of them."""
    _, _, dmin, Dd = case.pooled
    K, n = case.K, min(4, Dd)
    full = [d * K + (1 if K >= 3 else 0) for d in range(dmin, dmin + Dd)]
    valid = [g for g in full if case.dmin <= g <= case.dmax]
    if len(valid) < n:
        valid = [min(max(g, case.dmin), case.dmax) for g in full]
    return [valid[(len(valid) * (2 * k + 1)) // (2 * n)] for k in range(n)]


def column_band_pair(case):
    """The left image of the case's builder and a right image whose true disparity is constant per COLUMN band
    (band_levels), with the builder's kind of noise.  Aggregation boxes that span most of the pooled rows average row
    bands away; column bands wider than the large radius keep one winner each, so the arg-max still takes several
    values."""
    rng = np.random.default_rng(92_000 + case.seed)
    left = inputs(replace(case, columns=False))[0]
    W = case.W
    levels = band_levels(case)
    edges = np.linspace(0, W, len(levels) + 1).astype(int)
    right = np.empty_like(left)
    for b, g in enumerate(levels):
        cols = np.arange(edges[b], edges[b + 1])
        right[..., cols] = left[..., (cols + g) % W]
    amp = {"synthetic": 1, "rgb": 1, "shifted": 3, "shifted_rgb": 3}.get(case.kind, 6)
    noise = rng.integers(-amp, amp + 1, right.shape).astype(np.float32)
    if case.kind == "float":
        noise = noise + rng.random(right.shape).astype(np.float32) * np.float32(0.9)
        return left, (right + noise).astype(np.float32)
    return left, np.clip(np.rint(right) + noise, 0, 255).astype(np.float32)


def _shifts(case):
    """Two true disparities inside the range, at about a third and two thirds of it, that are no multiples of K."""
    out = []
    for f in (1, 2):
        s = case.dmin + ((case.dmax - case.dmin) * f) // 3
        if case.K > 1 and s % case.K == 0:
            s += 1
        out.append(min(max(s, case.dmin), case.dmax))
    return out


def inputs(case):
    """(left, right) float32: [H, W] gray or [3, H, W] RGB, seeded by the case."""
    H, W, K, D, seed = case.H, case.W, case.K, case.dmax + 1, case.seed
    if case.columns:
        return column_band_pair(case)
    if case.kind == "synthetic":
        return syn.make_pair(H, W, D, K, seed, dmin=case.dmin)[:2]
    if case.kind == "odd":
        return odd_disparity_pair(H, W, D, seed=seed)
    if case.kind == "float":
        return float_pair(H, W, D, seed=seed)
    if case.kind == "rgb":
        return syn.random_rgb_pair(H, W, D, K, seed, dmin=case.dmin)
    if case.kind == "slanted":
        return syn.make_slanted_pair(H, W, D, K, seed)[:2]
    if case.kind == "shifted":
        return shifted_noise_pair(H, W, _shifts(case), seed)
    if case.kind == "shifted_rgb":
        chans = [shifted_noise_pair(H, W, _shifts(case), 3 * seed + c) for c in range(3)]
        return np.stack([c[0] for c in chans]), np.stack([c[1] for c in chans])
    raise ValueError(case.kind)


def integer_inputs(case, rgb, index=0):
    """Integer-valued inputs in 0..255 for the u8 entries (and their f32 twins): gray [H, W] or RGB [3, H, W]."""
    H, W, K, D = case.H, case.W, case.K, case.dmax + 1
    if rgb:                                        # three channels with the same odd disparities and their own textures
        chans = [odd_disparity_pair(H, W, D, seed=200 + 3 * (case.seed + index) + c) for c in range(3)]
        return np.stack([c[0] for c in chans]), np.stack([c[1] for c in chans])
    return odd_disparity_pair(H, W, D, seed=300 + case.seed + index)


def batch_inputs(case, n):
    """n distinct pairs of the case's kind."""
    pairs = [inputs(replace(case, seed=case.seed + 17 * (i + 1))) for i in range(n)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


# ------------------------------------------------------------------------------------------------------------ fixed cases
CHUNK_CASES = [
    # the largest accepted tile (65,296 of 65,536 bytes): 14 chunks of 3 disparities, the last of one
    Case("rl18_chunks3", 80, 180, 2, 0, 79, R(1, 5, 5, 7, 12, 18), "odd", group="chunks", aims=("chunks",), exact_nd=3),
    Case("Dd400_two_chunks", 24, 520, 1, 0, 399, R(2, 3, 2, 2, 3, 5), "odd", group="chunks", aims=("chunks",), exact_nd=200),
    Case("rn4_rl14", 36, 150, 2, 0, 139, R(4, 9, 3, 0, 14, 14), "rgb", group="chunks", aims=("chunks",), exact_nd=35),
    # default radii, min_disparity / K beyond the disparity count: the volume route of the generic kernel
    Case("vol_default_chunks", 24, 420, 1, 200, 389, {}, "synthetic", group="chunks", aims=("chunks",), exact_nd=95, volume=True),
    Case("vol_rl17_chunks", 60, 200, 2, 20, 99, R(1, 4, 3, 2, 9, 17), "synthetic", group="chunks", aims=("chunks",), exact_nd=20,
         volume=True),
]

BOUNDARY_CASES = [
    Case("rn8", 60, 120, 2, 4, 67, R(8, 5, 5, 0, 10, 10), "rgb", volume=True),
    Case("all_zero_radii", 50, 90, 2, 0, 31, R(0, 0, 0, 0, 0, 0), "odd"),
    Case("Dd1", 40, 70, 2, 6, 7, {}, "odd", volume=True),
]

# pooled images of 5 x 11 and 1 x 11 pixels: under the default radii every box covers the whole image and one disparity wins
# everywhere; boxes of a few pixels keep a winner per column band
SMALL_BOXES = R(1, 5, 5, 0, 1, 2)

K_CASES = [
    Case("K5_float", 99, 183, 5, 0, 59, {}, "float", seed=2, group="K", aims=("step6", "K")),
    Case("K7_rgb", 100, 180, 7, 7, 90, {}, "shifted_rgb", group="K", aims=("step6", "K"), columns=True),
    Case("K16", 199, 331, 16, 0, 127, {}, "shifted", group="K", aims=("step6", "K")),
    Case("K64", 300, 700, 64, 0, 255, SMALL_BOXES, "shifted", group="K", aims=("step6", "K"), columns=True),
    # pooled image one row high; the seed at which each of the four bands (under three pooled columns wide) keeps its winner
    Case("K64_h1", 50, 700, 64, 0, 255, SMALL_BOXES, "shifted", seed=3, group="K", aims=("step6", "K"), columns=True),
]

STEP6_CASES = [
    Case("sad32", 72, 160, 2, 0, 31, dict(sad_patch_radius=32), "slanted", group="step6", aims=("step6",)),
    # 65-wide window on a 60-wide image: every window row wraps more than once
    Case("sad32_narrow", 44, 60, 2, 0, 15, dict(sad_patch_radius=32), "shifted", group="step6", aims=("step6",)),
    Case("K5_sad12_dmin", 100, 180, 5, 10, 74, dict(sad_patch_radius=12), "shifted", group="step6", aims=("step6", "K")),
    Case("sad0", 60, 110, 2, 0, 31, dict(sad_patch_radius=0), "slanted", group="step6", aims=("step6",)),
    Case("thr0", 62, 111, 3, 0, 35, dict(threshold=0), "shifted", group="step6", aims=("step6",)),
    Case("thr1e6", 62, 111, 3, 0, 35, dict(threshold=1_000_000), "shifted", group="step6", aims=("step6",)),
]

FIXED_CASES = CHUNK_CASES + BOUNDARY_CASES + K_CASES + STEP6_CASES

# the cases whose u8 gray and u8 RGB entries run too, and the ones that run as batches
ENTRY_CASE_IDS = ("K5_float", "K7_rgb", "K16", "K64", "sad32", "rl18_chunks3")
BATCH_CASE_IDS = ("rl18_chunks3", "vol_default_chunks", "K7_rgb")


# ---------------------------------------------------------------------------------------------------------- the wide sweep
SWEEP_N = 24
SWEEP_KS = (1, 2, 3, 4, 5, 6, 7, 8, 12, 16)
SWEEP_KINDS = ("synthetic", "odd", "float", "rgb")


def lds_refused(rn, rl, ex_th=16, ex_tw=64):
    """Would the tile of the generic exact-order kernel exceed 64 KB at one disparity per chunk?  Only the sweep's redraw
    uses this restatement of k_match_exact.h: exact_lds_floats; test_config_range_cpu.py checks every drawn case (and this
    function, over all radii) against the harness, which compiles the header itself."""
    hl = rl + rn
    floats = 2 * (ex_th + 2 * hl) * (ex_tw + 2 * hl) + (ex_th + 2 * rl) * (ex_tw + 2 * rl)
    return floats * 4 > 64 * 1024


def _sweep_case(i):
    rng = np.random.default_rng(77_000 + i)
    K = int(SWEEP_KS[i % len(SWEEP_KS)]) if i < 20 else int(rng.choice(SWEEP_KS))
    Dd = int(rng.choice([rng.integers(1, 9), rng.integers(9, 60), rng.integers(60, 161)]))
    while True:                                  # redraw what smx_create refuses
        rl = int(rng.integers(0, 19))
        rn = int(rng.integers(0, 9))
        if not lds_refused(rn, rl):
            break
    # pooled images of at most 40 x 120; the four column bands of the inputs at least 0.7 of the widest box each
    h = int(rng.integers(8, 41))
    w = int(rng.integers(min(max(40, 4 * ((7 * (2 * rl + 1) + 9) // 10)), 120), 121))
    H = h * K - int(rng.integers(0, K))          # also sizes that are not multiples of K
    W = w * K - int(rng.integers(0, K))
    sad = int(rng.integers(0, 33))
    thr = int(rng.choice([0, 255] + list(range(1, 13))))
    default_agg = i % 24 in (4, 11, 16, 23)         # the default aggregation radii under other K / sad / threshold
    extra = dict(sad_patch_radius=sad, threshold=thr) if default_agg else R(rn, sad, thr, int(rng.integers(0, rl + 1)),
                                                                            int(rng.integers(0, rl + 1)), rl)
    # a third on the volume route: other radii with any min_disparity / K > 0, the default radii with min_disparity / K
    # beyond the disparity count
    dmin = 0
    if i % 3 == 1:
        dmin = Dd + int(rng.integers(1, 4)) if default_agg else int(rng.integers(1, 6))
    lo = dmin * K + int(rng.integers(0, K))      # min / max_disparity that are no multiples of K either
    hi = max((dmin + Dd) * K - 1 - int(rng.integers(0, K)), lo)
    return Case(f"sweep{i:02d}_K{K}", H, W, K, lo, hi, extra, SWEEP_KINDS[i % 4], seed=500 + i, group="sweep", volume=dmin > 0,
                columns=True)


def sweep_cases(n):
    """The first n cases of the sweep (the suite runs SWEEP_N; soak runs ask for more)."""
    return [_sweep_case(i) for i in range(n)]


SWEEP_CASES = sweep_cases(SWEEP_N)
ALL_CASES = FIXED_CASES + SWEEP_CASES
BY_ID = {c.id: c for c in ALL_CASES}


# -------------------------------------------------------------------------------------------------------------- the harness
def build_harness(out_dir, sanitize=True):
    """Compile tests/config_range_harness.cpp as host code only (no HIP runtime linked), with the address and
    undefined-behaviour sanitizers when their runtimes link that way.  Returns (path, whether the sanitizers are in)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("smx_build", os.path.join(ROOT, "stereo-depth_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    exe = os.path.join(str(out_dir), "config_range")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    log = ""
    for extra in ([san, []] if sanitize else [[]]):
        cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + extra + ["-I", b.INCLUDE, "-I", b.CSRC,
                                                                                                "-o", exe, HARNESS]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode == 0:
            return exe, bool(extra)
        log += " ".join(cmd) + "\n" + r.stdout + r.stderr + "\n"
    raise AssertionError("config-range harness did not compile:\n" + log[-6000:])


def harness_line(case_id, H, W, K, dmin, dmax, fields):
    return (f"{case_id} {H} {W} {K} {dmin} {dmax} {fields['ncc_patch_radius']} {fields['sad_patch_radius']} {fields['threshold']} "
            f"{fields['small_mbm_radius']} {fields['mid_mbm_radius']} {fields['large_mbm_radius']}")


def run_harness(exe, lines):
    """Planner facts per case id ({field: int}) and the acceptance boundaries per ncc_patch_radius
    ({rn: dict(large=, exact_lds=, neighbour=, neighbour_lds=)}), from the harness's output."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    facts, bounds = {}, {}
    for ln in r.stdout.splitlines():
        t = ln.split()
        if t[0] == "case":
            facts[t[1]] = {t[k]: int(t[k + 1]) for k in range(2, len(t), 2)}
        elif t[0] == "boundary":
            d = {t[k]: int(t[k + 1]) for k in range(1, len(t), 2)}
            bounds[d.pop("ncc")] = d
    return facts, bounds, r.stdout


def case_lines(cases):
    return [harness_line(c.id, c.H, c.W, c.K, c.dmin, c.dmax, c.fields) for c in cases]


def boundary_cases(bounds, ncc_radii=(0, 1, 4, 16)):
    """Per ncc_patch_radius: the engine with the largest large_mbm_radius the harness accepts, as a case that runs, and its
    first refused neighbour as configuration kwargs.  Read from the harness, not typed in."""
    out = []
    for rn in ncc_radii:
        b = bounds[rn]
        rl = b["large"]
        ok = Case(f"boundary_rn{rn}_rl{rl}", 64, 150, 2, 0, 19, R(rn, 5, 5, rl // 3, rl // 2, rl), "odd", seed=40 + rn)
        refused = dict(ok.config_kwargs(), large_mbm_radius=b["neighbour"])
        out.append((ok, refused))
    return out
