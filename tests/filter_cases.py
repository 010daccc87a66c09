"""Inputs and shapes of the tests of the filtered exact-order route (k_match_filter.h + k_match_exact2_sparse):
tests/test_filter_bound_cpu.py (the error bound and the marking rule against the oracle) and tests/test_filter_route_gpu.py
(the kernels on those inputs and across their instantiations).

The first half builds inputs that sit next to the filter's threshold.  The filter rounds the pooled images to the 1/u grid
(u = K^2) and evaluates a disparity exactly only if its approximate cost reaches max - 2E; an input whose pooled values lie
0.49/u from a grid point, with the signs arranged so that every tap moves the same way, spends almost all of E.  The
second half is the shape table of the GPU file: every row is the smallest shape at which one thing can still go wrong.
tests/filter_bound_harness.cpp prints what the library's own plan functions choose for every row, and both test files
assert that the table covers the plan space."""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import subprocess
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "filter_bound_harness.cpp")

# ---- the launch rule of the filtered route (k_match_fast.h: match_fast_plan) ---------------------------------------------
# A call takes the filter only when its aggregation launch has the throughput shape: 8 * workgroups >= 13 * CUs, a
# workgroup covering 168 columns x 24 rows of one pooled pair.  tests/filter_bound_harness.cpp checks min_pairs against the
# function itself (small at n - 1, not small at n).
WG_COLS, WG_ROWS = 168, 24


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def min_pairs(h: int, w: int, cus: int) -> int:
    """The smallest n for which match_fast_plan(h, w, n, cus).small is false."""
    wgs = cdiv(w, WG_COLS) * cdiv(h, WG_ROWS)
    return cdiv(13 * cus, 8 * wgs)


# ---- inputs next to the threshold ---------------------------------------------------------------------------------------
DIRECTED_SHAPE = (64, 288, 96)                     # pooled rows, columns (6 blocks of 48: the cyclic wrap keeps the pattern), disparities
DIRECTED_G = 100.0
DIRECTED_SEEDS = (0, 1, 2)                         # the unique pairs of the GPU case


def directed_planes(K: int, seed: int = 0, g: float = DIRECTED_G, h: int = DIRECTED_SHAPE[0], w: int = DIRECTED_SHAPE[1],
                    block: int = 48) -> Tuple[np.ndarray, np.ndarray]:
    """Pooled planes (float64 targets) whose true winner trails the filter's approximate maximum by almost 2E.

    Left: uniform, 0.51/u above a grid point (rounds up by 0.49/u).  Right: 48-column blocks alternating between
    g - 5/u + 0.49/u and g + 5/u + 0.49/u (both round down by 0.49/u), a random 10 % of the pixels of the second kind
    raised by a further 1/u.  Real |l - r| is 5.02/u in the first kind of block and 4.98/u (5.98/u where raised: 5.08/u on
    average) in the second, so the reference's winner looks at blocks of the first kind; rounded, the first kind costs 6/u
    and the second 4/u (4.1/u on average): the filter's maximum looks at the second kind, ~1.9/u per tap above the true
    winner's approximate cost, where E allows 1.05/u per tap."""
    u = float(K * K)
    rng = np.random.default_rng(9100 + seed)
    left = np.full((h, w), g + 0.51 / u)
    second = (np.arange(w) // block) % 2 == 1
    right = np.broadcast_to(np.where(second, g + 5.0 / u + 0.49 / u, g - 5.0 / u + 0.49 / u), (h, w)).copy()
    raised = (rng.random((h, w)) < 0.10) & second[None, :]
    right[raised] += 1.0 / u
    return left, right


def uniform_worst_planes(K: int, h: int, w: int, g: float = 128.0):
    """l = g + 0.49/u, r = g - 0.49/u everywhere: every tap of every disparity loses 0.98/u to the rounding."""
    u = float(K * K)
    return np.full((h, w), g + 0.49 / u), np.full((h, w), g - 0.49 / u)


def half_offset_planes(K: int, h: int, w: int, shift: int, seed: int = 0):
    """Random integers with random +-0.49/u offsets; the right plane is the left one's integers moved by `shift` columns."""
    u = float(K * K)
    rng = np.random.default_rng(9200 + seed)
    base = rng.integers(1, 255, (h, w)).astype(np.float64)
    sl = np.where(rng.random((h, w)) < 0.5, -0.49, 0.49) / u
    sr = np.where(rng.random((h, w)) < 0.5, -0.49, 0.49) / u
    return base + sl, np.roll(base, -shift, axis=1) + sr


def noise_planes(K: int, h: int, w: int, seed: int = 0):
    """Independent uniform noise over the whole range, anywhere between the grid points."""
    rng = np.random.default_rng(9300 + seed)
    return rng.uniform(0.0, 255.0, (h, w)), rng.uniform(0.0, 255.0, (h, w))


def range_end_planes(K: int, h: int, w: int, seed: int = 0):
    """Every pixel at one end of [0, 255], 0.49/u inside it: taps of 255 and of ~0, the largest and smallest box sums."""
    u = float(K * K)
    rng = np.random.default_rng(9400 + seed)
    ends = np.array([0.49 / u, 255.0 - 0.49 / u])
    return ends[rng.integers(0, 2, (h, w))], ends[rng.integers(0, 2, (h, w))]


def gray_from_planes(K: int, plane: np.ndarray) -> np.ndarray:
    """Full-resolution float32 gray image, constant over each K x K block, whose mean pool is (within a rounding) `plane`."""
    return np.kron(plane.astype(np.float32), np.ones((K, K), np.float32))


def _pooled_of(oracle, K: int, v: np.ndarray) -> np.ndarray:
    """The oracle's own step 1 + step 2 on K x K blocks of R = G = B = v[t]: the pooled gray of every block."""
    t = v.size
    H, W = K, K * t
    plane = np.kron(v.astype(np.float32)[None, :], np.ones((K, K), np.float32))
    rgb = np.ascontiguousarray(np.broadcast_to(plane[None], (3, H, W)), dtype=np.float32)
    gray = np.empty((H, W), np.float32)
    out = np.empty((1, t), np.float32)
    fp = C.POINTER(C.c_float)
    oracle.lib.so_rgb_to_gray(rgb.ctypes.data_as(fp), C.c_int(H), C.c_int(W), gray.ctypes.data_as(fp))
    oracle.lib.so_mean_pool(gray.ctypes.data_as(fp), C.c_int(H), C.c_int(W), C.c_int(K), out.ctypes.data_as(fp))
    return out[0]


def rgb_levels_for(oracle, K: int, targets: np.ndarray) -> np.ndarray:
    """For every target pooled value the float32 v whose K x K block of R = G = B = v pools (oracle steps 1 and 2) closest
    to it.  Bisection over the bit patterns of positive float32 (ordered like the values; both steps are monotone in v)."""
    targets = np.asarray(targets, np.float64)
    lo = np.zeros(targets.shape, np.int64)                                   # pools to 0 <= target
    hi = np.full(targets.shape, int(np.float32(512.0).view(np.int32)), np.int64)
    as_f32 = lambda bits: bits.astype(np.int32).view(np.float32)
    assert (_pooled_of(oracle, K, as_f32(hi)) > targets).all() and (targets > 0).all()
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        below = _pooled_of(oracle, K, as_f32(mid)).astype(np.float64) <= targets
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    plo, phi = (_pooled_of(oracle, K, as_f32(b)).astype(np.float64) for b in (lo, hi))
    return as_f32(np.where(np.abs(plo - targets) <= np.abs(phi - targets), lo, hi))


def rgb_from_planes(oracle, K: int, plane: np.ndarray) -> np.ndarray:
    """[3, h K, w K] float32 with R = G = B, constant over each K x K block, whose pooled gray (as the oracle and the
    prologue kernel compute it) is the float32 closest to `plane` that such a block can reach."""
    values, inverse = np.unique(plane, return_inverse=True)
    v = rgb_levels_for(oracle, K, values)[inverse.reshape(plane.shape)]
    full = np.kron(v, np.ones((K, K), np.float32))
    return np.ascontiguousarray(np.broadcast_to(full[None], (3,) + full.shape), dtype=np.float32)


def directed_rgb_pair(oracle, K: int, seed: int = 0):
    l, r = directed_planes(K, seed)
    return rgb_from_planes(oracle, K, l), rgb_from_planes(oracle, K, r)


# ---- ordinary content for the sweeps of the GPU file ----------------------------------------------------------------------
def mixed_rgb_pairs(H: int, W: int, K: int, D: int, dmin: int = 0, seed: int = 0):
    """Four integer-valued RGB pairs (float32 [3, H, W]): textured bands (few candidates), independent noise and a flat
    pair (every disparity a candidate), and a periodic texture of period 8 pooled columns with a little noise (near ties
    and exact ties in the exact cost: the first maximum has to win)."""
    import stereo_synthetic as syn
    rng = np.random.default_rng(9500 + seed)
    pairs = [syn.random_rgb_pair(H, W, D, K, 90 + seed, dmin=dmin)]
    pairs.append((rng.integers(0, 256, (3, H, W)).astype(np.float32), rng.integers(0, 256, (3, H, W)).astype(np.float32)))
    pairs.append((np.full((3, H, W), 37.0, np.float32), np.full((3, H, W), 37.0, np.float32)))
    tile = rng.integers(0, 256, (3, H, 8 * K)).astype(np.float32)
    per_l = np.tile(tile, (1, 1, W // (8 * K) + 1))[:, :, :W]
    per_r = np.roll(per_l, -(dmin + 5 * K), axis=2).copy()
    spots = rng.random((3, H, W)) < 0.002
    per_r[spots] = np.clip(per_r[spots] + rng.integers(-3, 4, int(spots.sum())), 0, 255)
    pairs.append((per_l, per_r))
    return [(np.ascontiguousarray(l, dtype=np.float32), np.ascontiguousarray(r, dtype=np.float32)) for l, r in pairs]


# ---- the shape table of tests/test_filter_route_gpu.py --------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    K: int
    h: int                  # pooled rows
    w: int                  # pooled columns
    Dd: int                 # pooled disparities
    dmin: int = 0           # pooled minimum disparity (> 0: the capture route)
    cut: Tuple[int, int] = (0, 0)     # rows and columns the image is short of h K x w K (H, W not multiples of K)
    u8: bool = False
    pairs_factor: int = 1   # an LR call of n pairs is one internal call of 2 n
    scale: int = 1          # pairs of the call, in multiples of the smallest batch the filtered route serves
    at256: Optional[Tuple[int, int, int]] = None      # filter_plan's (th, wide, chunks) on 256 CUs, where the case is about them

    @property
    def H(self) -> int:
        return self.h * self.K - self.cut[0]

    @property
    def W(self) -> int:
        return self.w * self.K - self.cut[1]

    @property
    def disparities(self) -> Tuple[int, int]:
        """(min_disparity, max_disparity) of the configuration."""
        return self.dmin * self.K, (self.dmin + self.Dd) * self.K - 1

    def pairs(self, cus: int) -> int:
        """Pairs of the engine's internal call: `scale` times the smallest count the filtered route serves."""
        n = min_pairs(self.h, self.w, cus) * self.scale
        return cdiv(n, self.pairs_factor) * self.pairs_factor


_DH, _DW, _DD = DIRECTED_SHAPE
DIRECTED = [Case(f"directed_k{K}", K, _DH, _DW, _DD) for K in (1, 2, 4, 8)]
# unit-1 / 16 / 64 instantiations (PK16 = 2, 1, 0) on ordinary content
# (K = 8 as float32: 49 x 169 keeps three band rows and two tile columns in half the bytes)
UNITS = [Case("unit_k1", 1, 50, 300, 40), Case("unit_k4", 4, 50, 300, 40), Case("unit_k8", 8, 49, 169, 40),
         Case("unit_k8_u8", 8, 50, 300, 40, u8=True)]
# filter_plan picks the band height (24 / 27 / 32 rows) and the right-tile pitch (256: 67 disparities per chunk, 320: 131) by
# a cost model of whole rounds of workgroups, so its choice moves with the batch size: at the smallest batch the filtered route
# serves (less than one round) it is 27 rows and the wide tile whatever the shape; a few rounds (scale 2 or 3) bring out the
# choice by image height and range.  at256 is what the library picks on the 256 CUs of an MI355X (asserted against the
# harness by the CPU file); on another CU count the same rows run with whatever the plan picks there.
# either side of the 67 / 131 disparities of one right tile, at both pitches: one chunk that is exactly full, a second
# chunk of one disparity, two- and three-chunk walks
CHUNKS = [Case(f"chunk_d{Dd}_h{h}_x{scale}", 2, h, Dd + 40, Dd, scale=scale, at256=at256) for Dd, h, scale, at256 in (
    (66, 40, 3, (24, 0, 1)), (67, 40, 3, (24, 0, 1)), (68, 40, 3, (24, 1, 1)), (68, 49, 2, (27, 0, 2)),
    (130, 40, 3, (24, 1, 1)), (131, 40, 3, (24, 1, 1)), (131, 49, 2, (27, 0, 2)), (132, 40, 1, (27, 1, 2)),
    (132, 40, 3, (24, 0, 2)), (140, 49, 2, (27, 0, 3)), (140, 40, 3, (24, 1, 2)), (200, 49, 2, (27, 0, 3)),
    (200, 40, 3, (24, 1, 2)))]
# bit 31 / word 1 / word 2 of the candidate set
WORDS = [Case(f"words_d{Dd}", 2, 40, 200, Dd) for Dd in (31, 32, 33, 64, 65)]
# a wave's 42 columns and a workgroup's 168 ending on, before and after the 128-column tile edge; W odd
WIDTHS = [Case(f"width_{w}", 2, 40, w, 24, cut=(0, 1), scale=3, at256=(24, 0, 1)) for w in (127, 128, 129, 168, 169, 170, 211)]
# bands of 24 / 27 / 32 rows across 16-row tiles, partial last band and tile; H and W not multiples of K
HEIGHTS = [Case(f"height_{h}_x{scale}", 4 if h % 2 else 2, h, 200, 24, cut=(3, 2) if h % 2 else (1, 1), scale=scale, at256=at256)
           for h, scale, at256 in ((15, 3, (24, 0, 1)), (16, 3, (24, 0, 1)), (17, 3, (24, 0, 1)), (31, 3, (32, 0, 1)),
                                   (31, 2, (32, 1, 1)), (33, 3, (24, 0, 1)), (49, 2, (27, 0, 1)), (55, 2, (32, 0, 1)))]
# min_disparity > 0: the sparse capture kernel delivers the costs of step 6
DMIN = [Case("dmin_k4", 4, 50, 300, 40, dmin=8), Case("dmin_k1", 1, 50, 300, 40, dmin=8)]
RANGE_FLAG = Case("range_flag_k4", 4, 50, 300, 40)
LR = Case("lr_k2", 2, 50, 300, 40, pairs_factor=2)

ALL_CASES: List[Case] = DIRECTED + UNITS + CHUNKS + WORDS + WIDTHS + HEIGHTS + DMIN + [RANGE_FLAG, LR]


def harness_input(cus: int, cases: Optional[List[Case]] = None) -> str:
    """Lines "name h w Dd n" for tests/filter_bound_harness.cpp."""
    return "".join(f"{c.name} {c.h} {c.w} {c.Dd} {c.pairs(cus)}\n" for c in (cases or ALL_CASES))


class Plan(NamedTuple):
    cus: int
    name: str
    h: int
    w: int
    Dd: int
    n: int
    small_below: int
    small: int
    th: int
    wide: int
    chunks: int
    words: int


def parse_harness(text: str):
    """(E in aggregation units by u, plans) from the harness's output."""
    bounds, plans = {}, []
    for line in text.splitlines():
        f = line.split()
        if f and f[0] == "E":
            bounds[int(f[1])] = float(f[2])
        elif f and f[0] == "plan":
            plans.append(Plan(int(f[1]), f[2], *map(int, f[3:])))
    return bounds, plans


def check_plan_coverage(plans: List[Plan]) -> List[str]:
    """What the table must reach on one device; returns the list of things it does not (empty: covered)."""
    missing = []
    by = {p.name: p for p in plans}
    for c in ALL_CASES:
        p = by.get(c.name)
        if p is not None and p.cus == 256 and c.at256 is not None and (p.th, p.wide, p.chunks) != c.at256:
            missing.append(f"{c.name}: the plan on 256 CUs is {(p.th, p.wide, p.chunks)}, the table says {c.at256}")
    for p in plans:
        if p.small:
            missing.append(f"{p.name}: n = {p.n} still takes the small-call path")
        if not p.small_below and p.n == min_pairs(p.h, p.w, p.cus):
            missing.append(f"{p.name}: n = {p.n} is not the smallest batch the filtered route serves")
    if {p.th for p in plans} != {24, 27, 32}:
        missing.append(f"band heights {sorted({p.th for p in plans})}")
    chunk_plans = [by[c.name] for c in CHUNKS if c.name in by]
    if {p.wide for p in chunk_plans} != {0, 1}:
        missing.append(f"right-tile pitches of the chunk cases: wide in {sorted({p.wide for p in chunk_plans})}")
    counts = {min(p.chunks, 3) for p in chunk_plans}
    if counts != {1, 2, 3}:
        missing.append(f"chunk counts {sorted(counts)}")
    if {by[c.name].words for c in WORDS if c.name in by} != {1, 2, 3}:
        missing.append("candidate words 1, 2, 3")
    return missing


# ---- tests/filter_bound_harness.cpp ------------------------------------------------------------------------------------
def build_harness(directory) -> str:
    """Compiles the harness with build.py's flags and include directories; host code only, no HIP runtime linked."""
    spec = importlib.util.spec_from_file_location("smx_build", os.path.join(ROOT, "stereo-depth_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    exe = os.path.join(str(directory), "filter_bound")
    cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + ["-I", b.INCLUDE, "-I", b.CSRC, "-o", exe, HARNESS]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "harness did not compile:\n" + r.stdout + r.stderr
    return exe


def run_harness(exe: str, cus: int):
    r = subprocess.run([exe, str(cus)], input=harness_input(cus), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    bounds, plans = parse_harness(r.stdout)
    assert sorted(bounds) == [1, 4, 16, 64] and len(plans) == len(ALL_CASES), r.stdout[-2000:]
    return bounds, plans


def plan_table(plans) -> str:
    head = f"{'case':22s} {'h':>3s} {'w':>3s} {'Dd':>3s} {'n':>4s} small th wide chunks words"
    return "\n".join([head] + [f"{p.name:22s} {p.h:3d} {p.w:3d} {p.Dd:3d} {p.n:4d} {p.small:5d} {p.th:2d} {p.wide:4d} {p.chunks:6d} {p.words:5d}"
                               for p in plans])
