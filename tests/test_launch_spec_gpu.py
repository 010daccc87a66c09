"""The table from launch spec to kernel instantiation (smx_launch.h) reaches the right kernels.

plan_range() (stereo-depth_amd/csrc/smx_plan.h) names every launch of a call in a launch spec -- PrologueLaunch, ExactLaunch,
ExactCaptureLaunch, FastLaunch, FastCaptureLaunch, AutoLaunch, FilterLaunch, RefineLaunch, FillLaunch -- and the launchers
only look the instantiation up.  No device code is new here.  Every case below is one call whose plan holds one variant of a spec, run once and compared
bit for bit with the oracle, every stage (test_gpu_parity._check); which spec keys a case stands for is asked of the planner
itself: tests/launch_plan_harness.cpp, built for the device's CU count, prints them for the case's configuration, entry,
batch and decision (`spec`), and the keys its sweep's configurations reach at the two smallest pooled shapes, 48 x 80 and
64 x 128 (`reach`).  The cases together must cover all of those, and on top of them the throughput shape, which the sweep
(64 pairs at most) only reaches at its larger shapes: the smallest batch for which match_fast_plan(...).small is false, as 7
distinct pairs tiled over the batch so that the oracle runs 7 pairs.  LARGE_ONLY names what stays reachable at larger
shapes only.

The decision a case assumes (grid hint, form of the fast kernel, filter) is checked against the engine: route_info before
the call, the forced options, and the launch counts of the event profile."""
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import filter_cases as fc                           # noqa: E402
import stereo_synthetic as syn                      # noqa: E402
import test_gpu_parity as parity                    # noqa: E402
from test_launch_plan_cpu import HARNESS, _build_module     # noqa: E402

DISTINCT = 7
GRAY_F32, RGB_F32, GRAY_U8, RGB_U8 = 0, 1, 2, 3     # k_prologue.h
MODES = {"auto": 0, "exact_order": 1, "fast_grid": 2}
OTHER_RADII = dict(ncc_patch_radius=1, small_mbm_radius=2, mid_mbm_radius=3, large_mbm_radius=8)   # the harness's other radii
# Keys the sweep reaches only at its larger shapes (187 x 621, 540 x 960) and no case here does, on 256 CUs.  The one-launch
# kernel with the wide right tile (more than 193 pooled disparities) needs a grid report, which only k_refine_auto on the u8
# planes makes, and those exist only where the image is wider than K * (disparities + 2) + 8 columns (`reach` counts a grid
# hint only for such engines).  The split exact-order launch with 4 rows per thread needs a launch that fills the chip
# about once (60 tiles x 8 slices).  At the smallest batch of the throughput shape the filter kernel picks 27-row bands and
# the wide tile for both small shapes.
# The integer step-6 kernels that evaluate the SAD parabola (sx=0: K * (min_disparity / K + disparities) > 271) need the u8
# planes as well; at K = 1 that is an image wider than 280 columns with more than 271 disparities.
LARGE_ONLY = {"auto.th=8.wide=1", "auto.th=10.wide=1", "auto.th=12.wide=1", "exact.split=yes.rows=4", "filter.th=24.wide=0",
              "filter.th=24.wide=1", "filter.th=27.wide=0", "filter.th=32.wide=0", "refine.INT.kt=1.apron=0.sx=0",
              "refine.INT_V.kt=1.apron=0.sx=0", "refine.AUTO.kt=1.apron=0.sx=0", "refine.AUTO_V.kt=1.apron=0.sx=0"}

class Case:
    def __init__(self, name, h, w, Dd, entry, n=1, dmin=0, K=2, radii=True, warm=False, dense=0, dense_small=-1,
                 exact_filter=0, hint=-1, launches=None, crop=0, offset=0, lanes=False):
        # crop: W = K * w - crop; offset: the u8 inputs start that many bytes into their allocation; lanes: an engine-stream call
        self.crop, self.offset, self.lanes = crop, offset, lanes
        self.name, self.h, self.w, self.Dd, self.entry, self.n, self.dmin, self.K = name, h, w, Dd, entry, n, dmin, K
        self.radii, self.warm, self.dense, self.dense_small = radii, warm, dense, dense_small
        self.exact_filter, self.hint, self.launches = exact_filter, hint, launches

    def pairs(self, cus):
        """n, or for the throughput shape (n = 0) the smallest batch that is not `small` on this device."""
        return self.n if self.n else fc.min_pairs(self.h, self.w, cus)


S, M, T = (48, 80), (64, 128), (32, 160)
CASES = [
    # the latency shape: AUTO on f32 gray before any grid report (gated launches, the exact-order one split) ...
    Case("gated_split_th8", *S, 16, GRAY_F32, launches=(1, 1)),
    # ... and after an on-grid report: the one-launch kernel at its three band heights
    Case("auto_th8", *S, 16, GRAY_F32, warm=True, hint=0, launches=(1, 0)),
    Case("auto_th12", *M, 64, GRAY_F32, n=9, warm=True, hint=0, launches=(1, 0)),
    Case("auto_th10", *M, 64, GRAY_F32, n=17, warm=True, hint=0, launches=(1, 0)),
    # the fast kernel's latency shape and its forms
    Case("fast_th12_sparse", *M, 64, GRAY_U8, n=9, launches=(1, 0)),
    Case("fast_th12_dense_small", *M, 64, GRAY_U8, n=9, dense_small=1, launches=(1, 0)),
    Case("fast_th10_wide", *M, 194, GRAY_U8, n=17, launches=(1, 0)),
    Case("fast_pass1_capture", *S, 64, GRAY_U8, dmin=8, launches=(1, 0)),
    Case("fast_pass1_capture_wide", *S, 194, GRAY_U8, dmin=8, launches=(1, 0)),
    Case("fast_pk1", *S, 16, GRAY_U8, K=4, launches=(1, 0)),
    # the exact-order kernels
    Case("exact_unsplit", *S, 16, RGB_U8, n=5, launches=(0, 1)),
    Case("exact_split_capture", *S, 64, RGB_U8, dmin=8, launches=(0, 1)),
    Case("gated_unsplit_capture_rows4", *S, 16, GRAY_F32, dmin=8, warm=True, hint=0, launches=(1, 1)),
    Case("exact_generic", *S, 16, GRAY_F32, radii=False, launches=(0, 1)),
    Case("exact_generic_volume", *S, 16, GRAY_F32, dmin=8, radii=False, launches=(0, 1)),
    # the throughput shape (n = 0: the smallest batch that has it)
    Case("tall_24_sparse", *S, 64, GRAY_U8, n=0, launches=(1, 0)),
    Case("tall_32_sparse", *M, 194, GRAY_U8, n=0, launches=(1, 0)),
    Case("tall_32_planned_27_dense", *M, 194, GRAY_U8, n=0, dense=1, launches=(1, 0)),
    Case("tall_24_wide_dense", *S, 194, GRAY_U8, n=0, dense=1, launches=(1, 0)),
    Case("tall_32_dense_fallback_sparse", *M, 257, GRAY_U8, n=0, dense=1, launches=(1, 0)),
    Case("tall_capture", *S, 64, GRAY_U8, n=0, dmin=8, launches=(1, 0)),
    Case("tall_capture_wide", *S, 194, GRAY_U8, n=0, dmin=8, launches=(1, 0)),
    Case("filtered_u8", *S, 64, RGB_U8, n=0, exact_filter=1, launches=(1, 1)),
    Case("filtered_f32_gated_dense_capture", *M, 64, RGB_F32, n=0, dmin=8, exact_filter=1, launches=(1, 1)),
    # steps 1-2: the generic prologue for a gray entry at K = 2 (W = 159), the K = 4 block kernel for every entry and its
    # fallbacks (W = 318; u8 input that starts one byte into its allocation)
    Case("prologue_generic_odd_w_f32", *S, 16, GRAY_F32, crop=1, launches=(1, 1)),
    Case("prologue_generic_odd_w_u8", *S, 16, GRAY_U8, crop=1, launches=(1, 0)),
    Case("prologue_k4_gray_f32", *S, 16, GRAY_F32, K=4, launches=(1, 1)),
    Case("prologue_k4_rgb_u8", *S, 16, RGB_U8, K=4, launches=(0, 1)),
    Case("prologue_k4_rgb_f32", *S, 16, RGB_F32, K=4, launches=(0, 1)),
    Case("prologue_k4_fallback_w318", *S, 16, GRAY_U8, K=4, crop=2, launches=(1, 0)),
    Case("prologue_k4_fallback_unaligned_u8", *S, 16, GRAY_U8, K=4, offset=1, launches=(1, 0)),
    # steps 6 and 7-9, generic kernels: K = 3 (no power of two), K = 8 (power of two, kt = 0)
    Case("generic_k3", *S, 16, GRAY_U8, K=3, launches=(0, 1)),
    Case("generic_k8", *S, 16, GRAY_U8, K=8, launches=(1, 0)),
    # K = 1: k_fill4<1, 4>, the step-6 kernels at kt = 1 and the generic prologue for both gray entries
    Case("k1_int", *S, 16, GRAY_U8, K=1, launches=(1, 0)),
    Case("k1_int_v", *S, 16, GRAY_U8, K=1, n=5, launches=(1, 0)),
    Case("k1_auto", *S, 16, GRAY_F32, K=1, launches=(1, 1)),
    Case("k1_auto_v", *S, 16, GRAY_F32, K=1, n=5, launches=(1, 1)),
    Case("k1_float_apron", *S, 16, RGB_U8, K=1, launches=(0, 1)),
    Case("k1_float_no_planes", *S, 194, GRAY_U8, K=1, launches=(1, 0)),
    # kt = 4 beside the cases above
    Case("k4_auto_v", *S, 16, GRAY_F32, K=4, n=5, launches=(1, 1)),
    Case("k4_float_no_planes", *S, 194, GRAY_U8, K=4, launches=(1, 0)),
    # the fill with 4 pixels per thread: an engine-stream call of 5 pairs
    Case("fill_px4_k2", *S, 16, GRAY_U8, n=5, lanes=True, launches=(1, 0)),
    Case("fill_px4_k4", *S, 16, GRAY_U8, K=4, n=5, lanes=True, launches=(1, 0)),
    # sx = 0, the integer step-6 kernels that evaluate the SAD parabola: K = 2, max_disparity 271 (136 pooled disparities,
    # 2 * 136 = 272 > 271; the left apron of 284 columns fits the 320-wide image) ...
    Case("sx0_int", *T, 136, GRAY_U8, launches=(1, 0)),
    Case("sx0_int_v", *T, 136, GRAY_U8, n=5, launches=(1, 0)),
    Case("sx0_auto", *T, 136, GRAY_F32, launches=(1, 1)),
    Case("sx0_auto_v", *T, 136, GRAY_F32, n=5, launches=(1, 1)),
    # ... and K = 4 on the capture route: 4 * (8 + 64) = 288
    Case("sx0_k4_int", *S, 64, GRAY_U8, K=4, dmin=8, launches=(1, 0)),
    Case("sx0_k4_int_v", *S, 64, GRAY_U8, K=4, dmin=8, n=5, launches=(1, 0)),
    Case("sx0_k4_auto", *S, 64, GRAY_F32, K=4, dmin=8, launches=(1, 1)),
    Case("sx0_k4_auto_v", *S, 64, GRAY_F32, K=4, dmin=8, n=5, launches=(1, 1)),
]


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


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not found")
    b = _build_module()
    exe = str(tmp_path_factory.mktemp("launch_spec") / "launch_plan")
    cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + ["-I", b.INCLUDE, "-I", b.CSRC, "-o", exe, HARNESS]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "harness did not compile:\n" + r.stdout + r.stderr
    return exe


def _keys(harness, cus, case):
    """The spec keys of the case's plan on this device, from the planner itself."""
    n = case.pairs(cus)
    args = [cus, int(case.radii), case.K, case.h, case.w, case.Dd, case.dmin, max(n, 1), MODES["auto"], -1 if case.dense == 0 else 1,
            case.dense_small, case.entry, int(case.lanes), int(case.dense == 1), int(case.exact_filter >= 0), case.hint, n, 1,
            case.crop, int(case.offset % 4 == 0)]
    r = subprocess.run([harness, "spec"] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("keys"), r.stdout + r.stderr
    return set(r.stdout.split()[1:])


def test_cases_cover_what_the_sweep_reaches_at_the_two_small_shapes(cus, harness):
    r = subprocess.run([harness, "reach", str(cus)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = {ln.split()[0]: set(ln.split()[1:]) for ln in r.stdout.splitlines()}
    covered = set()
    for case in CASES:
        keys = _keys(harness, cus, case)
        print(f"{case.name:34s} n {case.pairs(cus):4d}  {' '.join(sorted(keys))}")
        covered |= keys
    missing, large_only = lines["reach-small"] - covered, lines["reach-large-only"] - covered
    print(f"{cus} CUs; reachable at larger shapes only: {sorted(large_only)}")
    if cus == 256:
        assert not missing, sorted(missing)
        assert large_only == LARGE_ONLY, sorted(large_only ^ LARGE_ONLY)
    elif missing:
        print("not covered on this CU count:", sorted(missing))


def _distinct_pairs(case, count):
    H, W, D = case.h * case.K, case.w * case.K - case.crop, (case.dmin + case.Dd) * case.K
    if case.entry in (RGB_F32, RGB_U8):
        return [syn.random_rgb_pair(H, W, D, case.K, 40 + i, dmin=case.dmin * case.K) for i in range(count)]
    return [syn.make_pair(H, W, D, case.K, 40 + i, dmin=case.dmin * case.K)[:2] for i in range(count)]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_spec_variant_against_the_oracle(cd, oracle_omp, monkeypatch, cus, case):
    from cuda_depth import _native as N
    n = case.pairs(cus)
    if case.dense:
        monkeypatch.setenv("SMX_FAST_DENSE", "1")
    if case.dense_small >= 0:
        monkeypatch.setenv("SMX_FAST_DENSE_SMALL", str(case.dense_small))
    kw = OTHER_RADII if not case.radii else {}
    cfg, ocfg = parity._cfgs(cd, case.h * case.K, case.w * case.K - case.crop, case.K, case.dmin * case.K, (case.dmin + case.Dd) * case.K - 1, **kw)
    pairs = _distinct_pairs(case, min(n, DISTINCT))
    u8 = case.entry in (GRAY_U8, RGB_U8)
    idx = torch.arange(n, device="cuda") % len(pairs)
    tl, tr = (torch.from_numpy(np.stack([p[k] for p in pairs])).cuda() for k in (0, 1))
    tl, tr = ((t.to(torch.uint8) if u8 else t)[idx].contiguous() for t in (tl, tr))
    if case.offset:                                     # the same bytes, `offset` bytes into a flat allocation
        flat = [torch.empty(t.numel() + case.offset, dtype=torch.uint8, device="cuda") for t in (tl, tr)]
        tl, tr = (b[case.offset:].view(t.shape).copy_(t) for b, t in zip(flat, (tl, tr)))
        assert tl.data_ptr() % 4 == case.offset % 4 and tr.data_ptr() % 4 == case.offset % 4
    sm = cd.StereoMatching(cfg, max_batch=n, exact_filter=case.exact_filter)
    if case.warm:                                       # an on-grid f32 gray call first: its report is the grid hint 0
        sm.compute_disparity_map_batch(tl[:1], tr[:1])
        torch.cuda.synchronize()
    info = sm.route_info()
    assert info["offgrid_hint"] == case.hint and (case.dense == 1 or info["fast_dense"] == 0), info
    sm.profile_begin(1)
    out = sm.compute_disparity_map_batch(tl, tr, engine_streams=case.lanes)
    if case.lanes:
        sm.join()
    prof = sm.profile_end()
    torch.cuda.synchronize()
    assert (prof["match_fast"][1], prof["match_exact"][1]) == case.launches, prof
    if case.exact_filter == 1:
        assert sm.route_info()["last_call_filtered"] == 1
    rgb = case.entry in (RGB_F32, RGB_U8)
    stages = {"down_left": N.STAGE_DOWN_LEFT, "down_right": N.STAGE_DOWN_RIGHT, "wta": N.STAGE_WTA, "refined": N.STAGE_REFINED,
              "costs": N.STAGE_MBM_COSTS}
    if rgb:
        stages.update(gray_left=N.STAGE_GRAY_LEFT, gray_right=N.STAGE_GRAY_RIGHT)
    if int(N.LIB.smx_stage_bytes(sm._handle, N.STAGE_AGG_VOLUME)):
        stages["agg_volume"] = N.STAGE_AGG_VOLUME
    want = []
    for i, (l, r) in enumerate(pairs):
        ref_out, ref = oracle_omp.run(ocfg, l, r, intermediates=True, volumes=True)
        im = {k: sm.intermediate(st, i).cpu().numpy() for k, st in stages.items()}
        im["out"] = out[i].cpu().numpy()
        parity._check(im, ref_out, ref, case.dmin)
        want.append(ref_out)
    # ... and every pair of the batch is its distinct pair's map
    expect = torch.from_numpy(np.stack(want)).cuda()[idx]
    differing = (out != expect).flatten(1).any(dim=1).nonzero().flatten().tolist()
    assert not differing, f"pairs {differing[:20]} of {n} differ from the oracle's map of their distinct pair"
