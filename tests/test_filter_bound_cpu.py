"""The error bound and the marking rule of the filtered exact-order route (k_match_filter.h) against the oracle.  No GPU.

The route evaluates a disparity in the reference's order only if its approximate cost A~ -- the aggregation of the pooled
images rounded to the 1/K^2 grid -- reaches max A~ - 2E, with E = filter_error_bound_units derived by hand in the header.
If E were too small the reference's winner would silently drop out of the evaluated set.  Here the model of
tests/filter_ref.py (A and A~ both from the oracle, E from the library through tests/filter_bound_harness.cpp) checks

  a. max |A~ - A| <= E on inputs built to spend the bound (tests/filter_cases.py), for K = 1, 2, 4, 8;
  b. on the directed pair, whose true winner trails the approximate maximum by almost 2E: the winner's deficit
     (max A~ - A~(m)) / E stays <= 2 at every pixel -- and the pair really does go beyond 1.5 (K = 8: 1.0) on most pixels,
     so that a kernel thresholding at E instead of 2E, or an E 12 % smaller, loses winners on it;
  c. both again on the full-resolution RGB form of the directed pair that tests/test_filter_route_gpu.py feeds the kernels,
     on the pooled planes the oracle actually produces from it.

Measured (CPU model values, this file's inputs; E from the library):

    max |A~ - A| / E          K = 1     K = 2     K = 4     K = 8
      uniform worst sign      0.922     0.903     0.827     0.625
      +-0.49/u, true shift    0.592     0.580     0.529     0.401
      noise                   0.073     0.065     0.054     0.036
      ends of [0, 255]        0.139     0.135     0.124     0.093
      directed pair           0.893     0.896     0.826     0.621
    directed pair, winner's deficit / E (three seeds; planes and RGB form agree to the digits shown)
      maximum                 1.776     1.787     1.650     1.235
      share of pixels > 1.5   0.88-0.92 0.88-0.92 0.79-0.81 0
      share of pixels > 1.0   0.99-1.00 0.97-1.00 0.99-1.00 1.00

Mutation check done by hand: with the assertion of (b) changed to deficit <= 1 the directed tests fail at every K."""
import os
import shutil

import numpy as np
import pytest

import filter_cases as fc
import filter_ref as fr

KS = (1, 2, 4, 8)
BOUND_SHAPE = (40, 120, 32)              # pooled rows, columns, disparities of the inputs of (a)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not found")
    return fc.build_harness(tmp_path_factory.mktemp("filter_bound"))


@pytest.fixture(scope="module")
def bound_units(harness):
    """filter_error_bound_units(u) by u, from the library."""
    return fc.run_harness(harness, 256)[0]


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_shape_table_covers_the_plan_space(harness, cus):
    """Every row of the GPU file's shape table is served by the filtered route at its batch size (and, at the smallest
    batch, not one pair earlier); across the table filter_plan picks all three band heights, both right-tile pitches and
    walks of 1, 2 and 3 chunks, and the candidate sets take 1, 2 and 3 words -- on the 256 CUs of an MI355X exactly the
    instantiation each row names."""
    _, plans = fc.run_harness(harness, cus)
    print(fc.plan_table(plans))
    assert fc.check_plan_coverage(plans) == [], fc.plan_table(plans)


def test_bound_is_the_headers_formula_scaled_by_the_unit(bound_units):
    """E grows as u^2 (rounding term: u^3 / u) plus the float32 term u^3; K = 2 is 0.32 % of the largest possible cost,
    as the header says -- a guard against the harness printing something else than the bound."""
    cost_max = 63.0 * 2295.0 * 63.0 * 2295.0 * 81.0 * 2295.0
    assert bound_units[4] / 4.0 ** 3 / cost_max == pytest.approx(0.0032, abs=0.0001)
    e_gray = [bound_units[u] / float(u) ** 3 for u in (1, 4, 16, 64)]
    assert e_gray[0] > e_gray[1] > e_gray[2] > e_gray[3] > 1e-4 * cost_max


def _model(oracle, K, left_plane, right_plane, Dd, bound_units):
    return fr.filter_model(oracle, fc.gray_from_planes(K, left_plane), fc.gray_from_planes(K, right_plane), K, Dd, bound_units[K * K])


@pytest.mark.parametrize("K", KS)
def test_approximate_cost_stays_within_the_bound(oracle_omp, bound_units, K):
    """(a): max |A~ - A| <= E on the uniform worst-sign pair, random +-0.49/u offsets around a truly shifted image, noise,
    and gray at both ends of [0, 255].  The uniform pair spends more than half of E at every K: the bound is not slack."""
    h, w, Dd = BOUND_SHAPE
    inputs = {"uniform": fc.uniform_worst_planes(K, h, w), "half_offsets": fc.half_offset_planes(K, h, w, shift=7),
              "noise": fc.noise_planes(K, h, w), "range_ends": fc.range_end_planes(K, h, w)}
    ratios = {name: _model(oracle_omp, K, l, r, Dd, bound_units).error_ratio() for name, (l, r) in inputs.items()}
    print(f"K={K} max|A~-A|/E:", {k: round(v, 4) for k, v in ratios.items()})
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert ratios["uniform"] > 0.5, ratios


def _check_directed(model, K, what):
    ratio, deficit = model.error_ratio(), model.deficit()
    over15, over10 = float((deficit > 1.5).mean()), float((deficit > 1.0).mean())
    print(f"K={K} {what}: max|A~-A|/E {ratio:.4f}  deficit/E max {deficit.max():.4f}  share > 1.5: {over15:.3f}  > 1.0: {over10:.3f}")
    assert ratio <= 1.0, (what, ratio)
    assert deficit.max() <= 2.0, (what, float(deficit.max()))                  # what the kernel relies on
    # conditions on the INPUT: the pair sits where a threshold of E, or of 1.5 E, loses the reference's winner
    if K == 8:
        assert over10 >= 0.30, (what, over10)
    else:
        assert over15 >= 0.30, (what, over15)


@pytest.mark.parametrize("K", KS)
def test_marking_rule_on_the_directed_pair(oracle_omp, bound_units, K):
    """(b): pooled planes 64 x 288, 96 disparities, through the gray entry."""
    Dd = fc.DIRECTED_SHAPE[2]
    l, r = fc.directed_planes(K, fc.DIRECTED_SEEDS[0])
    _check_directed(_model(oracle_omp, K, l, r, Dd, bound_units), K, "planes")


@pytest.mark.parametrize("seed", fc.DIRECTED_SEEDS)
@pytest.mark.parametrize("K", KS)
def test_marking_rule_on_the_rgb_form_the_gpu_gets(oracle_omp, bound_units, K, seed):
    """(c): the float32 RGB images of the GPU test (R = G = B, constant over K x K blocks, levels found by bisection on the
    oracle's steps 1 and 2), every seed it uses: the planes the oracle pools from them lie within 0.005/u of the targets
    -- 0.49/u and 0.51/u keep their side of the rounding -- and satisfy (a) and (b)."""
    u, Dd = K * K, fc.DIRECTED_SHAPE[2]
    tl, tr = fc.directed_planes(K, seed)
    L, R = fc.directed_rgb_pair(oracle_omp, K, seed)
    assert L.shape == (3, tl.shape[0] * K, tl.shape[1] * K) and L.dtype == np.float32
    assert np.array_equal(L[0], L[1]) and np.array_equal(L[0], L[2]) and np.array_equal(R[0], R[2])
    model = fr.filter_model(oracle_omp, L, R, K, Dd, bound_units[u])
    assert np.abs(model.down_left - tl).max() * u < 0.005 and np.abs(model.down_right - tr).max() * u < 0.005
    assert np.array_equal(fr.round_to_grid(model.down_left, u), np.floor(tl * u + 0.5) / u)
    assert np.array_equal(fr.round_to_grid(model.down_right, u), np.floor(tr * u + 0.5) / u)
    _check_directed(model, K, f"rgb seed {seed}")
