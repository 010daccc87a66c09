"""The filtered exact-order route (k_match_filter.h + k_match_exact2_sparse) on inputs next to its threshold and across its
instantiations, against the dense exact-order kernel and the oracle, bit for bit.

Every case builds two engines, exact_filter = 1 (always filtered) and -1 (always dense), asserts from the event profile that
the filter kernel ran in the first and not in the second, and compares the output and the WTA / step-6 cost / refined
intermediates between them, every unique pair with the oracle, and a second call with left and right swapped (the sparse
kernel has to leave the candidate bits cleared).  The unique pairs are replicated on the device up to the smallest batch the
filtered route serves (match_fast_plan(...).small false, from the device's CU count; tests/filter_cases.py), times the
row's scale where the row is about a plan that only a fuller chip brings out.

The directed pairs are the ones tests/test_filter_bound_cpu.py proves to sit between E and 2E below the approximate
maximum on most pixels: a kernel that thresholded at E, applied a bound in the wrong units, or an E a little smaller, loses
the reference's winner there.  (Mutation check done by hand: with the engine's filter_two_e halved the four directed cases
fail; everything else still passes.)  The directed K = 8 case holds 2 x 0.95 GB of float32 input on the device at 256 CUs
(70 pairs of 512 x 2304 x 3): the pooled size is the one the CPU file checks, and float32 is the only entry that can place
pooled values between the points of the 1/64 grid."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import filter_cases as fc                           # noqa: E402
from oracle_lib import OracleConfig                 # noqa: E402

STAGES = ("STAGE_WTA", "STAGE_MBM_COSTS", "STAGE_REFINED")


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


def _configs(cd, case):
    dmin, dmax = case.disparities
    kw = dict(height=case.H, width=case.W, downscale_factor=case.K, min_disparity=dmin, max_disparity=dmax)
    return cd.StereoMatchingConfiguration(**kw), OracleConfig(**kw)


def _on_device(pairs, n, u8):
    """The unique pairs, replicated on the device: pair i of the batch is unique pair i % len(pairs)."""
    idx = torch.arange(n, device="cuda") % len(pairs)
    sides = []
    for k in (0, 1):
        uniq = torch.from_numpy(np.stack([p[k] for p in pairs])).cuda()
        sides.append((uniq.to(torch.uint8) if u8 else uniq)[idx].contiguous())
    return sides


def _filtered_against_dense(cd, oracle_omp, case, pairs, cus, odd_pair=None, min_density=None):
    """The checks every case makes.  odd_pair: (index, (left, right)) replaces one pair of the batch."""
    from cuda_depth import _native as N
    n = case.pairs(cus)
    cfg, ocfg = _configs(cd, case)
    tl, tr = _on_device(pairs, n, case.u8)
    watch = sorted({0, n - 1, *range(len(pairs))})
    expect = {i: pairs[i] for i in range(len(pairs))}
    if odd_pair is not None:
        at, (ol, orr) = odd_pair
        tl[at], tr[at] = torch.from_numpy(ol).cuda(), torch.from_numpy(orr).cuda()
        expect[at] = (ol, orr)
        watch = sorted({*watch, at - 1, at, at + 1})
    filt = cd.StereoMatching(cfg, max_batch=n, exact_filter=1)
    dense = cd.StereoMatching(cfg, max_batch=n, exact_filter=-1)
    assert filt.route_info()["filter_available"] == 1
    torch.cuda.synchronize()
    filt.profile_begin(1)
    of = filt.compute_disparity_map_batch(tl, tr)
    assert filt.profile_end()["match_fast"][1] == 1, f"{case.name}: the filter kernel did not run (n = {n}, {cus} CUs)"
    dense.profile_begin(1)
    od = dense.compute_disparity_map_batch(tl, tr)
    assert dense.profile_end()["match_fast"][1] == 0, f"{case.name}: the dense engine ran the filter kernel"
    assert filt.last_match_mode() == "exact_order" and dense.last_match_mode() == "exact_order"
    torch.cuda.synchronize()
    density = filt.route_info()["candidate_density"]
    print(f"{case.name}: n = {n}, candidate density {density:.3f}")
    differing = (of != od).flatten(1).any(dim=1).nonzero().flatten().tolist()
    assert not differing, f"{case.name}: filtered and dense outputs differ in pairs {differing[:20]} of {n}"
    for i in watch:
        for st in STAGES:
            assert torch.equal(filt.intermediate(getattr(N, st), i), dense.intermediate(getattr(N, st), i)), f"{case.name}: pair {i} {st}"
    got = {i: of[i].cpu().numpy() for i in expect}
    for i, (l, r) in expect.items():
        want = oracle_omp.run(ocfg, l, r)
        bad = int((got[i] != want).sum())
        assert bad == 0, f"{case.name}: pair {i} differs from the oracle in {bad} of {want.size} pixels"
    if min_density is not None:
        assert density > min_density, f"{case.name}: candidate density {density}: the marks are not happening"
    # left and right swapped on the same engines: the candidate bits of the first call were cleared
    of2 = filt.compute_disparity_map_batch(tr, tl)
    od2 = dense.compute_disparity_map_batch(tr, tl)
    differing = (of2 != od2).flatten(1).any(dim=1).nonzero().flatten().tolist()
    assert not differing, f"{case.name}: swapped call: filtered and dense outputs differ in pairs {differing[:20]} of {n}"
    for i in (0, n - 1):
        for st in STAGES:
            assert torch.equal(filt.intermediate(getattr(N, st), i), dense.intermediate(getattr(N, st), i)), f"{case.name}: swapped, pair {i} {st}"


def _mixed(case):
    dmin, dmax = case.disparities
    pairs = fc.mixed_rgb_pairs(case.H, case.W, case.K, dmax + 1, dmin)
    return pairs


def _ids(cases):
    return [c.name for c in cases]


def test_shape_table_on_this_device(cd, cus, tmp_path):
    """The plans the library picks for the rows below on THIS device's CU count, from its own functions
    (tests/filter_bound_harness.cpp): every row is served by the filtered route.  On 256 CUs the table must reach all three
    band heights, both right-tile pitches, 1 / 2 / 3-chunk walks and 1 / 2 / 3 candidate words; on another CU count
    filter_plan may pick differently at these batch sizes -- the rows then run with what it picks, and what the table does
    not reach there is printed, not forced."""
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not found")
    _, plans = fc.run_harness(fc.build_harness(tmp_path), cus)
    print(f"{cus} CUs\n" + fc.plan_table(plans))
    missing = fc.check_plan_coverage(plans)
    assert not [m for m in missing if "small-call path" in m], missing
    if cus == 256:
        assert missing == [], missing
    elif missing:
        print("not reached on this CU count:", missing)


@pytest.mark.parametrize("case", fc.DIRECTED, ids=_ids(fc.DIRECTED))
def test_directed_pairs_next_to_the_threshold(cd, oracle_omp, cus, case):
    """The winner trails the approximate maximum by up to 1.78 E (K = 8: 1.23 E): the test that fails if the threshold or
    E is wrong.  Nearly every disparity is within 2E of the maximum, so nearly all are marked."""
    pairs = [fc.directed_rgb_pair(oracle_omp, case.K, seed) for seed in fc.DIRECTED_SEEDS]
    _filtered_against_dense(cd, oracle_omp, case, pairs, cus, min_density=0.5)


@pytest.mark.parametrize("case", fc.UNITS, ids=_ids(fc.UNITS))
def test_grid_units_1_16_64(cd, oracle_omp, cus, case):
    """K = 1, 4, 8: the PK16 = 2 / 1 / 0 instantiations of the filter kernel (grid units 1, 16, 64; the existing tests run
    unit 4), float32 RGB and at K = 8 uint8 RGB too."""
    _filtered_against_dense(cd, oracle_omp, case, _mixed(case), cus)


@pytest.mark.parametrize("case", fc.CHUNKS, ids=_ids(fc.CHUNKS))
def test_right_tile_chunks_and_pitch(cd, oracle_omp, cus, case):
    """Disparity counts either side of what one right tile holds (67 at pitch 256, 131 at pitch 320), walks of two and
    three chunks, a last chunk of a single disparity."""
    _filtered_against_dense(cd, oracle_omp, case, _mixed(case), cus)


@pytest.mark.parametrize("case", fc.WORDS, ids=_ids(fc.WORDS))
def test_candidate_word_boundaries(cd, oracle_omp, cus, case):
    """Dd = 31, 32, 33, 64, 65: bit 31, word 1 and word 2 of the candidate set (and the cyclic neighbour of disparity 0)."""
    _filtered_against_dense(cd, oracle_omp, case, _mixed(case), cus)


@pytest.mark.parametrize("case", fc.WIDTHS, ids=_ids(fc.WIDTHS))
def test_tile_columns(cd, oracle_omp, cus, case):
    """A wave's 42 columns and a workgroup's 168 ending on, before and after the 128-column edge of the exact-order tile
    the marks go to; odd image width."""
    _filtered_against_dense(cd, oracle_omp, case, _mixed(case), cus)


@pytest.mark.parametrize("case", fc.HEIGHTS, ids=_ids(fc.HEIGHTS))
def test_band_rows_across_tile_rows(cd, oracle_omp, cus, case):
    """Bands of 24 / 27 / 32 rows that start inside a 16-row tile and mark up to three tile rows, partial last band and
    tile; image height and width not multiples of K."""
    _filtered_against_dense(cd, oracle_omp, case, _mixed(case), cus)


@pytest.mark.parametrize("case", fc.DMIN, ids=_ids(fc.DMIN))
def test_min_disparity_capture_route(cd, oracle_omp, cus, case):
    """min_disparity > 0 at K = 4 and K = 1: the filtered route delivers the arg-max, the sparse capture kernel the costs
    step 6 reads."""
    _filtered_against_dense(cd, oracle_omp, case, _mixed(case), cus)


def test_range_flag_of_one_pair_at_k4(cd, oracle_omp, cus):
    """One float32 RGB pair whose gray leaves [0, 255] inside a batch of in-range pairs: that pair takes the gated dense
    kernel (the bound does not hold for it), its neighbours the filter; same bits everywhere."""
    case = fc.RANGE_FLAG
    pairs = _mixed(case)
    tex_l, tex_r = pairs[0]
    odd = (tex_l * 8.0 - 890.0, tex_r * 8.0 - 890.0)        # pooled gray from about -160 to 440 (the texture's is 91 .. 167)
    weigh = lambda x: 0.2989 * x[0] + 0.5870 * x[1] + 0.1140 * x[2]
    assert weigh(odd[0]).min() < -50.0 and weigh(odd[0]).max() > 300.0
    assert max(weigh(l).max() for l, _ in pairs) < 255.0 and min(weigh(l).min() for l, _ in pairs) >= 0.0
    _filtered_against_dense(cd, oracle_omp, case, pairs, cus, odd_pair=(5, odd))


def test_lr_entry_takes_the_filtered_route(cd, oracle_omp, cus):
    """compute_disparity_map_batch_lr on an RGB batch whose 2n internal pairs (the given ones and the mirrored ones) are
    enough for the filtered route: out and right_out equal the dense engine's, and the right-view map of every unique pair
    is the oracle's on the mirrored pair."""
    case = fc.LR
    n = case.pairs(cus) // 2
    cfg, ocfg = _configs(cd, case)
    pairs = _mixed(case)
    tl, tr = _on_device(pairs, n, False)
    filt = cd.StereoMatching(cfg, max_batch=2 * n, exact_filter=1)
    dense = cd.StereoMatching(cfg, max_batch=2 * n, exact_filter=-1)
    rf, rd = torch.full((n, case.H, case.W), 7.0, device="cuda"), torch.full((n, case.H, case.W), 9.0, device="cuda")
    torch.cuda.synchronize()
    filt.profile_begin(1)
    of = filt.compute_disparity_map_batch_lr(tl, tr, right_out=rf)
    assert filt.profile_end()["match_fast"][1] == 1, f"the filter kernel did not run on the {2 * n} internal pairs"
    dense.profile_begin(1)
    od = dense.compute_disparity_map_batch_lr(tl, tr, right_out=rd)
    assert dense.profile_end()["match_fast"][1] == 0
    assert torch.equal(of, od) and torch.equal(rf, rd)
    flip = lambda a: np.ascontiguousarray(a[..., ::-1])
    for i, (l, r) in enumerate(pairs):
        assert np.array_equal(rf[i].cpu().numpy(), flip(oracle_omp.run(ocfg, flip(r), flip(l)))), f"right view of pair {i}"
    of2 = filt.compute_disparity_map_batch_lr(tr, tl, right_out=rf)
    od2 = dense.compute_disparity_map_batch_lr(tr, tl, right_out=rd)
    assert torch.equal(of2, od2) and torch.equal(rf, rd)
