"""The HIP path against the oracle across the configuration range smx_create accepts (tests/config_range_cases.py).

The other parity files stay where ncc <= 3, sad <= 8, large_mbm_radius <= 12, K in {1, 2, 3, 4, 8} and the generic
exact-order kernel stages its right tile once.  Here: several right-tile chunks of k_match_exact (also with the aggregated
volume written), the largest tile smx_create accepts and the first one it refuses, K = 5, 7, 16, 64 through the generic
prologue, the generic float step 6 up to a 65-wide window on a 60-wide image, k_fill<false> / k_fill<true>, thresholds 0 and
10^6, one disparity, radii 0, and a seeded sweep of 24 configurations over all of it.  Every stage is compared bit for bit
(test_gpu_parity._check); a configuration the engine refuses fails its test unless the list declares it refused.
tests/test_config_range_cpu.py checks, without a GPU, that each case still reaches the code it is aimed at."""
import ctypes as C
import shutil
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle_lib import OracleConfig                         # noqa: E402
import config_range_cases as crc                           # noqa: E402
from test_gpu_parity import _run_hip, _check               # noqa: E402
from test_lr_check_gpu import oracle_lr, assert_bitwise    # noqa: E402


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


@pytest.fixture(scope="module")
def refs(oracle_omp):
    """(left, right, oracle output, oracle intermediates) per case id, computed once and shared."""
    cache = {}

    def get(case):
        if case.id not in cache:
            left, right = crc.inputs(case)
            cache[case.id] = (left, right) + oracle_omp.run(OracleConfig(**case.config_kwargs()), left, right,
                                                            intermediates=True, volumes=True)
        return cache[case.id]
    return get


def _compare(cd, case, left, right, ref_out, ref, mode="auto"):
    cfg = cd.StereoMatchingConfiguration(**case.config_kwargs())
    im = _run_hip(cd, cfg, left, right, mode)          # a RuntimeError (a refused configuration) fails the test
    _check(im, ref_out, ref, case.pooled[2])
    assert ("agg_volume" in im) == case.volume
    return im


# ------------------------------------------------------------------------------------------------ fixed cases and the sweep
@pytest.mark.parametrize("mode", ["auto", "exact_order"])
@pytest.mark.parametrize("case", crc.FIXED_CASES, ids=[c.id for c in crc.FIXED_CASES])
def test_fixed_case(cd, refs, case, mode):
    left, right, ref_out, ref = refs(case)
    _compare(cd, case, left, right, ref_out, ref, mode)


# SMX_CONFIG_RANGE_SEEDS=N widens the sweep (soak runs; the suite runs the 24 cases the CPU file checks)
SWEEP = crc.sweep_cases(max(int(os.environ.get("SMX_CONFIG_RANGE_SEEDS", "0")), crc.SWEEP_N))


@pytest.mark.parametrize("case", SWEEP, ids=[c.id for c in SWEEP])
def test_sweep_case(cd, refs, case):
    left, right, ref_out, ref = refs(case)
    _compare(cd, case, left, right, ref_out, ref)


# ------------------------------------------------------------------------------------------------------------- the entries
@pytest.mark.parametrize("case_id", crc.ENTRY_CASE_IDS)
def test_u8_entries_equal_f32_entries_and_the_oracle(cd, oracle_omp, case_id):
    """Every entry has a prologue of its own (f32 / u8, gray / RGB): integer-valued inputs in 0..255 through all four, every
    stage against the oracle, the u8 maps equal to the f32 maps."""
    case = crc.BY_ID[case_id]
    ocfg = OracleConfig(**case.config_kwargs())
    for rgb in (False, True):
        left, right = crc.integer_inputs(case, rgb)
        assert np.array_equal(left, left.astype(np.uint8)) and np.array_equal(right, right.astype(np.uint8))
        ref_out, ref = oracle_omp.run(ocfg, left, right, intermediates=True, volumes=True)
        f32 = _compare(cd, case, left, right, ref_out, ref)
        u8 = _compare(cd, case, left.astype(np.uint8), right.astype(np.uint8), ref_out, ref)
        for k in ("out", "wta", "refined", "down_left", "down_right"):
            assert np.array_equal(f32[k], u8[k]), (k, "rgb" if rgb else "gray")


# ------------------------------------------------------------------------------------------------------------------ batches
BATCH_N = 5
_batch_refs = {}


def _batch_ref(oracle, case):
    if case.id not in _batch_refs:
        L, R = crc.batch_inputs(case, BATCH_N)
        ocfg = OracleConfig(**case.config_kwargs())
        _batch_refs[case.id] = (L, R, [oracle.run(ocfg, L[i], R[i]) for i in range(BATCH_N)])
    return _batch_refs[case.id]


@pytest.mark.parametrize("lanes", [False, True], ids=["caller_stream", "engine_streams"])
@pytest.mark.parametrize("case_id", crc.BATCH_CASE_IDS)
def test_batches(cd, oracle_omp, case_id, lanes):
    """Five distinct pairs in one call (pair b's tiles, volume slice and planes at their own offsets), on the caller's stream
    and on the engine's stream lanes followed by join()."""
    case = crc.BY_ID[case_id]
    L, R, want = _batch_ref(oracle_omp, case)
    assert not any(np.array_equal(want[0], w) for w in want[1:])
    sm = cd.StereoMatching(cd.StereoMatchingConfiguration(**case.config_kwargs()), max_batch=BATCH_N)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    torch.cuda.synchronize()
    if lanes:
        out = sm.compute_disparity_map_batch(tl, tr, engine_streams=True)
        sm.join()
    else:
        out = sm.compute_disparity_map_batch(tl, tr)
    out = out.cpu().numpy()
    for i in range(BATCH_N):
        assert np.array_equal(out[i], want[i]), f"pair {i}"


def test_lr_batch_under_K3_and_large_radius_12(cd, oracle_omp):
    """The left-right checked batch entry under a configuration off its usual corner: K = 3 (generic prologue, step 6 and fill)
    and large_mbm_radius 12 (the generic exact-order kernel), compared as tests/test_lr_check_gpu.py compares."""
    case = crc.Case("lr_K3_rl12", 60, 150, 3, 0, 44, crc.R(1, 5, 5, 2, 6, 12), "odd", seed=9)
    n = 2
    L, R = crc.batch_inputs(case, n)
    ocfg = OracleConfig(**case.config_kwargs())
    sm = cd.StereoMatching(cd.StereoMatchingConfiguration(**case.config_kwargs()), max_batch=2 * n)
    right_out = torch.full((n, case.H, case.W), 7.0, device="cuda")
    out = sm.compute_disparity_map_batch_lr(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), right_out=right_out,
                                            max_diff=1.0, invalid_disparity=-1.0)
    out, right_out = out.cpu().numpy(), right_out.cpu().numpy()
    for i in range(n):
        exp, dr = oracle_lr(oracle_omp, ocfg, L[i], R[i])
        assert_bitwise(right_out[i], dr, f"right_out pair {i}")
        assert_bitwise(out[i], exp, f"out pair {i}")
        assert 0.05 < float(np.mean(exp == -1.0)) < 0.95          # both outcomes of the check occur


# ----------------------------------------------------------------------------------------------------------- the boundary
@pytest.fixture(scope="module")
def boundary(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not found")
    exe, _ = crc.build_harness(tmp_path_factory.mktemp("config_range"), sanitize=False)
    _, bounds, _ = crc.run_harness(exe, [])
    return {ok.fields["ncc_patch_radius"]: (ok, refused) for ok, refused in crc.boundary_cases(bounds)}


@pytest.mark.parametrize("rn", [0, 1, 4, 16])
def test_largest_accepted_radius_runs_and_its_neighbour_is_refused(cd, oracle_omp, boundary, rn):
    """Per ncc_patch_radius the largest large_mbm_radius whose tile fits the 64 KB (read from the planner's own header through
    tests/config_range_harness.cpp): that engine runs and matches the oracle; one more is SMX_ERR_UNSUPPORTED with the
    message that names the radii."""
    from cuda_depth import _native as N
    ok, refused = boundary[rn]
    left, right = crc.inputs(ok)
    ref_out, ref = oracle_omp.run(OracleConfig(**ok.config_kwargs()), left, right, intermediates=True, volumes=True)
    _compare(cd, ok, left, right, ref_out, ref)
    cfg = cd.StereoMatchingConfiguration(**refused)
    rl = refused["large_mbm_radius"]
    with pytest.raises(RuntimeError, match=rf"radii too large for the LDS tile: ncc_patch_radius {rn} \+ large_mbm_radius {rl} need "
                                           rf"\d+ bytes of the 65536 available.*\(status -5\)"):
        cd.StereoMatching(cfg)
    c = cfg._as_struct(0, 1, 0)
    h = C.c_void_p()
    assert N.LIB.smx_create(C.byref(c), C.byref(h)) == -5 and not h.value
