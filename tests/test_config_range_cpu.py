"""The configuration-range case list (tests/config_range_cases.py) kept honest without a GPU.

tests/test_config_range_gpu.py compares the HIP path with the oracle over the configuration range smx_create accepts; a
case only does its work while it still reaches the code it is aimed at and while its inputs make that code matter.  Here:

  1. the planner's facts per case, from tests/config_range_harness.cpp (host-only: it compiles smx_plan.h and runs
     derive_facts): every chunk case has exact_nd < Dd, every volume case is on the volume route, every step-6 case takes the
     generic float kernel (kt == 0 or pitch8 == 0), no case is refused, the acceptance boundary per ncc_patch_radius is
     accepted and its neighbour refused -- after a change of EX_TH, EX_TW or the planner these fail instead of the GPU
     file silently covering less;
  2. the C oracle equals its NumPy twin (oracle/stereo_numpy.py) bit for bit on the final map of every case: these
     configurations have no fixtures from the reference, the two restatements are the reference here;
  3. non-vacuity, from the oracle alone: the WTA index of every case takes at least min(4, Dd) distinct values, and in every
     case aimed at step 6 or at K step 6 moves at least 10 % of the pooled pixels off their WTA value."""
import shutil
import os

import numpy as np
import pytest

import stereo_numpy
from oracle_lib import OracleConfig
import config_range_cases as crc

CASES = crc.ALL_CASES
IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not found")
    exe, sanitized = crc.build_harness(tmp_path_factory.mktemp("config_range"))
    print("config-range harness built", "with -fsanitize=address,undefined" if sanitized else "WITHOUT the sanitizers (their runtimes did not link)")
    facts, bounds, text = crc.run_harness(exe, crc.case_lines(CASES))
    print(text)
    return exe, facts, bounds


@pytest.fixture(scope="module")
def oracle_runs(oracle_omp):
    """Oracle output and intermediates per case id, computed once."""
    cache = {}

    def get(case):
        if case.id not in cache:
            left, right = crc.inputs(case)
            cache[case.id] = (left, right) + oracle_omp.run(OracleConfig(**case.config_kwargs()), left, right, intermediates=True)
        return cache[case.id]
    return get


# ------------------------------------------------------------------------------------------------------- 1. planner facts
def test_every_case_has_facts_and_none_is_refused(planner):
    _, facts, _ = planner
    assert sorted(facts) == sorted(IDS)
    for c in CASES:
        f = facts[c.id]
        assert f["refused"] == 0 and f["exact_lds"] <= 64 * 1024, (c.id, f)
        assert f["Dd"] == c.pooled[3], (c.id, f)
        assert f["has_volume"] == int(c.volume), (c.id, f)


def test_chunk_cases_run_several_chunks(planner):
    _, facts, _ = planner
    chunked = [c for c in CASES if "chunks" in c.aims]
    assert len(chunked) >= 5
    for c in chunked:
        f = facts[c.id]
        print(f"{c.id}: Dd {f['Dd']} exact_nd {f['exact_nd']} exact_lds {f['exact_lds']} chunks {-(-f['Dd'] // f['exact_nd'])} "
              f"last {f['Dd'] - (-(-f['Dd'] // f['exact_nd']) - 1) * f['exact_nd']}")
        assert f["exact_nd"] < f["Dd"], (c.id, f)
        assert f["exact_nd"] == c.exact_nd, (c.id, f)
        # the generic kernel: other radii, or the volume route of the default radii
        assert f["default_radii"] == 0 or f["has_volume"] == 1, (c.id, f)
    f = facts["rl18_chunks3"]
    assert f["exact_lds"] == 65296 and f["Dd"] % f["exact_nd"] == 1        # the largest tile; a last chunk of one disparity
    both = [c.id for c in chunked if facts[c.id]["has_volume"]]
    assert len(both) >= 2, both                                            # WRITE_VOL with several chunks
    # the sweep reaches the loop too
    assert any(facts[c.id]["exact_nd"] < facts[c.id]["Dd"] for c in crc.SWEEP_CASES)


def test_step6_cases_take_the_generic_float_kernel(planner):
    _, facts, _ = planner
    aimed = [c for c in CASES if "step6" in c.aims]
    assert len(aimed) >= 10
    for c in aimed:
        f = facts[c.id]
        assert f["kt"] == 0 or f["pitch8"] == 0, (c.id, f)
        assert c.K != 1, c.id                       # step 6 never moves a value at K = 1
    ks = {c.K for c in CASES if "K" in c.aims}
    assert {5, 7, 16, 64} <= ks
    assert any(c.pooled[0] == 1 for c in CASES if "K" in c.aims)            # a pooled image one row high
    assert any(2 * c.fields["sad_patch_radius"] + 1 > c.W for c in aimed)   # a step-6 window wider than the image


def test_acceptance_boundary_and_its_neighbours(planner):
    exe, _, bounds = planner
    assert sorted(bounds) == list(range(17))
    assert bounds[1]["large"] == crc.BY_ID["rl18_chunks3"].fields["large_mbm_radius"] == 18
    lines, expect = [], {}
    for rn, b in bounds.items():
        assert 0 <= b["large"] < 32 and b["exact_lds"] <= 64 * 1024 < b["neighbour_lds"], (rn, b)
        # the sweep's redraw rule is the harness's rule
        assert not crc.lds_refused(rn, b["large"]) and crc.lds_refused(rn, b["neighbour"]), (rn, b)
        for Dd in (1, 40, 400):                     # acceptance does not depend on the disparity count
            for rl, refused in ((b["large"], 0), (b["neighbour"], 1)):
                key = f"rn{rn}_rl{rl}_Dd{Dd}"
                lines.append(crc.harness_line(key, 64, 600, 1, 0, Dd - 1, crc.R(rn, 5, 5, 0, 0, rl)))
                expect[key] = refused
    facts, _, _ = crc.run_harness(exe, lines)
    assert {k: f["refused"] for k, f in facts.items()} == expect
    # the cases the GPU file runs at the boundary
    pairs = crc.boundary_cases(bounds)
    assert len(pairs) >= 4
    lines = crc.case_lines([ok for ok, _ in pairs])
    for ok, refused in pairs:
        lines.append(crc.harness_line(ok.id + "_neighbour", ok.H, ok.W, ok.K, ok.dmin, ok.dmax,
                                      dict(ok.fields, large_mbm_radius=refused["large_mbm_radius"])))
    facts, _, _ = crc.run_harness(exe, lines)
    for ok, _ in pairs:
        assert facts[ok.id]["refused"] == 0 and facts[ok.id + "_neighbour"]["refused"] == 1, ok.id


def test_the_sweep_spans_the_range():
    sw = crc.SWEEP_CASES
    assert len(sw) == crc.SWEEP_N == 24
    assert {c.K for c in sw} == set(crc.SWEEP_KS)
    assert {c.kind for c in sw} == set(crc.SWEEP_KINDS)
    assert sum(c.volume for c in sw) == 8
    f = [c.fields for c in sw]
    assert max(x["large_mbm_radius"] for x in f) >= 16 and min(x["large_mbm_radius"] for x in f) == 0
    assert max(x["ncc_patch_radius"] for x in f) >= 7 and max(x["sad_patch_radius"] for x in f) >= 29
    assert {0, 255} <= {x["threshold"] for x in f}
    for c in sw:
        h, w, _, Dd = c.pooled
        assert h <= 40 and w <= 120 and 1 <= Dd <= 160, c.id
        assert c.fields["small_mbm_radius"] <= c.fields["large_mbm_radius"] >= c.fields["mid_mbm_radius"], c.id


# ------------------------------------------------------------------------------------------- 2. the oracle against its twin
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_equals_numpy_twin(oracle_runs, case):
    left, right, out_c, _ = oracle_runs(case)
    out_n, _ = stereo_numpy.run(OracleConfig(**case.config_kwargs()), left, right)
    assert np.array_equal(out_c, out_n)


# ------------------------------------------------------------------------------------------------------ 3. non-vacuity
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_is_not_vacuous(oracle_runs, case):
    _, _, _, im = oracle_runs(case)
    Dd = case.pooled[3]
    distinct = len(np.unique(im["wta_index"]))
    moved = float(np.mean(im["refined"] != im["wta"]))
    print(f"{case.id}: {distinct} distinct WTA indices of {Dd}, step 6 moves {100 * moved:.0f} % of the pooled pixels")
    assert distinct >= min(4, Dd)
    if "step6" in case.aims or "K" in case.aims:
        assert moved >= 0.10
