"""The second pass of the stacked bands (k_match_fast.h: fast_stacked_tail) on paper: tests/stacked_tail_ref.py.

1. The rule.  tests/stacked_tail_harness.cpp prints the header's own fast_tail_leftover / fast_tail_rows /
   fast_tail_rows_halves (host side of the __host__ __device__ functions the kernel runs); every line equals the model's
   restatement, and the joint tail never marches more tile rows than the per-band tail: for every count triple up to 8, for
   1,000 random needed sets dealt march by march, and for every window of every input below.  A dealt set is also complete:
   every (disparity, row) that a unit band needs lies in the row mask of a march of that disparity over that unit band.
   The second table costs no LDS: it takes the place of the second exchange row (fast_xch_rows).
2. The inputs of tests/test_stacked_tail_gpu.py.  From the oracle's winner map alone, every case (its eight contents tiled
   over one batch) holds a window with a disparity needed by both unit bands, one needed by the upper and one by the lower
   band only, an odd count in each of the three queues (the leftover rule runs), a full march whose row mask has bits at or
   above 32, and the winners 0 and Dd - 1 (whose neighbours wrap) -- except what a shape's geometry excludes
   (stacked_tail_ref.CASES, `lacks`), which is asserted absent.  Over all cases every leftover code occurs.  A bit-for-bit
   pass of the GPU test therefore covers every march form and every branch of the rule.
No GPU."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import stacked_tail_ref as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "stacked_tail_harness.cpp")


def _build_module():
    spec = importlib.util.spec_from_file_location("smx_build", os.path.join(ROOT, "stereo-depth_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def harness_lines(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not found")
    b = _build_module()
    exe = str(tmp_path_factory.mktemp("stacked_tail") / "stacked_tail")
    cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + ["-I", b.INCLUDE, "-I", b.CSRC, "-o", exe, HARNESS]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "harness did not compile:\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def test_the_model_restates_the_header_rule(harness_lines):
    left = [[int(v) for v in ln[1:]] for ln in harness_lines if ln[0] == "left"]
    rows = [[int(v) for v in ln[1:]] for ln in harness_lines if ln[0] == "rows"]
    assert len(left) == 8 and len(rows) == 9 ** 3
    for b, u, l, code, r in left:
        assert code == st.leftover_code(b, u, l) and r == st.leftover_rows(code), (b, u, l, code, r)
    assert sorted(c for _, _, _, c, _ in left) == list(range(8)), "eight cases, eight codes"
    for nb, nu, nl, joint, halves in rows:
        assert joint == st.rows_joint(nb, nu, nl) and halves == st.rows_halves(nb, nu, nl), (nb, nu, nl, joint, halves)
        assert joint <= halves, (nb, nu, nl, joint, halves)
        assert halves - joint >= 22 * (nb // 2), "every pair needed by both unit bands saves 2 * 46 - 70 rows"


def test_the_second_table_takes_the_place_of_an_exchange_row(harness_lines):
    """The workgroup's LDS is what it was: a stacked kernel keeps one exchange row of 76 64-bit entries per wave instead of
    two, and the second table of at most 68 words fits the 608 bytes that frees."""
    lds = {int(ln[1]): (int(ln[2]), int(ln[3])) for ln in harness_lines if ln[0] == "lds"}
    xch = {int(ln[1]): int(ln[2]) for ln in harness_lines if ln[0] == "xch"}
    assert xch == {48: 1, 32: 2, 27: 2, 24: 2, 12: 2, 8: 2}, xch
    for Dd, (nbytes, fits) in lds.items():
        words = (Dd + 1) & ~1
        assert nbytes == 70 * (192 + 256) * 2 + 4 * words * 4 + 4 * 2 * 2 * 76 * 4, (Dd, nbytes)   # the per-band tail's figure
        assert 2 * words * 4 + 1 * 2 * 76 * 4 <= words * 4 + 2 * 2 * 76 * 4, "two tables and one row inside one table and two rows"
        assert fits == 1 and 2 * (-(-nbytes // 1280) * 1280) <= 160 * 1024 < 3 * (-(-nbytes // 1280) * 1280), (Dd, nbytes)
    assert set(lds) == {2, 33, 64, 67}


def _covered(wu, wl, ms):
    """Every needed (disparity, unit band, row) lies in a march of that disparity over that unit band, under its row mask."""
    got_u, got_l = [0] * len(wu), [0] * len(wl)
    for kind, da, db, lo, hi in ms:
        mask = lo | (hi << 32)
        for d in {da, db}:
            if kind == "full":
                got_u[d] |= mask & 0xffffff
                got_l[d] |= mask >> st.FA_TH
            elif kind == "upper":
                got_u[d] |= mask
            else:
                got_l[d] |= mask
    return all(wu[d] & ~got_u[d] == 0 and wl[d] & ~got_l[d] == 0 for d in range(len(wu)))


def test_random_needed_sets_never_march_more_rows():
    rng = np.random.default_rng(8)
    seen = set()
    for trial in range(1000):
        Dd = int(rng.integers(2, 68))
        pu, pl = rng.random(2) * rng.choice([0.05, 0.3, 1.0])
        wu = [int(rng.integers(1, 1 << 24)) if rng.random() < pu else 0 for _ in range(Dd)]
        wl = [int(rng.integers(1, 1 << 24)) if rng.random() < pl else 0 for _ in range(Dd)]
        b, u, l = st.classes(wu, wl)
        ms, code = st.marches(wu, wl)
        seen.add(code)
        joint, halves = st.rows_of_marches(ms), st.rows_halves(len(b), len(u), len(l))
        assert joint == st.rows_joint(len(b), len(u), len(l)) and joint <= halves, (trial, len(b), len(u), len(l), joint, halves)
        assert _covered(wu, wl, ms), trial
        marched = sorted(d for m in ms for d in {m[1], m[2]})
        assert set(marched) == set(b) | set(u) | set(l), "exactly the needed disparities are marched"
    assert seen == set(range(8)), seen


def _ocfg(case):
    import oracle_lib
    K = case["K"]
    return oracle_lib.OracleConfig(height=case["h"] * K, width=case["w"] * K, downscale_factor=K, min_disparity=0,
                                   max_disparity=case["Dd"] * K - 1)


_CODES = {}


@pytest.mark.parametrize("case", st.CASES, ids=[c["name"] for c in st.CASES])
def test_every_gpu_input_reaches_every_march_form(oracle_omp, case):
    Dd = case["Dd"]
    has = dict(both=0, upper=0, lower=0, odd_both=0, odd_upper=0, odd_lower=0, hi_rows=0, winner_0=0, winner_last=0)
    codes = [0] * 8
    for _, _, _, im in st.oracle_runs(oracle_omp, _ocfg(case), case):
        a = im["wta_index"]
        assert a.shape == (case["h"], case["w"])
        has["winner_0"] += int((a == 0).sum())
        has["winner_last"] += int((a == Dd - 1).sum())
        for _, _, win in st.windows(a):
            wu, wl = st.window_tables(win, Dd)
            b, u, l = st.classes(wu, wl)
            ms, code = st.marches(wu, wl)
            assert st.rows_of_marches(ms) == st.rows_joint(len(b), len(u), len(l)) <= st.rows_halves(len(b), len(u), len(l))
            assert _covered(wu, wl, ms)
            codes[code] += 1
            has["both"] += len(b) > 0
            has["upper"] += len(u) > 0
            has["lower"] += len(l) > 0
            has["odd_both"] += len(b) & 1
            has["odd_upper"] += len(u) & 1
            has["odd_lower"] += len(l) & 1
            has["hi_rows"] += any(m[0] == "full" and m[4] != 0 for m in ms)
    _CODES[case["name"]] = codes
    print(f"{case['name']}: {has}, leftover codes {codes}")
    absent = set()
    if "lower" in case["lacks"]:             # no image row in the lower unit band: nothing but "upper only"
        absent |= {"both", "lower", "odd_both", "odd_lower"}
    if "hi_rows" in case["lacks"]:
        absent |= {"hi_rows"}
    for k, v in has.items():
        assert (v == 0) if k in absent else (v > 0), (case["name"], k, has)


def test_all_inputs_together_reach_every_leftover_code(oracle_omp):
    for case in st.CASES:
        if case["name"] not in _CODES:
            test_every_gpu_input_reaches_every_march_form(oracle_omp, case)
    total = [sum(c[k] for c in _CODES.values()) for k in range(8)]
    assert all(v > 0 for v in total), total


def test_the_geometry_of_the_cases_is_what_their_names_say():
    by = st.CASES_BY_NAME
    assert by["30x190_lower_6_rows"]["h"] - st.FA_TH == 6 and by["24x190_lower_empty"]["h"] == st.FA_TH
    assert by["54x190_second_band_6_rows"]["h"] - st.FA_STACK_TH == 6
    assert by["48x64_one_partial_window"]["w"] - st.FA_VALID == 22          # a full window and one of 22 columns: one active... two waves
    assert by["48x190_range_67"]["Dd"] == 256 - 190 + 1                       # the most a pitch-256 right tile holds
    assert by["48x190_k4_sliding"]["K"] == 4 and by["48x190_prefix"]["K"] == 2  # fast_prefix_form: K <= 2 only
    assert set(st.REPORT_CASES) <= set(by)
