"""Box sums from prefix sums in the fast aggregation kernel (k_match_fast.h: fast_pass_pair<..., PREFIX>): when are the
differences of prefixes the same bits as the sliding sums?

tests/prefix_sums_ref.py runs both recurrences of one 64-column window in float32, in the kernel's operation order, on
integer inputs.  Every quantity is an integer in units of 1 / K^2; the two forms agree bit for bit while every prefix stays
an exact float32 integer, and the largest prefix is PH at tile row TH + 10: (TH + 11) * 48,195 * K^2 on saturated content
(s = 255 K^2 everywhere).  Checked here:
  * K = 2 (and K = 1), TH in {8, 12, 24, 27, 32, 48}: saturated and near-saturated inputs (s in {255 K^2 - 1, 255 K^2}, which
    makes every partial sum odd or even at random: the lowest bit is what rounding would lose) give the same (Vs, Cs, Hs)
    on every output row, equal to the sums in float64;
  * K = 2: the same holds at TH = 76, the last height the rule allows, and fails at TH = 77 on the near-saturated input;
  * K = 4, TH = 48: the largest prefix is 45.5 M > 2^24 and the near-saturated input gives different bits -- the reason
    for the bound.  (Exactly saturated input does NOT differ there: with s = 255 * 16 everywhere every sum is a multiple
    of 16 and stays representable up to 2^28.  The test asserts that too, so that nobody takes the saturated image for the
    proof that K = 4 is safe.)
  * fast_prefix_exact / fast_prefix_form themselves through tests/prefix_exact_harness.cpp, compiled for the host.
No GPU."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import prefix_sums_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "prefix_exact_harness.cpp")
HEIGHTS = [8, 12, 24, 27, 32, 48]


def _inputs(K, th, seed):
    top = 255 * K * K
    rng = np.random.default_rng(seed)
    sat = np.full((th + 22, 64), top, np.float32)
    near = (top - rng.integers(0, 2, (th + 22, 64))).astype(np.float32)
    return {"saturated": sat, "near_saturated": near}


@pytest.mark.parametrize("K", [2, 1])
@pytest.mark.parametrize("th", HEIGHTS + [76])
def test_prefix_form_gives_the_bits_of_the_sliding_sums(K, th):
    for name, s in _inputs(K, th, 100 * K + th).items():
        old = ref.sliding(s)
        new, largest = ref.prefix(s)
        assert largest < 2 ** 24, (name, largest)
        if name == "saturated":
            assert largest == (th + 11) * 48195 * K * K            # the figure fast_prefix_exact bounds
        assert old.shape == (3, th, ref.VALID)
        assert np.array_equal(old.view(np.uint32), new.view(np.uint32)), f"K={K} TH={th} {name}: (Vs, Cs, Hs) differ"
        assert np.array_equal(new.astype(np.float64), ref.exact_in_float64(s)), f"K={K} TH={th} {name}: not the exact sums"


def test_one_row_past_the_bound_at_k2_the_bits_differ():
    s = _inputs(2, 77, 7)["near_saturated"]
    new, largest = ref.prefix(s)
    assert largest >= 2 ** 24
    assert not np.array_equal(ref.sliding(s), new)
    assert np.array_equal(ref.sliding(s).astype(np.float64), ref.exact_in_float64(s))     # the sliding sums stay exact


def test_k4_at_48_rows_is_why_the_form_is_bound_to_k2():
    ins = _inputs(4, 48, 11)
    new_sat, largest = ref.prefix(ins["saturated"])
    assert largest == 59 * 48195 * 16 and largest > 2 ** 24
    new, _ = ref.prefix(ins["near_saturated"])
    old = ref.sliding(ins["near_saturated"])
    assert np.array_equal(old.astype(np.float64), ref.exact_in_float64(ins["near_saturated"]))
    wrong = int((old != new).sum())
    assert wrong > 0, "K = 4, TH = 48: the prefix form must lose bits on near-saturated input"
    # exactly saturated: all sums are multiples of 16 -- exact although they exceed 2^24
    assert np.array_equal(ref.sliding(ins["saturated"]), new_sat)


def _build_module():
    spec = importlib.util.spec_from_file_location("smx_build", os.path.join(ROOT, "stereo-depth_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not found")
    b = _build_module()
    exe = str(tmp_path_factory.mktemp("prefix_exact") / "prefix_exact")
    cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + ["-I", b.INCLUDE, "-I", b.CSRC, "-o", exe, HARNESS]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "harness did not compile:\n" + r.stdout + r.stderr
    return exe


def test_the_exactness_rule_of_the_engine(harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=120)
    summary = re.search(r"^prefix-exact checks (\d+) failures (\d+)$", r.stdout, re.M)
    assert summary, r.stdout[-2000:] + r.stderr[-2000:]
    checks, failures = map(int, summary.groups())
    failed = [ln for ln in r.stdout.splitlines() if ln.startswith("failed")]
    assert failures == 0 and r.returncode == 0, "\n".join(failed)
    assert checks >= 500, summary.group(0)
