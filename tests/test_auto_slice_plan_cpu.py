"""Host-side launch plans of the disparity-split kernels against the slice buffer they write into.

The one-launch AUTO kernel (k_match_auto.h) turns the workgroups of off-grid pairs into disparity slices that write
partial arg-max records at [slice][word][pair][h][w] into the calling stream lane's region of the engine's slice buffer;
the split exact-order launch (smx_plan.h: exact_launch) does the same for calls of up to 4 pairs.  A record written past the region
lands in the other lane's region or past the allocation.  tests/auto_slice_plan_harness.cpp compiles the library's own
plan functions (match_fast_plan, match_auto_nsplit, the launch gate, exact_split and slice_region_floats, which sizes the
region in smx_create) for the host and sweeps them over frame shapes up to C4's, disparity counts, batch limits, stream-lane
modes and CU counts.  No GPU and no HIP runtime involved."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "auto_slice_plan_harness.cpp")


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
    exe = str(tmp_path_factory.mktemp("slice_plan") / "slice_plan")
    # build.py's flags and include directories; host code only, and no HIP runtime linked (-no-hip-rt): the harness
    # calls nothing but the inline plan functions of the kernel headers
    cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + ["-I", b.INCLUDE, "-I", b.CSRC,
                                                                                    "-o", exe, HARNESS]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "harness did not compile:\n" + r.stdout + r.stderr
    return exe


def test_every_accepted_launch_writes_inside_the_lane_region(harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=600)
    summary = re.search(r"^checked (\d+) accepted (\d+) split (\d+) violations (\d+)$", r.stdout, re.M)
    assert summary, r.stdout[-2000:] + r.stderr
    configs, accepted, split, violations = map(int, summary.groups())
    overflows = [ln for ln in r.stdout.splitlines() if ln.startswith("overflow")]
    assert violations == 0 and r.returncode == 0, (
        f"{violations} launch plans write slice records past the lane region "
        "(kind h w Dd B n on_lanes cus nsplit th need_floats region_floats):\n" + "\n".join(overflows))
    # the sweep reached both kinds of launch, many times over
    assert configs > 100_000 and accepted > 1_000_000 and split > 100_000, summary.group(0)
