"""When the launch planner stacks the bands of the throughput aggregation kernel (k_match_fast.h: FA_STACK).

tests/stack_plan_harness.cpp runs the engine's own plan functions (smx_plan.h, host-only) on directed cases: a C2 call of
32 pairs on the stream lanes plans th = 24, stack = 2 at pitch 256 (and smx_get_match_geometry's function reports 48-row
bands with 70 marched rows); the same call stays at stack = 1 on a caller's stream, in the dense form, with
min_disparity > 0 (pass1_only), in the latency shape and when SMX_FAST_STACK=0 forbids the form; SMX_FAST_STACK=1 forces it
wherever the instantiation exists (pitch 256) and nowhere else; image heights at which 27-row bands march fewer
rows keep them; and the stacked tile, rounded to the LDS allocation granule, fits a CU's 160 KB twice and not three times.
No GPU."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "stack_plan_harness.cpp")


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
    exe = str(tmp_path_factory.mktemp("stack_plan") / "stack_plan")
    cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + ["-I", b.INCLUDE, "-I", b.CSRC, "-o", exe, HARNESS]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "harness did not compile:\n" + r.stdout + r.stderr
    return exe


def test_stacked_bands_are_planned_by_the_rule(harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=120)
    summary = re.search(r"^stack-plan checks (\d+) failures (\d+)$", r.stdout, re.M)
    assert summary, r.stdout[-2000:] + r.stderr[-2000:]
    checks, failures = map(int, summary.groups())
    failed = [ln for ln in r.stdout.splitlines() if ln.startswith("failed")]
    assert failures == 0 and r.returncode == 0, "\n".join(failed)
    assert checks >= 80, summary.group(0)


def test_the_build_refuses_scratch_and_spills_in_the_stacked_unit():
    """build.py checks the compiler's resource remarks of tu_fast_stack.hip: the march must stay in registers."""
    b = _build_module()
    assert "tu_fast_stack.hip" in b.NO_SCRATCH and "-Rpass-analysis=kernel-resource-usage" in b.PER_FILE_FLAGS["tu_fast_stack.hip"]
    assert "-pragma-unroll-threshold=65536" in b.PER_FILE_FLAGS["tu_fast_stack.hip"]
    clean = "\n".join(["k.h:1:1: remark: Function Name: _ZN3smx12k_match_fastILi48ELi256EEEv [-Rpass-analysis=kernel-resource-usage]",
                       "k.h:1:1: remark:     VGPRs: 186 [-Rpass-analysis=kernel-resource-usage]",
                       "k.h:1:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]",
                       "k.h:1:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]",
                       "k.h:1:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]"])
    b.check_resources("tu_fast_stack.hip", clean)
    for bad in (clean.replace("ScratchSize [bytes/lane]: 0", "ScratchSize [bytes/lane]: 2896"), clean.replace("VGPRs Spill: 0", "VGPRs Spill: 3"),
                clean.replace("SGPRs Spill: 0", "SGPRs Spill: 1"), ""):
        with pytest.raises(RuntimeError):
            b.check_resources("tu_fast_stack.hip", bad)
