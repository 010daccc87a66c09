"""Every workspace layout (stereo-depth_amd/csrc/smx_workspace.h) against what a launcher relies on and against the sizes before.

A size query and the launcher behind it read one layout function, so they cannot disagree; what is left to check is the
layout itself.  The header is host-only code, so tests/workspace_layout_harness.cpp sweeps the library's own lines over
map sizes (n, H, W in 1 .. 32768, up to 2^30 pixels), disparity counts on both sides of SGM's two roundings, point
capacities around the 4096-point tile and up to 2^30, and volumes around the 64-voxel chunk, and checks for each layout that
every part starts on a multiple of 256 bytes, that the parts ascend without touching, that the last ends inside `total`,
that each part has the bytes its kernels index, and that `total` equals a verbatim copy of the expression the launchers
used to carry by hand (kept in the harness).

Built like the launch-plan harness (host code only, no HIP runtime linked), with the address and undefined-behaviour
sanitizers when their runtimes link that way and without them otherwise.  No GPU."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "workspace_layout_harness.cpp")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
# the least number of layouts the sweep must have checked: the sizes of the sets in the harness, less what exceeds 2^30
AT_LEAST = dict(post=900, wls=900, sgm=6300, reproject=900, voxel=18, tsdf_integrate=900, tsdf_extract=300, mesh=300)


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
    exe = str(tmp_path_factory.mktemp("workspace_layout") / "workspace_layout")
    log = ""
    for extra in (SANITIZE, []):               # with the sanitizers if their runtimes link without the HIP runtime
        cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + extra + ["-I", b.INCLUDE, "-I", b.CSRC,
                                                                                                "-o", exe, HARNESS]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode == 0:
            print("workspace-layout harness built", "with -fsanitize=address,undefined" if extra else "WITHOUT the sanitizers (their runtimes did not link)")
            return exe
        log += " ".join(cmd) + "\n" + r.stdout + r.stderr + "\n"
    raise AssertionError("harness did not compile:\n" + log[-6000:])


def test_every_layout_is_aligned_disjoint_and_as_large_as_before(harness):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness], capture_output=True, text=True, timeout=600, env=env)
    summary = re.search(r"^workspace-layout " + " ".join(rf"{k} (\d+)" for k in AT_LEAST) + r" violations (\d+)$", r.stdout, re.M)
    assert summary, r.stdout[-3000:] + r.stderr[-3000:]
    print(summary.group(0))
    counts = dict(zip(AT_LEAST, map(int, summary.groups())))
    violations = int(summary.groups()[-1])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("violation")]
    assert violations == 0 and r.returncode == 0, f"{violations} violations:\n" + "\n".join(lines[:60]) + "\n" + r.stderr[-3000:]
    assert all(counts[k] >= v for k, v in AT_LEAST.items()), counts          # the sweep was not vacuous
