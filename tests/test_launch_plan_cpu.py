"""The engine's launch planner (stereo-depth_amd/csrc/smx_plan.h) against its prediction, its invariants and a hand-written table.

One call's launches are decided in one place: derive_facts() fixes what a configuration admits, plan_range() turns those
facts, the call and the content switches' decision into a RangePlan that enqueue_range executes, and call_kind() predicts
from the same plans which switch a call can report to.  The header is host-only code, so tests/launch_plan_harness.cpp runs
the engine's own lines over configurations (radii, K, min_disparity on the capture and the volume route, pooled shapes, disparity
counts, step-6 radius), match modes, entries, lanes, 1 .. max_batch pairs, whole calls and halves, every decision, the forced
forms and three CU counts, and checks

  1. prediction equals execution: call_kind()'s two flags against what an executor of the plans would hand to the kernels;
  2. the plan invariants (which route may appear when, splits only for whole calls, capture launches, what the fill
     launch publishes, the forms of the fast kernel);
  3. a table of cases written by hand from the rules.  Among them: before any grid report (hint -1) the gated
     exact-order launch of a whole small AUTO call may split the disparity range, exactly as after an off-grid report --
     the rule is `grid_hint != 0`, not `grid_hint == 1`;
  4. the launch specs every plan names for its aggregation launches (kernel instantiation, band height as launched, pitch,
     disparity split, LDS bytes, slice records) against the launcher glue of the time when the launchers still decided
     for themselves, restated by hand in the harness: no difference over the whole sweep; a split fits the lane's slice
     region and belongs to a whole call of at most 4 pairs; a dense form is planned only where its instantiation exists
     (calls planned dense that launch the sparse instantiation are counted); the LDS stays within the raised caps;
  5. the rest of the call: the prologue, step-6 and fill specs against launch_prologue's and launch_fill's own selection
     and enqueue_range's sad_exact and log2k of the time before those specs, the gates and the MatchParams of every
     aggregation launch (smx_plan.h: exact_params ... auto_params) against the lambdas enqueue_range had, all restated by
     hand -- no difference over the sweep, the prologue also with unaligned u8 pointers, plus an extension (K = 8, widths
     that are no multiple of K); the K = 2 prologue only for gray entries with even W, the K = 4 prologue only with W % 4
     == 0 and aligned u8 input; integer step-6 kinds only with kt != 0 and the u8 planes; sad_exact false exactly beyond
     the bound; a split launch has nsplit == split, pairs == n and no tickets; of a gated pair exactly one runs.  The
     summary's first hash covers what it covered before item 5 (it equals the parent's), hash2 the new fields.

Built like the slice-plan harness (host code only, no HIP runtime linked), with the address and undefined-behaviour
sanitizers when their runtimes link that way and without them otherwise.  No GPU."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "launch_plan_harness.cpp")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
ROUTES = ("FILTERED", "EXACT", "FAST", "AUTO_ONE_LAUNCH", "AUTO_GATED")
REFINES = ("FLOAT", "INT", "INT_V", "AUTO", "AUTO_V")
EXACT_KERNELS = ("GENERIC", "GENERIC_VOLUME", "TILED")
FAST_FORMS = ("SPARSE", "PASS1_ONLY", "DENSE", "DENSE_SMALL")


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
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan")
    log = ""
    for extra in (SANITIZE, []):               # with the sanitizers if their runtimes link without the HIP runtime
        cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + extra + ["-I", b.INCLUDE, "-I", b.CSRC,
                                                                                                "-o", exe, HARNESS]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode == 0:
            print("launch-plan harness built", "with -fsanitize=address,undefined" if extra else "WITHOUT the sanitizers (their runtimes did not link)")
            return exe
        log += " ".join(cmd) + "\n" + r.stdout + r.stderr + "\n"
    raise AssertionError("harness did not compile:\n" + log[-6000:])


def test_prediction_invariants_and_directed_table(harness):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness], capture_output=True, text=True, timeout=600, env=env)
    summary = re.search(r"^launch-plan plans (\d+) kinds (\d+) directed (\d+) routes (\d+) (\d+) (\d+) (\d+) (\d+) refused (\d+) "
                        r"refine (\d+) (\d+) (\d+) (\d+) (\d+) hash ([0-9a-f]{16}) violations (\d+) "
                        r"specs (\d+) exact (\d+) (\d+) (\d+) split (\d+) form (\d+) (\d+) (\d+) (\d+) dense-fallback (\d+) "
                        r"hash2 ([0-9a-f]{16}) prologue (\d+) (\d+) (\d+) fill (\d+) (\d+) (\d+) sx0 (\d+) params (\d+)$", r.stdout, re.M)
    assert summary, r.stdout[-3000:] + r.stderr[-3000:]
    print(summary.group(0))
    plans, kinds, directed = (int(v) for v in summary.groups()[:3])
    routes = dict(zip(ROUTES, map(int, summary.groups()[3:8])))
    refused = int(summary.group(9))
    refines = dict(zip(REFINES, map(int, summary.groups()[9:14])))
    violations = int(summary.group(16))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("violation")]
    assert violations == 0 and r.returncode == 0, f"{violations} violations:\n" + "\n".join(lines[:60]) + "\n" + r.stderr[-3000:]
    # the sweep was not vacuous: every route and every step-6 kernel many times over, refusals, predictions, the table
    assert all(v >= 1000 for v in routes.values()), routes
    assert all(v >= 1000 for v in refines.values()), refines
    assert plans > 10_000_000 and kinds > 500_000 and refused >= 1000 and directed >= 30, summary.group(0)
    # the launch specs: more specs than plans compared with the restated launchers, every kernel and form, splits, and
    # the dense calls without a dense instantiation (Dd = 257) -- a finding, NOTES.md "Launch specs"
    specs, split, fallback = int(summary.group(17)), int(summary.group(21)), int(summary.group(26))
    exact = dict(zip(EXACT_KERNELS, map(int, summary.groups()[17:20])))
    forms = dict(zip(FAST_FORMS, map(int, summary.groups()[21:25])))
    assert specs > plans and split >= 1000 and fallback >= 1000, summary.group(0)
    assert all(v >= 1000 for v in exact.values()), exact
    assert all(v >= 1000 for v in forms.values()), forms
    assert directed >= 37, summary.group(0)
    # the rest of the call: every prologue and fill kernel, step 6 beyond the parabola's bound, more parameter sets
    # compared with the restated lambdas than plans, and the directed rows of the three specs and the gates
    prologue = dict(zip(("GENERIC", "K2", "K4"), map(int, summary.groups()[27:30])))
    fill = dict(zip(("FILL_4", "POW2", "GENERIC"), map(int, summary.groups()[30:33])))
    sx0, params = int(summary.group(34)), int(summary.group(35))
    assert all(v >= 1000 for v in prologue.values()), prologue
    assert all(v >= 1000 for v in fill.values()), fill
    assert sx0 >= 1000 and params > plans and directed >= 141, summary.group(0)
