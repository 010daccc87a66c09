"""The march of smx_tsdf_raycast without a GPU: tests/raycast_march_harness.cpp compiles the library's per-pixel rule
(stereo-depth_amd/csrc/k_raycast_rule.h: the code every thread of the kernel runs, with its jumps over empty bricks and
over the space outside the volume's box) for the host and runs it over the cases of tests/raycast_cases.py.  Its five
outputs must equal the dense NumPy twin's bit for bit: what a jump skips never changes a result.

Built like the launch-plan harness (host code only, no HIP runtime linked), with the address and undefined-behaviour
sanitizers when their runtimes link that way and without them otherwise, so an index outside the volume, the brick bytes
or the outputs stops the run.  No GPU."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import raycast_cases as cases
import raycast_ref as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "raycast_march_harness.cpp")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
f32 = np.float32


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
    exe = str(tmp_path_factory.mktemp("raycast_march") / "raycast_march")
    log = ""
    for extra in (SANITIZE, []):
        cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + extra + ["-I", b.INCLUDE, "-I", b.CSRC,
                                                                                                "-o", exe, HARNESS]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode == 0:
            print("raycast-march harness built", "with -fsanitize=address,undefined" if extra else "WITHOUT the sanitizers")
            return exe
        log += " ".join(cmd) + "\n" + r.stdout + r.stderr + "\n"
    raise AssertionError("harness did not compile:\n" + log[-6000:])


def march(harness, tmp_path, state, Q, poses, shape, min_weight, step, depth_range, dims=cases.DIMS, origin=cases.ORIGIN,
          vs=cases.VS):
    """The harness's five outputs as raycast_ref's dict, and the fraction of bricks it found occupied."""
    H, W = shape
    poses = rc.view_pose(poses)
    n = poses.shape[0]
    M = rc.sample_count(depth_range[0], depth_range[1], f32(step))
    colour = state["color"] is not None
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array(list(dims) + [n, H, W, M, int(colour)], np.int32).tofile(f)
        np.array(list(origin) + [vs, min_weight, step, depth_range[0], -1.0], np.float32).tofile(f)
        np.asarray(Q, np.float32).tofile(f)
        poses.tofile(f)
        state["tsdf"].astype(np.float32).tofile(f)
        state["weight"].astype(np.float32).tofile(f)
        if colour:
            np.ascontiguousarray(state["color"]).tofile(f)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness, inp, outp], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    summary = re.search(r"^raycast-march pixels (\d+) bricks (\d+) set (\d+) free (\d+)$", r.stdout, re.M)
    assert summary and int(summary.group(1)) == n * H * W, r.stdout
    P = n * H * W
    raw = np.fromfile(outp, np.uint8)
    assert raw.size == 4 * P * 6 + (3 * P if colour else 0)
    fl = raw[:24 * P].view(np.float32)
    out = {"disparity": fl[:P].reshape(n, H, W), "depth": fl[P:2 * P].reshape(n, H, W),
           "normals": fl[2 * P:5 * P].reshape(n, 3, H, W), "weight": fl[5 * P:6 * P].reshape(n, H, W),
           "colors": raw[24 * P:].reshape(n, 3, H, W) if colour else None}
    march.free_bricks = int(summary.group(4))
    return out, int(summary.group(3)) / int(summary.group(2))


ALL_VIEWS = ("outside", "inside", "behind", "oblique")


@pytest.mark.parametrize("qkind", cases.QKINDS)
@pytest.mark.parametrize("step_voxels", cases.STEPS)
@pytest.mark.parametrize("min_weight", cases.MIN_WEIGHTS)
def test_march_equals_the_dense_rule(harness, tmp_path, qkind, step_voxels, min_weight):
    want = cases.expected(ALL_VIEWS, qkind, step_voxels, min_weight)
    got, _ = march(harness, tmp_path, cases.fused_state(), cases.q_of(qkind), cases.poses_of(ALL_VIEWS), cases.SHAPE,
                   min_weight, f32(cases.VS) * f32(step_voxels), cases.DEPTH_RANGE)
    cases.assert_same(got, want, f"{qkind} step {step_voxels} min_weight {min_weight}")
    hits = np.isfinite(want["depth"]).reshape(len(ALL_VIEWS), -1).mean(axis=1)
    if min_weight == 1.0:
        assert hits[0] > 0.5 and hits[1] > 0.3 and hits[3] > 0.1, hits          # the views do see the surface
    assert hits[2] == 0                                                          # looking away


@pytest.mark.parametrize("qkind", ["centred", "middlebury"])
def test_rays_along_an_axis_from_a_voxel_centre(harness, tmp_path, qkind):
    want = cases.expected(("aligned",), qkind, 1.0, 1.0)
    got, _ = march(harness, tmp_path, cases.fused_state(), cases.q_of(qkind), cases.poses_of(("aligned",)), cases.SHAPE,
                   1.0, f32(cases.VS), cases.DEPTH_RANGE)
    cases.assert_same(got, want, f"aligned {qkind}")
    assert np.isfinite(want["depth"][0, 16, 22])                                 # the ray with dw = (0, 0, 1) hits


def test_a_volume_measured_in_one_corner(harness, tmp_path):
    state = cases.fused_state(True, True)
    assert 0 < cases.occupied_bricks(state, 1.0) < 0.3
    for step_voxels in (0.5, 2.5):
        want = cases.expected(ALL_VIEWS, "kitti", step_voxels, 1.0, True, True)
        got, occupied = march(harness, tmp_path, state, cases.q_of("kitti"), cases.poses_of(ALL_VIEWS), cases.SHAPE, 1.0,
                              f32(cases.VS) * f32(step_voxels), cases.DEPTH_RANGE)
        assert occupied == cases.occupied_bricks(state, 1.0)
        cases.assert_same(got, want, f"corner, step {step_voxels}")
    assert np.isfinite(want["depth"]).any()


@pytest.mark.parametrize("step_voxels", cases.STEPS)
def test_measured_free_space_is_jumped_without_a_change(harness, tmp_path, step_voxels):
    """A ball in measured free space: most bricks are free (every corner measured, tsdf exactly 1) and are crossed in
    jumps that leave "valid, T = 1" behind; the hit behind them needs that state."""
    want = cases.expected_analytic(ALL_VIEWS, step_voxels)
    got, occupied = march(harness, tmp_path, cases.analytic_state(), cases.q_of("kitti"), cases.poses_of(ALL_VIEWS),
                          cases.SHAPE, 1.0, f32(cases.VS) * f32(step_voxels), cases.DEPTH_RANGE)
    assert march.free_bricks >= 20 and occupied < 1.0                            # free, mixed and empty bricks
    cases.assert_same(got, want, f"ball in free space, step {step_voxels}")
    assert np.isfinite(want["depth"][0]).mean() > 0.05 and np.isfinite(want["depth"][3]).any()


def test_no_colour_volume_empty_volume_and_long_rays(harness, tmp_path):
    state = cases.fused_state(False)
    want = cases.expected(ALL_VIEWS, "kitti", 1.0, 1.0, False)
    got, _ = march(harness, tmp_path, state, cases.q_of("kitti"), cases.poses_of(ALL_VIEWS), cases.SHAPE, 1.0,
                   f32(cases.VS), cases.DEPTH_RANGE)
    assert got["colors"] is None and want["colors"] is None
    cases.assert_same(got, want, "no colour")
    empty = {k: None if v is None else np.zeros_like(v) for k, v in state.items()}
    got, occupied = march(harness, tmp_path, empty, cases.q_of("kitti"), cases.poses_of(ALL_VIEWS), cases.SHAPE, 1.0,
                          f32(cases.VS), cases.DEPTH_RANGE)
    assert occupied == 0 and (got["disparity"] == -1.0).all() and np.isnan(got["depth"]).all()
    # thousands of samples past the box, and a range that starts inside the volume
    for depth_range in ((0.0, 40.0), (1.2, 3.0)):
        want = cases.expected(("outside", "oblique"), "kitti", 0.2, 1.0, True, False, depth_range)
        got, _ = march(harness, tmp_path, cases.fused_state(), cases.q_of("kitti"), cases.poses_of(("outside", "oblique")),
                       cases.SHAPE, 1.0, f32(cases.VS) * f32(0.2), depth_range)
        cases.assert_same(got, want, f"range {depth_range}")
