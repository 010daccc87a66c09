"""The rule of smx_track_camera without a GPU: tests/track_rule_harness.cpp compiles the library's per-pixel terms, solve
and pose update (stereo-depth_amd/csrc/k_track_rule.h, the code the kernels run) for the host and runs whole schedules
over the triples of tests/track_cases.py, summing in the header's order.  pose_out, info, rms and all thirty sums must
equal the NumPy twin's bit for bit.

Built like the ray-cast march harness (host code only, no HIP runtime linked), with the address and undefined-behaviour
sanitizers when their runtimes link that way and without them otherwise.  No GPU."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import track_cases as tc
import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "track_rule_harness.cpp")
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
    exe = str(tmp_path_factory.mktemp("track_rule") / "track_rule")
    log = ""
    for extra in (SANITIZE, []):
        cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + extra + ["-I", b.INCLUDE, "-I", b.CSRC,
                                                                                                "-o", exe, HARNESS]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode == 0:
            print("track-rule harness built", "with -fsanitize=address,undefined" if extra else "WITHOUT the sanitizers")
            return exe
        log += " ".join(cmd) + "\n" + r.stdout + r.stderr + "\n"
    raise AssertionError("harness did not compile:\n" + log[-6000:])


def run(harness, tmp_path, triples, schedule, **extra):
    """triples: (view, shape, k, confidence, misses) with one frame shape; returns one result dict per triple."""
    kw = dict(tc.PARAMS)
    kw.update(extra)
    frames = [tc.frame(v, s, k, c) for v, s, k, c, _ in triples]
    models = [tc.model(v, m) for v, _, _, _, m in triples]
    conf = triples[0][3]
    n, (H, W), (Hm, Wm) = len(triples), triples[0][1], tc.MODEL_SHAPE
    if conf:
        kw.setdefault("min_confidence", 0.1)
    sched = np.zeros((8, 2), np.int32)
    sched[:len(schedule)] = np.asarray(schedule, np.int32).reshape(-1, 2)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([n, H, W, Hm, Wm, int(conf), len(schedule), kw["min_inliers"]], np.int32).tofile(f)
        sched.tofile(f)
        np.array([kw.get("min_confidence", 0.0), kw["depth_range"][0], kw["depth_range"][1], -1.0, kw["max_distance"],
                  kw["min_pivot"], kw.get("rot_eps", 0.0), kw.get("trans_eps", 0.0)], f32).tofile(f)
        for m in (frames[0][1], models[0]["Qm"], models[0]["Pm"]):
            np.asarray(m, f32).tofile(f)
        for key in ("c2w", "w2c"):
            np.stack([m[key] for m in models]).astype(f32).tofile(f)
        np.stack([tc.start_pose(t[0]) for t in triples]).tofile(f)
        np.stack([fr[0] for fr in frames]).tofile(f)
        if conf:
            np.stack([fr[3] for fr in frames]).tofile(f)
        np.stack([m["depth"] for m in models]).tofile(f)
        np.stack([m["normals"] for m in models]).tofile(f)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness, inp, outp], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert re.search(rf"^track-rule triples {n} iterations \d+$", r.stdout, re.M), r.stdout
    raw = np.fromfile(outp, np.uint8)
    assert raw.size == n * (48 + 16 + 4 + 240)
    pose = raw[:48 * n].view(f32).reshape(n, 3, 4)
    info = raw[48 * n:64 * n].view(np.int32).reshape(n, 4)
    rms = raw[64 * n:68 * n].view(f32)
    sums = raw[68 * n:].view(np.float64).reshape(n, 30)
    return [{"pose": pose[i], "info": info[i], "rms": rms[i], "sums": sums[i]} for i in range(n)]


@pytest.mark.parametrize("shape", tc.FRAME_SHAPES)
@pytest.mark.parametrize("view", tc.MODEL_VIEWS)
def test_the_twin_tracks_the_cases(view, shape):
    """The cases are trackable: not LOST, at least half of the selected accepted pixels are inliers, and the pose ends
    nearer to the frame's true pose than it started."""
    want = tc.expected(view, shape)
    _, _, true_pose, _ = tc.frame(view, shape)
    m0, d0 = tr.pose_error(tc.start_pose(view), true_pose)
    m1, d1 = tr.pose_error(want["pose"], true_pose)
    print(f"{view} {shape}: {m0:.4f} m {d0:.3f} deg -> {m1:.4f} m {d1:.3f} deg, info {want['info']}")
    assert want["info"][0] == 0 and want["info"][1] == 19
    assert 2 * want["info"][2] >= want["info"][3] > 0
    assert m1 < 0.5 * m0 and d1 < 0.5 * d0
    for stride in (1, 2, 3):
        one = tc.expected(view, shape, schedule=((stride, 2),))
        assert one["info"][0] == 0 and 2 * one["info"][2] >= one["info"][3] > 0, (stride, one["info"])


@pytest.mark.parametrize("shape", tc.FRAME_SHAPES)
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_two_iterations_at_each_stride(harness, tmp_path, shape, stride):
    schedule = ((stride, 2),)
    got = run(harness, tmp_path, [("outside", shape, 0, False, False)], schedule)
    tc.assert_same(got[0], tc.expected("outside", shape, schedule=schedule), f"{shape} stride {stride}")


@pytest.mark.parametrize("confidence", [False, True])
def test_three_triples_with_the_middle_one_lost(harness, tmp_path, confidence):
    shape = tc.FRAME_SHAPES[0]
    triples = [("outside", shape, 0, confidence, False), ("left", shape, 1, confidence, True),
               ("left", shape, 2, confidence, False)]
    got = run(harness, tmp_path, triples, tr.DEFAULT_SCHEDULE)
    for g, (v, s, k, c, m) in zip(got, triples):
        tc.assert_same(g, tc.expected(v, s, k, c, m), f"{v} k {k} confidence {c} misses {m}")
    assert [int(g["info"][0]) for g in got] == [0, 1, 0]
    assert np.array_equal(got[1]["pose"].view(np.uint32), tc.start_pose("left").view(np.uint32))


def test_early_stop_and_zero_iterations(harness, tmp_path):
    shape = tc.FRAME_SHAPES[1]
    eps = dict(rot_eps=2e-3, trans_eps=2e-3)
    got = run(harness, tmp_path, [("outside", shape, 0, False, False)], tr.DEFAULT_SCHEDULE, **eps)[0]
    tc.assert_same(got, tc.expected("outside", shape, **eps), "early stop")
    assert 1 <= got["info"][1] < 19 and got["info"][0] == 0
    got = run(harness, tmp_path, [("outside", shape, 0, False, False)], ())[0]
    tc.assert_same(got, tc.expected("outside", shape, schedule=()), "zero iterations")
    assert got["info"].tolist() == [0, 0, 0, 0] and np.isnan(got["rms"]) and not got["sums"].any()
    assert np.array_equal(got["pose"].view(np.uint32), tc.start_pose("outside").view(np.uint32))
