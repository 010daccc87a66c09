"""The rule of smx_track_camera_photometric without a GPU: tests/track_photo_rule_harness.cpp compiles the library's
per-pixel terms (stereo-depth_amd/csrc/k_track_photo_rule.h, the code the kernels run) for the host and runs whole
schedules over the cases of tests/track_photo_cases.py, summing in the header's order.  Every output must equal the NumPy
twin's (tests/track_photo_ref.py) bit for bit; with a weight of 0 the outputs the two entries share must equal the
geometric twin's.

Built like the geometric rule's harness (host code only, no HIP runtime linked), with the address and undefined-behaviour
sanitizers when their runtimes link that way and without them otherwise.  No GPU."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import track_cases as tc
import track_photo_cases as pc
import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "track_photo_rule_harness.cpp")
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
    exe = str(tmp_path_factory.mktemp("track_photo_rule") / "track_photo_rule")
    log = ""
    for extra in (SANITIZE, []):
        cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + extra + ["-I", b.INCLUDE, "-I", b.CSRC,
                                                                                                "-o", exe, HARNESS]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode == 0:
            print("track-photo-rule harness built", "with -fsanitize=address,undefined" if extra else "WITHOUT the sanitizers")
            return exe
        log += " ".join(cmd) + "\n" + r.stdout + r.stderr + "\n"
    raise AssertionError("harness did not compile:\n" + log[-6000:])


def run_arrays(harness, tmp_path, disp, Q, starts, models, intensity, weight, max_difference, schedule, conf=None, **kw):
    """disp, intensity, conf: [n, H, W]; starts: [n, 3, 4]; models: n dicts sharing Qm and Pm; returns one result dict
    per triple."""
    n, H, W = disp.shape
    Hm, Wm = models[0]["depth"].shape
    sched = np.zeros((8, 2), np.int32)
    sched[:len(schedule)] = np.asarray(schedule, np.int32).reshape(-1, 2)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([n, H, W, Hm, Wm, int(conf is not None), len(schedule), kw["min_inliers"]], np.int32).tofile(f)
        sched.tofile(f)
        np.array([kw.get("min_confidence", 0.0), kw["depth_range"][0], kw["depth_range"][1], -1.0, kw["max_distance"],
                  kw["min_pivot"], kw.get("rot_eps", 0.0), kw.get("trans_eps", 0.0), weight, max_difference], f32).tofile(f)
        for m in (Q, models[0]["Qm"], models[0]["Pm"]):
            np.asarray(m, f32).tofile(f)
        for key in ("c2w", "w2c"):
            np.stack([m[key] for m in models]).astype(f32).tofile(f)
        np.asarray(starts, f32).tofile(f)
        np.asarray(disp, f32).tofile(f)
        if conf is not None:
            np.asarray(conf, f32).tofile(f)
        np.stack([m["depth"] for m in models]).astype(f32).tofile(f)
        np.stack([m["normals"] for m in models]).astype(f32).tofile(f)
        np.asarray(intensity, f32).tofile(f)
        np.stack([m["intensity"] for m in models]).astype(f32).tofile(f)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness, inp, outp], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert re.search(rf"^track-photo-rule triples {n} iterations \d+$", r.stdout, re.M), r.stdout
    raw = np.fromfile(outp, np.uint8)
    sizes = [48 * n, 16 * n, 4 * n, 264 * n, 8 * n, 4 * n]
    assert raw.size == sum(sizes)
    at = np.cumsum([0] + sizes)
    part = [raw[at[i]:at[i + 1]] for i in range(6)]
    pose, info = part[0].view(f32).reshape(n, 3, 4), part[1].view(np.int32).reshape(n, 4)
    rms, sums = part[2].view(f32), part[3].view(np.float64).reshape(n, 33)
    pinfo, prms = part[4].view(np.int32).reshape(n, 2), part[5].view(f32)
    return [{"pose": pose[i], "info": info[i], "rms": rms[i], "sums": sums[i], "pinfo": pinfo[i], "prms": prms[i]}
            for i in range(n)]


def run(harness, tmp_path, triples, schedule, weight=pc.WEIGHT, **extra):
    """triples: (view, shape, k, confidence, misses) with one frame shape."""
    kw = dict(tc.PARAMS)
    kw.update(extra)
    frames = [tc.frame(v, s, k, c) for v, s, k, c, _ in triples]
    conf = triples[0][3]
    if conf:
        kw.setdefault("min_confidence", 0.1)
    return run_arrays(harness, tmp_path, np.stack([fr[0] for fr in frames]), frames[0][1],
                      np.stack([tc.start_pose(t[0]) for t in triples]), [pc.model(v, m) for v, _, _, _, m in triples],
                      np.stack([pc.frame_intensity(s, k) for _, s, k, _, _ in triples]), weight, pc.MAX_DIFFERENCE, schedule,
                      conf=np.stack([fr[3] for fr in frames]) if conf else None, **kw)


@pytest.mark.parametrize("shape", tc.FRAME_SHAPES)
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_two_iterations_at_each_stride(harness, tmp_path, shape, stride):
    schedule = ((stride, 2),)
    got = run(harness, tmp_path, [("outside", shape, 0, False, False)], schedule)
    pc.assert_same(got[0], pc.expected("outside", shape, schedule=schedule), f"{shape} stride {stride}")


@pytest.mark.parametrize("shape", tc.FRAME_SHAPES)
def test_every_sum_of_one_iteration_and_the_default_schedule(harness, tmp_path, shape):
    got = run(harness, tmp_path, [("left", shape, 1, False, False)], ((1, 1),))
    pc.assert_same(got[0], pc.expected("left", shape, 1, schedule=((1, 1),)), f"one iteration {shape}")
    got = run(harness, tmp_path, [("outside", shape, 0, False, False)], tr.DEFAULT_SCHEDULE)
    pc.assert_same(got[0], pc.expected("outside", shape), f"default schedule {shape}")


@pytest.mark.parametrize("confidence", [False, True])
def test_a_weight_of_zero_is_the_geometric_rule(harness, tmp_path, confidence):
    shape = tc.FRAME_SHAPES[0]
    triples = [("outside", shape, 0, confidence, False), ("left", shape, 1, confidence, True),
               ("left", shape, 2, confidence, False)]
    got = run(harness, tmp_path, triples, tr.DEFAULT_SCHEDULE, weight=0.0)
    for g, (v, s, k, c, m) in zip(got, triples):
        pc.assert_same(g, pc.expected(v, s, k, c, m, weight=0.0), f"{v} k {k} weight 0")
        geo = dict(g, sums=g["sums"][:30])
        tc.assert_same(geo, tc.expected(v, s, k, c, m), f"{v} k {k} against the geometric twin")
    assert [int(g["info"][0]) for g in got] == [0, 1, 0] and got[0]["pinfo"][0] > 0
    assert np.array_equal(got[1]["pose"].view(np.uint32), tc.start_pose("left").view(np.uint32))


@pytest.mark.parametrize("confidence", [False, True])
def test_three_triples_with_the_middle_one_lost(harness, tmp_path, confidence):
    shape = tc.FRAME_SHAPES[0]
    triples = [("outside", shape, 0, confidence, False), ("left", shape, 1, confidence, True),
               ("left", shape, 2, confidence, False)]
    got = run(harness, tmp_path, triples, tr.DEFAULT_SCHEDULE)
    for g, (v, s, k, c, m) in zip(got, triples):
        pc.assert_same(g, pc.expected(v, s, k, c, m), f"{v} k {k} confidence {c} misses {m}")
    assert [int(g["info"][0]) for g in got] == [0, 1, 0]
    assert np.array_equal(got[1]["pose"].view(np.uint32), tc.start_pose("left").view(np.uint32))


@pytest.mark.parametrize("shape", pc.PLANE_SHAPES)
def test_the_plane(harness, tmp_path, shape):
    d, Q, inten = pc.plane_frame(shape)
    _, want = pc.plane_expected(shape)
    got = run_arrays(harness, tmp_path, d[None], Q, pc.plane_start()[None], [pc.plane_model()], inten[None], pc.WEIGHT, 40.0,
                     tr.DEFAULT_SCHEDULE, **pc.PLANE_PARAMS)[0]
    pc.assert_same(got, want, f"plane {shape}")


@pytest.mark.parametrize("name", pc.EDGE_NAMES)
def test_the_edges_of_the_tap_rule(harness, tmp_path, name):
    disp, Q, start, m, inten, weight, max_difference, count = pc.edge_case(name)
    got = run_arrays(harness, tmp_path, disp[None], Q, start[None], [m], inten[None], weight, max_difference, ((1, 1),),
                     **pc.EDGE_PARAMS)[0]
    pc.assert_same(got, pc.edge_expected(name), name)
    assert got["info"][2] == 1 and got["pinfo"].tolist() == [count, 1 - count]


@pytest.mark.parametrize("shape", pc.TREE_SHAPES)
def test_one_iteration_on_the_deep_tree_frames(harness, tmp_path, shape):
    disp, Q = tc.scaled_frame(shape)
    got = run_arrays(harness, tmp_path, disp[None], Q, tc.start_pose(tc.TREE_VIEW)[None], [pc.tree_model()],
                     pc.tree_intensity(shape)[None], pc.WEIGHT, 200.0, ((1, 1),), conf=tc.wide_confidence(shape)[None],
                     **tc.PARAMS)[0]
    pc.assert_same(got, pc.tree_expected(shape), f"tree {shape}")


def test_zero_iterations(harness, tmp_path):
    shape = tc.FRAME_SHAPES[1]
    got = run(harness, tmp_path, [("outside", shape, 0, False, False)], ())[0]
    pc.assert_same(got, pc.expected("outside", shape, schedule=()), "zero iterations")
    assert got["info"].tolist() == [0, 0, 0, 0] and got["pinfo"].tolist() == [0, 0]
    assert np.isnan(got["rms"]) and np.isnan(got["prms"]) and not got["sums"].any()
