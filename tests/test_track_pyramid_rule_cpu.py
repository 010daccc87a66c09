"""The rules of smx_intensity_pyramid and smx_track_camera_pyramid without a GPU: tests/track_pyramid_rule_harness.cpp
compiles the library's reduce rule and per-pixel terms (stereo-depth_amd/csrc/k_track_pyramid_rule.h over
k_track_photo_rule.h, the code the kernels run) for the host, builds both pyramids and runs whole schedules over the cases
of tests/track_pyramid_cases.py, summing in the header's order.  Every output, the pyramids included, must equal the NumPy
twin's (tests/track_pyramid_ref.py) bit for bit; with every level 0 and huber_delta = inf the outputs must equal the
photometric twin's.

Built like the photometric rule's harness (host code only, no HIP runtime linked), with the address and
undefined-behaviour sanitizers when their runtimes link that way and without them otherwise.  No GPU."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import track_cases as tc
import track_photo_cases as pc
import track_pyramid_cases as yc
import track_pyramid_ref as ty
import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "track_pyramid_rule_harness.cpp")
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
    exe = str(tmp_path_factory.mktemp("track_pyramid_rule") / "track_pyramid_rule")
    log = ""
    for extra in (SANITIZE, []):
        cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + extra + ["-I", b.INCLUDE, "-I", b.CSRC,
                                                                                                "-o", exe, HARNESS]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode == 0:
            print("track-pyramid-rule harness built", "with -fsanitize=address,undefined" if extra else "WITHOUT the sanitizers")
            return exe
        log += " ".join(cmd) + "\n" + r.stdout + r.stderr + "\n"
    raise AssertionError("harness did not compile:\n" + log[-6000:])


def run_arrays(harness, tmp_path, disp, Q, starts, models, intensity, weight, max_difference, schedule, schedule_levels,
               levels, huber_delta=np.inf, conf=None, **kw):
    """disp, intensity, conf: [n, H, W]; starts: [n, 3, 4]; models: n dicts sharing Qm and Pm, with "intensity"; returns
    (one result dict per triple, the frame pyramid's levels [n, Hl, Wl], the model pyramid's)."""
    n, H, W = disp.shape
    Hm, Wm = models[0]["depth"].shape
    sched = np.zeros((8, 2), np.int32)
    sched[:len(schedule)] = np.asarray(schedule, np.int32).reshape(-1, 2)
    slev = np.zeros(8, np.int32)
    slev[:len(schedule_levels)] = schedule_levels
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([n, H, W, Hm, Wm, int(conf is not None), len(schedule), kw["min_inliers"], levels], np.int32).tofile(f)
        sched.tofile(f)
        slev.tofile(f)
        np.array([kw.get("min_confidence", 0.0), kw["depth_range"][0], kw["depth_range"][1], -1.0, kw["max_distance"],
                  kw["min_pivot"], kw.get("rot_eps", 0.0), kw.get("trans_eps", 0.0), weight, max_difference, huber_delta],
                 f32).tofile(f)
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
    assert re.search(rf"^track-pyramid-rule triples {n} iterations \d+$", r.stdout, re.M), r.stdout
    raw = np.fromfile(outp, np.uint8)
    fdims, mdims = ty.level_dims(H, W, levels), ty.level_dims(Hm, Wm, levels)
    sizes = [48 * n, 16 * n, 4 * n, 264 * n, 8 * n, 4 * n] + [4 * n * h * w for h, w in fdims + mdims]
    assert raw.size == sum(sizes)
    at = np.cumsum([0] + sizes)
    part = [raw[at[i]:at[i + 1]] for i in range(len(sizes))]
    pose, info = part[0].view(f32).reshape(n, 3, 4), part[1].view(np.int32).reshape(n, 4)
    rms, sums = part[2].view(f32), part[3].view(np.float64).reshape(n, 33)
    pinfo, prms = part[4].view(np.int32).reshape(n, 2), part[5].view(f32)
    fpyr = [part[6 + l].view(f32).reshape(n, h, w) for l, (h, w) in enumerate(fdims)]
    mpyr = [part[6 + levels + l].view(f32).reshape(n, h, w) for l, (h, w) in enumerate(mdims)]
    res = [{"pose": pose[i], "info": info[i], "rms": rms[i], "sums": sums[i], "pinfo": pinfo[i], "prms": prms[i]}
           for i in range(n)]
    return res, fpyr, mpyr


def run(harness, tmp_path, triples, schedule=yc.SCHEDULE, schedule_levels=yc.SCHEDULE_LEVELS, levels=yc.LEVELS,
        huber_delta=np.inf, weight=pc.WEIGHT, clean=False, **extra):
    """triples: (view, shape, k, confidence, misses) with one frame shape."""
    kw = dict(tc.PARAMS)
    kw.update(extra)
    frames = [tc.frame(v, s, k, c) for v, s, k, c, _ in triples]
    conf = triples[0][3]
    if conf:
        kw.setdefault("min_confidence", 0.1)
    return run_arrays(harness, tmp_path, np.stack([fr[0] for fr in frames]), frames[0][1],
                      np.stack([tc.start_pose(t[0]) for t in triples]), [yc.model(v, m, levels, clean) for v, _, _, _, m in triples],
                      np.stack([pc.frame_intensity(s, k) for _, s, k, _, _ in triples]), weight, pc.MAX_DIFFERENCE, schedule,
                      schedule_levels, levels, huber_delta, conf=np.stack([fr[3] for fr in frames]) if conf else None, **kw)


@pytest.mark.parametrize("shape", tc.FRAME_SHAPES)
def test_the_schedule_through_three_levels_and_the_pyramids(harness, tmp_path, shape):
    got, fpyr, mpyr = run(harness, tmp_path, [("outside", shape, 0, False, False)])
    want = yc.expected("outside", shape)
    assert want["info"][0] == 0 and want["info"][1] == 7 and want["pinfo"][0] > 100
    yc.assert_same(got[0], want, f"{shape}")
    for l in range(yc.LEVELS):
        assert yc.same_planes(fpyr[l][0], yc.frame_pyramid(shape)[l]), f"frame level {l}"
        assert yc.same_planes(mpyr[l][0], yc.model("outside")["pyramid"][l]), f"model level {l}"
    assert np.isnan(mpyr[2]).any() and np.isfinite(mpyr[2]).any()


@pytest.mark.parametrize("schedule, schedule_levels", [(((4, 2),), (1,)), (((6, 2),), (1,)), (((4, 1), (1, 1)), (0, 0))])
def test_levels_below_the_strides_own(harness, tmp_path, schedule, schedule_levels):
    shape = tc.FRAME_SHAPES[0]
    got, _, _ = run(harness, tmp_path, [("left", shape, 1, False, False)], schedule, schedule_levels)
    yc.assert_same(got[0], yc.expected("left", shape, 1, schedule=schedule, schedule_levels=schedule_levels),
                   f"{schedule} at {schedule_levels}")


@pytest.mark.parametrize("shape", tc.FRAME_SHAPES)
@pytest.mark.parametrize("level", [0, 1, 2])
def test_every_sum_of_one_iteration_at_each_level(harness, tmp_path, level, shape):
    schedule = ((1 << level, 1),)
    want = yc.expected("left", shape, 1, schedule=schedule, schedule_levels=(level,), huber_delta=yc.HUBER, clean=True)
    assert np.count_nonzero(want["sums"]) == 33 and want["pinfo"][0] >= 12
    got, _, _ = run(harness, tmp_path, [("left", shape, 1, False, False)], schedule, (level,), huber_delta=yc.HUBER,
                    clean=True)
    yc.assert_same(got[0], want, f"level {level}")


@pytest.mark.parametrize("confidence", [False, True])
def test_three_triples_with_the_middle_one_lost_and_a_finite_huber_delta(harness, tmp_path, confidence):
    shape = tc.FRAME_SHAPES[0]
    triples = [("outside", shape, 0, confidence, False), ("left", shape, 1, confidence, True),
               ("left", shape, 2, confidence, False)]
    got, _, _ = run(harness, tmp_path, triples, huber_delta=yc.HUBER)
    for g, (v, s, k, c, m) in zip(got, triples):
        yc.assert_same(g, yc.expected(v, s, k, c, m, huber_delta=yc.HUBER), f"{v} k {k} confidence {c} misses {m}")
    assert [int(g["info"][0]) for g in got] == [0, 1, 0]
    assert np.array_equal(got[1]["pose"].view(np.uint32), tc.start_pose("left").view(np.uint32))


def test_level_0_without_huber_is_the_photometric_rule(harness, tmp_path):
    shape = tc.FRAME_SHAPES[0]
    triples = [("outside", shape, 0, True, False), ("left", shape, 1, True, True), ("left", shape, 2, True, False)]
    got, _, _ = run(harness, tmp_path, triples, tr.DEFAULT_SCHEDULE, (0, 0, 0))
    for g, (v, s, k, c, m) in zip(got, triples):
        pc.assert_same(g, pc.expected(v, s, k, c, m), f"{v} k {k} against the photometric twin")


def test_the_wall(harness, tmp_path):
    d, Q, inten, _ = yc.wall_frame()
    _, _, want = yc.wall_expected()
    got, _, _ = run_arrays(harness, tmp_path, d[None], Q, yc.wall_start()[None], [yc.wall_model()], inten[None], yc.WALL_WEIGHT,
                           yc.WALL_MAX_DIFFERENCE, yc.WALL_SCHEDULE, yc.WALL_SCHEDULE_LEVELS, yc.WALL_LEVELS, yc.WALL_HUBER,
                           **yc.WALL_PARAMS)
    yc.assert_same(got[0], want, "wall")


@pytest.mark.parametrize("name", yc.EDGE_NAMES)
def test_the_edges_of_the_tap_rule_at_level_1(harness, tmp_path, name):
    disp, Q, start, m, frame, weight, max_difference = yc.edge_case(name)
    got, _, mpyr = run_arrays(harness, tmp_path, disp[None], Q, start[None], [m], frame[0][None], weight, max_difference,
                              ((2, 1),), (1,), yc.EDGE_LEVELS, **yc.EDGE_PARAMS)
    assert yc.same_planes(mpyr[1][0], m["pyramid"][1])
    yc.assert_same(got[0], yc.edge_expected(name), name)
    count = yc.EDGE_COUNTS[name]
    assert got[0]["info"][2] == 1 and got[0]["pinfo"].tolist() == [count, 1 - count]


@pytest.mark.parametrize("delta", [3.0, 2.0, np.inf])
def test_hubers_threshold(harness, tmp_path, delta):
    disp, Q, start, m, frame, weight, max_difference = yc.huber_case()
    got, _, _ = run_arrays(harness, tmp_path, disp[None], Q, start[None], [m], frame[0][None], weight, max_difference,
                           ((1, 1),), (0,), 1, delta, **pc.EDGE_PARAMS)
    yc.assert_same(got[0], yc.huber_expected(delta), f"delta {delta}")
    assert got[0]["sums"][31] == (float(f32(2.0) / f32(3.0)) if delta == 2.0 else 1.0)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (2, 3), (5, 1), (67, 131)])
def test_the_reduce_rule_on_small_and_odd_planes(harness, tmp_path, shape):
    """The pyramid alone: a schedule of no pairs, the frame's planes those of the pyramid cases."""
    planes, mask = yc.pyramid_planes(2, shape, masked=True)
    levels = 4
    m = dict(pc.edge_case("inside")[3])
    n = 2
    Hm, Wm = shape
    models = [dict(m, depth=mask[i], normals=np.zeros((3, Hm, Wm), f32), intensity=planes[i]) for i in range(n)]
    got, fpyr, mpyr = run_arrays(harness, tmp_path, np.zeros((n,) + shape, f32), m["Qm"], np.zeros((n, 3, 4), f32), models,
                                 planes, 0.0, 1.0, (), (), levels, **pc.EDGE_PARAMS)
    for l, (a, b) in enumerate(zip(yc.pyramid_expected(n, shape, levels), yc.pyramid_expected(n, shape, levels, True))):
        assert yc.same_planes(fpyr[l], a), f"level {l}"
        assert yc.same_planes(mpyr[l], b), f"masked level {l}"
    assert all(g["info"].tolist() == [0, 0, 0, 0] for g in got)
