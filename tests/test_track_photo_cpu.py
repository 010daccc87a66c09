"""The rule of smx_track_camera_photometric on the CPU: the NumPy twin (tests/track_photo_ref.py) on the cases of
tests/track_photo_cases.py.  That the term is not idle in the cases the device tests compare (a quarter of the geometric
inliers have it, every new sum is non-zero); that a weight of 0 gives the geometric twin's bits; that the geometric twin
loses the textured plane and the photometric one tracks it to a tenth of the start's error; the edges of the tap rule by
hand; that the deep-tree frames give the combine kernel chunks of more than one partial; the intensity rule; and the
argument errors of the Python layer and of the C entries that need no device.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import track_cases as tc
import track_photo_cases as pc
import track_photo_ref as tp
import track_ref as tr

f32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stereo-depth_amd", "csrc")


def assert_the_term_is_not_idle(want, what):
    assert want["info"][0] == 0, what
    assert 4 * want["pinfo"][0] >= want["info"][2] > 0, (what, want["pinfo"], want["info"])
    assert np.count_nonzero(want["sums"][30:]) == 3 and want["sums"][32] == want["pinfo"][0], what
    assert np.isfinite(want["prms"]) and want["prms"] > 0, what


@pytest.mark.parametrize("shape", tc.FRAME_SHAPES)
def test_the_term_is_not_idle_in_the_bit_cases(shape):
    for stride in (1, 2, 3):
        assert_the_term_is_not_idle(pc.expected("outside", shape, schedule=((stride, 2),)), f"{shape} stride {stride}")
    one = pc.expected("left", shape, 1, schedule=((1, 1),))
    assert_the_term_is_not_idle(one, f"{shape} one iteration")
    assert np.count_nonzero(one["sums"]) == 33
    full = pc.expected("outside", shape)
    assert_the_term_is_not_idle(full, f"{shape} default schedule")
    assert full["info"][1] == 19
    # the term moves the result: the joint system is not the geometric one
    geo = tc.expected("left", shape, 1, schedule=((1, 1),))
    assert not np.array_equal(one["sums"][:27], geo["sums"][:27]) and np.array_equal(one["sums"][27:30], geo["sums"][27:30])
    # NaNs in both planes, and model misses next to hits
    m = pc.model("left")
    assert np.isnan(m["intensity"]).any() and np.isnan(pc.frame_intensity(shape, 1)).any()
    hit = np.isfinite(m["depth"])
    assert (hit[:, 1:] != hit[:, :-1]).any()


@pytest.mark.parametrize("confidence", [False, True])
def test_a_weight_of_zero_gives_the_geometric_twins_bits(confidence):
    shape = tc.FRAME_SHAPES[0]
    for view, k, misses in (("outside", 0, False), ("left", 1, True), ("left", 2, False)):
        got = pc.expected(view, shape, k, confidence, misses, weight=0.0)
        want = tc.expected(view, shape, k, confidence, misses)
        tc.assert_same(dict(got, sums=got["sums"][:30]), want, f"{view} {k}")
        if not misses:
            assert got["pinfo"][0] > 0 and got["sums"][30] > 0       # counted, though every product is +-0.0


@pytest.mark.parametrize("shape", pc.PLANE_SHAPES)
def test_the_geometric_twin_loses_the_plane_and_the_photometric_one_tracks_it(shape):
    geo, photo = pc.plane_expected(shape)
    assert geo["info"][0] == 1 and geo["info"][1] == 1
    assert geo["info"][2] >= pc.PLANE_PARAMS["min_inliers"]          # lost by a pivot, not for want of inliers
    assert np.array_equal(geo["pose"].view(np.uint32), pc.plane_start().view(np.uint32))
    m0, d0 = tr.pose_error(pc.plane_start(), pc.plane_true_pose())
    m1, d1 = tr.pose_error(photo["pose"], pc.plane_true_pose())
    print(f"plane {shape}: {m0:.4f} m {d0:.3f} deg -> {m1:.5f} m {d1:.4f} deg, info {photo['info']} {photo['pinfo']}, "
          f"rms {photo['prms']:.3f}")
    assert 0.03 < m0 < 0.05 and 1.0 < d0 < 1.3
    assert photo["info"][0] == 0 and photo["info"][1] == 19
    assert m1 <= 0.1 * m0 and d1 <= 0.1 * d0


@pytest.mark.parametrize("name", pc.EDGE_NAMES)
def test_the_edges_of_the_tap_rule(name):
    *_, count = pc.edge_case(name)
    want = pc.edge_expected(name)
    assert want["info"][2] == 1 and want["info"][3] == 1              # the pixel is a geometric inlier in every case
    assert want["pinfo"].tolist() == [count, 1 - count], name
    if name == "inside":
        # by hand: the taps 20, 36, 32, 48 at (1.5, 1.5) give Im = 34, e = 3, and w e e = 9
        assert want["sums"][30] == 9.0 and want["sums"][31] == 1.0 and want["prms"] == f32(3.0)
    if name == "difference_at_threshold":
        assert want["sums"][30] == 64.0
    if not count:
        assert not want["sums"][30:].any() and np.isnan(want["prms"])


def test_the_tree_cases_reach_every_form_of_the_combine():
    """track_photo_cases.py restates the joint rule's combine constants as the source has them, every case has the len it
    names, and together they take the forms of the chunk tree: a pair, a tree of four, and leaves of eight under the
    stack."""
    source = open(os.path.join(CSRC, "k_track_photo.h")).read()
    assert f"constexpr int TRKP_CHUNKS = {pc.CHUNKS};" in source and f"constexpr int TRKP_STACK = {pc.STACK};" in source
    assert pc.STACK == 7
    for shape, want in pc.TREE_CASES:
        assert pc.tree_len(shape) == want, (shape, pc.tree_len(shape))
    assert {n for _, n in pc.TREE_CASES} == pc.TREE_LENS == {2, 4, 8, 32}
    assert [tc.track_grid(s, 1)["groups"] for s in pc.TREE_SHAPES] == [94, 257, 20, 33]


@pytest.mark.parametrize("shape", pc.TREE_SHAPES)
def test_the_deep_tree_frames_reach_past_one_partial_per_chunk(shape):
    want = pc.tree_expected(shape)
    assert want["pinfo"][0] > 1000 and np.count_nonzero(want["sums"]) == 33
    grid = tc.track_grid(shape, 1)
    assert grid["groups"] > pc.CHUNKS
    # every group of four tiles holds inliers: no partial is the +0.0 that any order sums right
    assert want["tiles"].shape == (tp.SLOTS, grid["tiles"])
    partials = tc.group_partials(want["tiles"])
    assert partials.shape[1] == grid["groups"] and (partials[29] != 0).all()


def test_the_intensity_rule_is_exact():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (2, 3, 5, 7)).astype(np.uint8)
    got = tp.intensity_planes_ref(img, 3)
    want = (77.0 * img[:, 0] + 150.0 * img[:, 1] + 29.0 * img[:, 2]) / 256.0      # float64
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    white = np.full((1, 3, 1, 1), 255, np.uint8)
    assert tp.intensity_planes_ref(white, 3)[0, 0, 0] == 255.0
    assert np.array_equal(tp.intensity_planes_ref(img[:, :1], 1), img[:, 0].astype(f32))


# ---- the library without a device -----------------------------------------------------------------------------------------------

def test_c_abi_is_declared_and_sized():
    import cuda_depth._native as native
    assert len(native.EXPORTS["smx_track_camera_photometric"][1]) == len(native.EXPORTS["smx_track_camera"][1]) + 6
    assert len(native.EXPORTS["smx_intensity_planes"][1]) == 8
    q, old = native.LIB.smx_track_camera_photometric_workspace_bytes, native.LIB.smx_track_camera_workspace_bytes
    assert q(0, 37, 70) == 0 and q(1, 8192, 8192) == 0 and q(1, 40000, 4) == 0
    for n, H, W in ((1, 1, 1), (2, 37, 70), (3, 1027, 193), (1, 32765, 193)):
        groups = tc.track_grid((H, W), 1)["groups"]
        part = lambda b: -(-b // 256) * 256  # noqa: E731
        assert q(n, H, W) == part(n * 128) + part(n * groups * 34 * 8) > old(n, H, W)
    assert native.LIB.smx_abi_version() == 4


def test_c_entries_reject_bad_arguments_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_track_photo_gpu.py holds the checks there")
    import cuda_depth._native as native
    lib = native.LIB
    img = (C.c_uint8 * 64)()
    out = (C.c_float * 64)()
    a, o = C.addressof(img), C.addressof(out)
    for args, text in (((1, 1, 4, 4, None, o, None), "non-NULL"), ((1, 1, 4, 4, a, None, None), "non-NULL"),
                       ((0, 1, 4, 4, a, o, None), "n >= 1"), ((1, 2, 4, 4, a, o, None), "channels"),
                       ((1, 1, 0, 4, a, o, None), "H"), ((1, 1, 4, 4, a, a, None), "overlap"),
                       ((1, 1, 4, 4, a, o, native.STREAM_ENGINE.value), "caller stream")):
        assert lib.smx_intensity_planes(0, *args) == -1, args
        assert text in native.last_error() and "smx_intensity_planes" in native.last_error(), native.last_error()


def test_python_argument_errors():
    import cuda_depth as cd
    with pytest.raises(RuntimeError, match="photometric_weight"):
        cd.track_camera(None, None, None, None, None, photometric_weight=-1.0)
    with pytest.raises(RuntimeError, match="photometric_weight"):
        cd.track_camera(None, None, None, None, None, photometric_weight=math.nan)
    with pytest.raises(TypeError, match="photometric_weight"):
        cd.track_camera(None, None, None, None, None, photometric_weight="1")
    with pytest.raises(RuntimeError, match="max_intensity_difference"):
        cd.track_camera(None, None, None, None, None, max_intensity_difference=0.0)
    with pytest.raises(RuntimeError, match="needs the frame's image"):
        cd.track_camera(None, None, None, None, None, photometric_weight=0.01)
    with pytest.raises(TypeError, match="torch.Tensor"):
        cd.intensity_planes(np.zeros((1, 3, 4, 4), np.uint8))
    r = cd.TrackingResult(*[None] * 8)
    assert r.photometric_inliers is None and r.photometric_rms is None
