"""smx_intensity_pyramid, smx_intensity_pyramid_bytes and smx_track_camera_pyramid without a GPU: declared in
include/stereo_mi355x.h and exported with their signatures; the pyramid entry refuses every bad argument before a device is
touched; the Python layer's new arguments and their errors."""
import ctypes as C
import inspect
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stereo_mi355x.h")
p, i, f, z = C.c_void_p, C.c_int, C.c_float, C.c_size_t
F16, I32 = C.POINTER(C.c_float), C.POINTER(C.c_int32)
SIGNATURES = {
    "smx_intensity_pyramid_bytes": (z, [i, i, i, i], ["n", "H", "W", "levels"]),
    "smx_intensity_pyramid": (i, [i, i, i, i, i, p, p, p, p],
                              ["device_id", "n", "H", "W", "levels", "plane", "mask_depth", "pyramid", "stream"]),
    "smx_track_camera_pyramid": (
        i, [i, i, i, i, p, p, F16, f, f, f, f, i, i, p, p, F16, F16, p, p, p, i, I32, f, i, f, f, f, p, p, i, I32, f, f, f, p,
            p, p, p, p, p, p, z, p],
        ["device_id", "n", "H", "W", "disp", "confidence", "Q[16]", "min_confidence", "z_min", "z_max", "invalid_disparity",
         "Hm", "Wm", "model_depth", "model_normals", "Qm[16]", "Pm[16]", "model_camera_to_world", "model_world_to_camera",
         "pose_in", "schedule_pairs", "schedule", "max_distance", "min_inliers", "min_pivot", "rot_eps", "trans_eps",
         "frame_pyramid", "model_pyramid", "levels", "schedule_levels", "photometric_weight", "max_intensity_difference",
         "huber_delta", "pose_out", "info", "rms", "normal_equations", "photometric_info", "photometric_rms", "workspace",
         "workspace_bytes", "stream"]),
}


@pytest.fixture(scope="module")
def cd():
    import cuda_depth
    return cuda_depth


@pytest.fixture(scope="module")
def native():
    import cuda_depth._native as native
    return native


@pytest.mark.parametrize("name", SIGNATURES)
def test_symbol_is_declared_and_exported(native, name):
    restype, argtypes, names = SIGNATURES[name]
    text = open(HEADER).read()
    ret = "size_t" if restype is z else "int"
    decl = re.search(r"^" + ret + " " + name + r"\((.*?)\);", text, flags=re.S | re.M)
    assert decl, "not declared"
    assert name in text.split("Conventions")[0], "missing from the header's list of entry points"
    assert re.search(r"\bT " + name + r"\b", os.popen(f"nm -D --defined-only {native.LIB_PATH}").read())
    assert native.EXPORTS[name] == (restype, argtypes)
    fn = getattr(native.LIB, name)
    assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert [re.sub(r".*[ *]", "", part.strip()) for part in decl.group(1).split(",")] == names


def test_the_limits_are_stated_anew():
    text = open(HEADER).read()
    assert "no pyramid, no robust weights" not in text
    for word in ("exposure", "the geometric term has no pyramid"):
        assert word in text
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "smx_track_camera_pyramid" in open(os.path.join(ROOT, doc)).read(), doc


def test_the_combine_has_the_joint_rules_shape():
    """k_track_pyramid.h states the combine's chunks and stack again; they are k_track_photo.h's."""
    csrc = os.path.join(ROOT, "stereo-depth_amd", "csrc")
    photo, pyramid = (open(os.path.join(csrc, name)).read() for name in ("k_track_photo.h", "k_track_pyramid.h"))
    for ours, theirs in (("TRKY_CHUNKS", "TRKP_CHUNKS"), ("TRKY_STACK", "TRKP_STACK")):
        a = re.search(r"constexpr int " + ours + r" = (\d+);", pyramid)
        b = re.search(r"constexpr int " + theirs + r" = (\d+);", photo)
        assert a and b and a.group(1) == b.group(1), (ours, theirs)
    assert "TrackJointRule<TrackPyramidArgs, TRKY_CHUNKS, TRKY_STACK>" in pyramid


def test_pyramid_bytes_and_bad_arguments_before_the_device(native):
    import torch
    lib, bad = native.LIB, -1                                         # SMX_ERR_INVALID_ARG
    q = lib.smx_intensity_pyramid_bytes
    assert q(1, 96, 128, 3) == 4 * (96 * 128 + 48 * 64 + 24 * 32) and q(3, 37, 70, 4) == 4 * 3 * (37 * 70 + 19 * 35 + 10 * 18 + 5 * 9)
    assert q(2, 1, 1, 8) == 64 and q(1, 32768, 32768, 8) > 2 ** 32
    assert q(0, 4, 4, 1) == 0 and q(1, 0, 4, 1) == 0 and q(1, 4, 32769, 1) == 0 and q(2, 32768, 32768, 1) == 0
    assert q(1, 4, 4, 0) == 0 and q(1, 4, 4, 9) == 0

    def call(**kw):
        # two planes of 5 x 7 (280 bytes), three levels (408 bytes); invented addresses
        a = dict(dev=0, n=2, H=5, W=7, levels=3, plane=p(0x2000000), mask=p(0x3000000), pyramid=p(0x4000000), stream=None)
        a.update(kw)
        return lib.smx_intensity_pyramid(*a.values())

    if not torch.cuda.is_available():            # a valid call stops at the device; with one it would run on these addresses
        assert call() == -3 and "cannot select HIP device" in native.last_error()
        assert call(mask=None) == -3
        assert call(pyramid=p(0x2000000 + 280), mask=p(0x2000000 + 280 + 408)) == -3      # operands just clear of each other
    for kw, word in ((dict(plane=None), "non-NULL"), (dict(pyramid=None), "non-NULL"), (dict(n=0), "n >= 1"),
                     (dict(H=0), "H"), (dict(W=32769), "W"), (dict(n=2, H=32768, W=32768), "2^30"), (dict(levels=0), "levels"),
                     (dict(levels=9), "levels"), (dict(pyramid=p(0x2000000 + 276)), "overlap"),
                     (dict(pyramid=p(0x2000000 - 404)), "overlap"), (dict(pyramid=p(0x3000000 + 100)), "overlap"),
                     (dict(stream=native.STREAM_ENGINE), "stream")):
        assert call(**kw) == bad and word in native.last_error(), (kw, native.last_error())
        assert "smx_intensity_pyramid" in native.last_error()
    # the order of the rules: the earlier one answers a doubly wrong call
    assert call(plane=None, n=0) == bad and "non-NULL" in native.last_error()
    assert call(n=0, levels=0) == bad and "n >= 1" in native.last_error()
    assert call(levels=0, pyramid=p(0x2000000)) == bad and "levels" in native.last_error()
    assert call(pyramid=p(0x2000000), stream=native.STREAM_ENGINE) == bad and "overlap" in native.last_error()


def test_surface_of_the_python_layer(cd):
    sig = inspect.signature(cd.track_camera)
    kw = {n: prm.default for n, prm in sig.parameters.items() if prm.kind is prm.KEYWORD_ONLY}
    assert kw["pyramid_levels"] is None and kw["huber_delta"] == math.inf and kw["schedule_levels"] is None
    assert list(inspect.signature(cd.intensity_pyramid).parameters) == ["planes", "levels", "mask_depth"]
    for word in ("pyramid_levels", "huber_delta", "schedule_levels", "exposure"):
        assert word in cd.track_camera.__doc__
    sched = cd._check_tracking_schedule(((8, 1), (6, 1), (4, 1), (3, 1), (1, 1)))
    assert cd._check_schedule_levels(sched, 3, None).tolist() == [2, 1, 2, 0, 0]
    assert cd._check_schedule_levels(sched, 1, None).tolist() == [0, 0, 0, 0, 0]
    assert cd._check_schedule_levels(sched, 4, (3, 0, 1, 0, 0)).tolist() == [3, 0, 1, 0, 0]
    for levels, given in ((3, (3, 0, 0, 0, 0)), (3, (0, 2, 0, 0, 0)), (3, (0, 0, 0, 1, 0)), (3, (0, 0, 0, 0)), (3, (-1, 0, 0, 0, 0))):
        with pytest.raises(RuntimeError, match="level"):
            cd._check_schedule_levels(sched, levels, given)
    with pytest.raises(TypeError, match="schedule_levels"):
        cd._check_schedule_levels(sched, 3, (0.5, 0, 0, 0, 0))
    # checked before any tensor is looked at
    for bad, text in ((dict(pyramid_levels=0), "pyramid_levels"), (dict(pyramid_levels=True), "pyramid_levels"),
                      (dict(huber_delta=2.0), "need pyramid_levels"), (dict(schedule_levels=(0,)), "need pyramid_levels"),
                      (dict(pyramid_levels=2, huber_delta=-1.0), "huber_delta")):
        with pytest.raises(RuntimeError, match=text):
            cd.track_camera(None, None, None, None, None, **bad)
    assert cd._pyramid_dims(37, 70, 4) == [(37, 70), (19, 35), (10, 18), (5, 9)]
