"""The windowed copy of a TSDF volume without a GPU: smx_tsdf_window (include/stereo_mi355x.h) is declared and exported
with its signature and refuses every bad argument before a device is touched; the spill boxes of TSDFVolume.shift, the
origins of moved volumes and the shift of TSDFVolume.follow against their independent restatement
(tests/tsdf_window_ref.py); the Python-level errors of the volume's and the pipeline's new arguments."""
import ctypes as C
import dataclasses
import inspect
import math
import os
import re

import numpy as np
import pytest

import tsdf_window_ref as wref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stereo_mi355x.h")
NAME = "smx_tsdf_window"


@pytest.fixture(scope="module")
def cd():
    import cuda_depth
    return cuda_depth


@pytest.fixture(scope="module")
def native():
    import cuda_depth._native as native
    return native


# ---- the C ABI --------------------------------------------------------------------------------------------------------------

def test_symbol_is_declared_and_exported(native):
    text = open(HEADER).read()
    assert re.search(r"\bint " + NAME + r"\(", text)
    assert NAME in text.split("Conventions")[0], "missing from the header's list of entry points"
    assert re.search(r"\bT " + NAME + r"\b", os.popen(f"nm -D --defined-only {native.LIB_PATH}").read())
    restype, argtypes = native.EXPORTS[NAME]
    p, i = C.c_void_p, C.c_int
    assert restype is C.c_int
    assert argtypes == [i, i, i, i, p, p, p, i, i, i, i, i, i, p, p, p, p]
    fn = getattr(native.LIB, NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == argtypes
    # the header's parameter list, in order
    decl = re.search(r"\bint " + NAME + r"\((.*?)\);", text, flags=re.S).group(1)
    names = [re.sub(r".*[ *]", "", part.strip()) for part in decl.split(",")]
    assert names == ["device_id", "nx", "ny", "nz", "tsdf", "weight", "color", "x0", "y0", "z0", "bx", "by", "bz",
                     "tsdf_out", "weight_out", "color_out", "stream"]
    assert native.LIB.smx_abi_version() == 4


def test_bad_arguments_are_refused_before_the_device(native):
    import torch
    lib, bad = native.LIB, -1                                         # SMX_ERR_INVALID_ARG

    def p(addr):
        return C.c_void_p(addr)

    # source 16 x 12 x 10 (7680 bytes per array), window 8 x 6 x 5 (960 bytes per array); invented addresses
    def call(**kw):
        a = dict(dev=0, nx=16, ny=12, nz=10, tsdf=p(0x2000000), weight=p(0x3000000), color=p(0x4000000), x0=-3, y0=2,
                 z0=7, bx=8, by=6, bz=5, tsdf_out=p(0x6000000), weight_out=p(0x7000000), color_out=p(0x8000000),
                 stream=None)
        a.update(kw)
        return lib.smx_tsdf_window(*a.values())

    if not torch.cuda.is_available():            # a valid call stops at the device; with one it would run on these addresses
        assert call() == -3 and "cannot select HIP device" in native.last_error()
        assert call(color=None, color_out=None) == -3
        assert call(x0=8192, y0=-8192, z0=8192) == -3
        assert call(nx=4096, ny=4096, nz=64, tsdf=p(1 << 40), weight=p(2 << 40), color=p(3 << 40)) == -3
        # operands just clear of each other
        assert call(tsdf_out=p(0x2000000 + 7680), weight_out=p(0x2000000 - 960), color_out=p(0x6000000 + 960)) == -3
    broken = dict(
        null=[dict(tsdf=None), dict(weight=None), dict(tsdf_out=None), dict(weight_out=None)],
        colour=[dict(color=None), dict(color_out=None)],
        source_dims=[dict(nx=0), dict(ny=4097), dict(nz=-1), dict(nx=4096, ny=4096, nz=65), dict(nx=1025, ny=1024, nz=1024)],
        window_dims=[dict(bx=0), dict(by=4097), dict(bz=-1), dict(bx=4096, by=4096, bz=65), dict(bx=1024, by=1025, bz=1024)],
        start=[dict(x0=8193), dict(x0=-8193), dict(y0=8193), dict(y0=-8193), dict(z0=8193), dict(z0=-(2 ** 31))],
        overlaps=[dict(tsdf_out=p(0x2000000)), dict(tsdf_out=p(0x2000000 + 7676)), dict(tsdf_out=p(0x3000000 - 956)),
                  dict(weight_out=p(0x4000000 + 100)), dict(color_out=p(0x3000000 + 7679)),
                  dict(weight_out=p(0x6000000 + 956)), dict(color_out=p(0x6000000 - 959)),
                  dict(color_out=p(0x7000000)), dict(tsdf_out=p(0x2000000), tsdf=p(0x2000000))],
        stream=[dict(stream=native.STREAM_ENGINE)])
    for rule, cases in broken.items():
        for kw in cases:
            assert call(**kw) == bad, (rule, kw)
            assert NAME in native.last_error(), (rule, kw, native.last_error())
    for kw, word in ((dict(tsdf=None), "non-NULL"), (dict(color_out=None), "both"), (dict(nx=0), "nx, ny, nz"),
                     (dict(bz=0), "bx, by, bz"), (dict(x0=9000), "x0"), (dict(y0=-9000), "y0"), (dict(z0=9000), "z0"),
                     (dict(tsdf_out=p(0x3000000)), "out of place"), (dict(color_out=p(0x7000000 + 4)), "destination arrays"),
                     (dict(stream=native.STREAM_ENGINE), "stream")):
        assert call(**kw) == bad and word in native.last_error(), (kw, native.last_error())
    # the order of the rules: the earlier one answers a doubly wrong call
    assert call(weight=None, color=None) == bad and "non-NULL" in native.last_error()
    assert call(color=None, nx=0) == bad and "both" in native.last_error()
    assert call(nx=0, bx=0) == bad and "nx, ny, nz" in native.last_error()
    assert call(bx=0, x0=9000) == bad and "bx, by, bz" in native.last_error()
    assert call(z0=9000, tsdf_out=p(0x2000000)) == bad and "z0" in native.last_error()
    assert call(tsdf_out=p(0x2000000), stream=native.STREAM_ENGINE) == bad and "out of place" in native.last_error()


# ---- the host arithmetic ----------------------------------------------------------------------------------------------------

SPILL_SHIFTS = [(0, 0, 2), (-3, 0, 0), (2, -1, 0), (1, 1, -1)]
MARGINS = [0, 1, 2]


@pytest.mark.parametrize("d", SPILL_SHIFTS + [(0, 7, 0), (13, 0, -5), (-40, 3, 0), (12, -6, 4)])
@pytest.mark.parametrize("margin", MARGINS + [9])
@pytest.mark.parametrize("dims", [(13, 7, 5), (24, 16, 20)])
def test_spill_boxes_match_the_twin(cd, dims, margin, d):
    got = cd.tsdf_spill_boxes(dims, d, margin)
    expect = wref.spill_boxes_ref(dims, d, margin)
    assert got == expect
    assert len(got) == sum(c != 0 for c in d)
    vs, origin, offset = 0.1, (-1.3, 0.7, 2.05), (5, -9, 1000)
    for start, size in got:
        assert all(0 <= s and s + n <= m and n >= 1 for s, n, m in zip(start, size, dims))
        moved = tuple(a + b for a, b in zip(offset, start))
        assert cd.tsdf_window_origin(origin, moved, vs) == wref.origin_ref(origin, moved, vs)


def test_spill_box_arguments(cd):
    assert cd.tsdf_spill_boxes((8, 8, 8), (0, 0, 0), 1) == []
    assert cd.tsdf_spill_boxes((8, 8, 8), (3, 0, 0), 0) == [((0, 0, 0), (3, 8, 8))]
    assert cd.tsdf_spill_boxes((8, 8, 8), (0, -3, 0), 1) == [((0, 4, 0), (8, 4, 8))]
    with pytest.raises(RuntimeError, match="margin"):
        cd.tsdf_spill_boxes((8, 8, 8), (1, 0, 0), -1)
    with pytest.raises(TypeError):
        cd.tsdf_spill_boxes((8, 8, 8), (1.0, 0, 0), 1)
    with pytest.raises(TypeError):
        cd.tsdf_spill_boxes((8, 8, 8), (1, 0), 1)


def test_origin_does_not_drift(cd):
    """The origin after many shifts is ONE product and sum from the constructor's origin, not a running sum."""
    vs, origin = 0.1, (0.3, -7.7, 1e-3)
    offset, running = [0, 0, 0], list(origin)
    for k in range(1000):
        step = (3, -1, 7 * (k % 2))
        offset = [a + b for a, b in zip(offset, step)]
        running = [r + s * vs for r, s in zip(running, step)]
    got = cd.tsdf_window_origin(origin, offset, vs)
    assert got == wref.origin_ref(origin, offset, vs) == tuple(o + k * vs for o, k in zip(origin, offset))
    assert got != tuple(running), "the test's path does not tell a running sum from the product"
    assert cd.tsdf_window_origin(origin, (0, 0, 0), vs) == origin
    assert all(type(v) is float for v in got)


FOLLOW_CASES = [
    # (position, origin, dims, voxel_size, anchor)
    ((2.4, 1.6, 2.4), (0.0, 0.0, 0.0), (48, 32, 48), 0.1, (0.5, 0.5, 0.5)),          # at the anchor
    ((3.0625, 2.0, 3.0), (0.0, 0.0, 0.0), (48, 32, 48), 0.125, (0.5, 0.5, 0.5)),     # exactly half a voxel: away from 0
    ((2.9375, 2.0, 2.8125), (0.0, 0.0, 0.0), (48, 32, 48), 0.125, (0.5, 0.5, 0.5)),  # -0.5 and -1.5
    ((3.1875, 2.1875, 3.4375), (0.0, 0.0, 0.0), (48, 32, 48), 0.125, (0.5, 0.5, 0.5)),   # 1.5, 1.5, 3.5
    ((-17.3, -0.04, -250.0), (-4.0, -2.0, -1.0), (40, 24, 56), 0.05, (0.5, 0.5, 0.25)),  # negative positions
    ((0.3, 0.2999999999999999, 0.30000000000000004), (0.0, 0.0, 0.0), (4, 4, 4), 0.2, (0.0, 0.0, 0.0)),
    ((1.0, 2.0, 3.0), (0.1, 0.2, 0.3), (37, 29, 41), 0.07, (1.0, 0.0, 0.3)),
    ((0.049999999999999996, 0.05, 0.15000000000000002), (0.0, 0.0, 0.0), (2, 2, 2), 0.1, (0.0, 0.0, 0.0)),
]


@pytest.mark.parametrize("case", FOLLOW_CASES)
def test_follow_shift_matches_the_twin(cd, case):
    position, origin, dims, vs, anchor = case
    got = cd.tsdf_follow_shift(position, origin, dims, vs, anchor)
    assert got == wref.follow_shift_ref(position, origin, dims, vs, anchor)
    assert all(type(c) is int for c in got)


def test_follow_rounds_halves_away_from_zero(cd):
    dims, vs = (48, 32, 48), 0.125                                    # anchor point (3, 2, 3): exact in binary
    for frac, expect in ((0.5, 1), (-0.5, -1), (1.5, 2), (-1.5, -2), (2.5, 3), (-2.5, -3), (0.4375, 0), (-0.4375, 0),
                         (0.0, 0), (7.5, 8), (-100.5, -101)):
        position = (3.0 + frac * vs, 2.0 - frac * vs, 3.0)
        assert cd.tsdf_follow_shift(position, (0.0, 0.0, 0.0), dims, vs) == (expect, -expect, 0), frac
    assert wref.round_half_away(0.49999999999999994) == 0 and wref.round_half_away(-0.5) == -1
    assert cd.tsdf_follow_shift((0.49999999999999994, 0.0, 0.0), (0.0, 0.0, 0.0), (1, 1, 1), 1.0, (0, 0, 0)) == (0, 0, 0)
    with pytest.raises(RuntimeError, match="finite"):
        cd.tsdf_follow_shift((math.nan, 0.0, 0.0), (0.0, 0.0, 0.0), dims, vs)


class _HostVolume:
    """TSDFVolume's host side alone: follow's arithmetic and thresholds without device state (shift records its calls)."""

    def __new__(cls, cd, dims, vs, origin):
        vol = object.__new__(type("HostVolume", (cd.TSDFVolume,), {"shift": cls.shift}))
        vol.dims, vol.voxel_size, vol.origin = dims, vs, origin
        vol.calls = []
        return vol

    def shift(self, voxels, *, spill=False, margin=1):
        self.calls.append((voxels, spill, margin))
        self._offset = tuple(a + b for a, b in zip(self._offset, voxels))
        return ["box"] * sum(c != 0 for c in voxels) if spill else []


def pose_at(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def test_follow_thresholds_and_batches(cd):
    dims, vs, origin = (48, 32, 48), 0.125, (0.0, 0.0, 0.0)           # default threshold min(dims) // 8 = 4
    vol = _HostVolume(cd, dims, vs, origin)
    for pos, threshold in (((3.0 + 3 * vs, 2.0, 3.0), None), ((3.0, 2.0 - 3.4 * vs, 3.0), None),
                           ((3.0, 2.0, 3.0 + 4.4 * vs), 5), ((3.0, 2.0, 3.0), 1)):
        assert vol.follow(pose_at(*pos), threshold=threshold) == ((0, 0, 0), []), pos
        assert wref.follow_ref(pos, origin, dims, vs, threshold) == (0, 0, 0)
    assert vol.calls == [] and vol.offset == (0, 0, 0)
    # the threshold's edge: |d| == threshold shifts
    pos = (3.0 + 4 * vs, 2.0 - 1 * vs, 3.0)
    assert wref.follow_ref(pos, origin, dims, vs) == (4, -1, 0)
    assert vol.follow(pose_at(*pos)) == ((4, -1, 0), [])
    assert vol.calls == [((4, -1, 0), False, 1)] and vol.offset == (4, -1, 0)
    assert vol.origin == (0.5, -0.125, 0.0)
    assert vol.follow(pose_at(*pos)) == ((0, 0, 0), [])               # the camera is at the anchor now
    # spill and margin are handed on; with threshold=1 half a voxel is enough
    pos2 = (pos[0], pos[1], 3.0 - 4 * vs)
    assert vol.follow(pose_at(*pos2), spill=True, margin=2) == ((0, 0, -4), ["box"])
    assert vol.calls[-1] == ((0, 0, -4), True, 2)
    assert vol.follow(pose_at(pos2[0] + 0.5 * vs, pos2[1], pos2[2]), threshold=1)[0] == (1, 0, 0)
    # a batch: the last pose counts; tensors are accepted
    import torch
    batch = np.stack([pose_at(100.0, 0.0, 0.0), pose_at(*pos2)])
    assert vol.follow(batch, threshold=1)[0] == (-1, 0, 0)
    assert vol.follow(torch.from_numpy(batch), threshold=1) == ((0, 0, 0), [])
    assert vol.offset == (4, -1, -4)
    # anchor: the point that follows the camera
    vol2 = _HostVolume(cd, dims, vs, origin)
    assert vol2.follow(pose_at(3.0, 2.0, 3.0), anchor=(0.5, 0.5, 0.25))[0] == (0, 0, 12)
    assert wref.follow_ref((3.0, 2.0, 3.0), origin, dims, vs, None, (0.5, 0.5, 0.25)) == (0, 0, 12)
    # a small volume's default threshold is at least 1
    vol3 = _HostVolume(cd, (5, 4, 6), 1.0, origin)
    assert vol3.follow(pose_at(3.5, 2.0, 3.0))[0] == (1, 0, 0)


def test_follow_argument_errors(cd):
    vol = _HostVolume(cd, (48, 32, 48), 0.125, (0.0, 0.0, 0.0))
    eye = np.eye(4)
    for exc, match, kw in ((TypeError, "threshold", dict(threshold=2.0)), (TypeError, "threshold", dict(threshold=True)),
                           (RuntimeError, "threshold", dict(threshold=0)), (TypeError, "anchor", dict(anchor=0.5)),
                           (TypeError, "anchor", dict(anchor=(0.5, 0.5))), (TypeError, "anchor", dict(anchor=("a", 0, 0))),
                           (RuntimeError, "anchor", dict(anchor=(math.nan, 0.5, 0.5)))):
        with pytest.raises(exc, match=match):
            vol.follow(eye, **kw)
    with pytest.raises(RuntimeError, match="camera_to_world"):
        vol.follow(np.eye(3))
    with pytest.raises(RuntimeError, match="finite"):
        vol.follow(pose_at(math.inf, 0.0, 0.0))
    assert vol.calls == []


def test_shift_and_window_argument_errors(cd):
    """Checked before any state or device is touched."""
    vol = object.__new__(cd.TSDFVolume)
    vol.dims, vol.voxel_size, vol.origin = (16, 12, 10), 0.1, (0.0, 0.0, 0.0)
    for bad in ((1, 2), 3, (1.0, 0, 0), (True, 0, 0), "abc"):
        with pytest.raises(TypeError, match="voxels"):
            vol.shift(bad)
        with pytest.raises(TypeError, match="start"):
            vol.window(bad, (4, 4, 4))
    with pytest.raises(RuntimeError, match="8192"):
        vol.shift((0, 8193, 0))
    with pytest.raises(RuntimeError, match="8192"):
        vol.window((0, 0, -8193), (4, 4, 4))
    with pytest.raises(TypeError, match="spill"):
        vol.shift((1, 0, 0), spill=1)
    with pytest.raises(RuntimeError, match="margin"):
        vol.shift((1, 0, 0), spill=True, margin=-1)
    with pytest.raises(TypeError, match="margin"):
        vol.shift((1, 0, 0), spill=True, margin=1.5)
    with pytest.raises(RuntimeError, match="4096"):
        vol.window((0, 0, 0), (4097, 1, 1))
    with pytest.raises(TypeError, match="dims"):
        vol.window((0, 0, 0), 7)
    assert vol.shift((0, 0, 0)) == [] and vol.shift((0, 0, 0), spill=True) == []      # no state was needed
    assert vol.offset == (0, 0, 0) and vol.origin == (0.0, 0.0, 0.0)
    vol.release_spare()


def test_surface_of_the_new_methods(cd):
    sig = inspect.signature(cd.TSDFVolume.shift)
    assert [(n, p.default) for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY] == [("spill", False),
                                                                                                 ("margin", 1)]
    sig = inspect.signature(cd.TSDFVolume.follow)
    kw = {n: p.default for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY}
    assert kw == dict(threshold=None, anchor=(0.5, 0.5, 0.5), spill=False, margin=1)
    assert list(inspect.signature(cd.TSDFVolume.window).parameters) == ["self", "start", "dims"]
    assert isinstance(cd.TSDFVolume.offset, property) and isinstance(cd.TSDFVolume.origin, property)
    for word in ("twice", "release_spare", "different tensors"):
        assert word in cd.TSDFVolume.shift.__doc__
    for word in ("margin layer", "corner", "voxel_downsample"):
        assert word in cd.TSDFVolume.shift.__doc__


# ---- the pipeline's keywords ----------------------------------------------------------------------------------------------

def test_pipeline_keywords_and_result_fields():
    import pipeline
    sig = inspect.signature(pipeline.DepthEstimationPipeline.__init__)
    got = {n: sig.parameters[n].default for n in ("follow_camera", "follow_threshold", "follow_anchor", "keep_spill")}
    assert got == dict(follow_camera=False, follow_threshold=None, follow_anchor=(0.5, 0.5, 0.5), keep_spill=False)
    fields = {f.name: f for f in dataclasses.fields(pipeline.DepthEstimationResult)}
    assert fields["volume_shift"].kw_only and fields["volume_shift"].default == (0, 0, 0)
    assert fields["spilled_volumes"].kw_only and fields["spilled_volumes"].default_factory is list
    assert list(fields)[-1] == "confidence_map" and list(fields)[:3] == ["left_image", "right_image", "disparity_map"]
    cfg = pipeline.DepthEstimationPipelineConfig(image_shape=(32, 48), min_disparity=0, max_disparity=15)
    for exc, kw in ((ValueError, dict(follow_camera=True)), (TypeError, dict(follow_camera=1)),
                    (ValueError, dict(keep_spill=True)), (ValueError, dict(follow_threshold=3)),
                    (ValueError, dict(follow_anchor=(0.5, 0.5, 0.25)))):
        with pytest.raises(exc, match="follow_camera|tsdf_volume"):
            pipeline.DepthEstimationPipeline(cfg, **kw)
