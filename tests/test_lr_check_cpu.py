"""Left-right consistency check, the parts that need no GPU: the five C-ABI symbols, argument checks that return before
the device is touched, the pipeline's new config fields, and known answers of the NumPy twin of the rule
(include/stereo_mi355x.h: smx_compute_lr_*; lr_ref.lr_rule) that the GPU tests compare the kernels against."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lr_ref import lr_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LR_SYMBOLS = ("smx_compute_lr_gray_batch", "smx_compute_lr_gray_u8_batch", "smx_compute_lr_rgb_batch",
              "smx_compute_lr_rgb_u8_batch", "smx_lr_check")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from cuda_depth import _native
    return _native


def test_the_five_symbols_are_declared_listed_and_exported(native):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stereo_mi355x.h")).read(), flags=re.S)
    lib = C.CDLL(native.LIB_PATH)
    for name in LR_SYMBOLS:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in native.EXPORTS, name
        assert hasattr(lib, name), name
    assert native.LIB.smx_abi_version() == 4


@pytest.mark.parametrize("fn", LR_SYMBOLS[:4])
def test_engine_entries_reject_bad_arguments_without_a_device(native, fn):
    f = getattr(native.LIB, fn)
    buf = C.c_void_p(0x1000)                   # never dereferenced: every check returns first
    cases = [
        (None, 1, 1.0, -1.0, "engine is NULL"),
        (None, 0, 1.0, -1.0, "engine is NULL"),
        (None, 1, -0.5, -1.0, "max_diff must be finite and >= 0"),
        (None, 1, float("nan"), -1.0, "max_diff must be finite"),
        (None, 1, float("inf"), -1.0, "max_diff must be finite"),
        (None, 1, 1.0, float("nan"), "invalid_disparity must be finite"),
        (None, 1, 1.0, float("-inf"), "invalid_disparity must be finite"),
    ]
    for engine, n, md, inv, msg in cases:
        assert f(engine, n, buf, buf, buf, None, md, inv, None) == -1, (n, md, inv)
        assert msg in native.last_error(), native.last_error()


def test_standalone_check_rejects_bad_arguments_without_a_device(native):
    f = native.LIB.smx_lr_check
    a, b, c = C.c_void_p(0x1000), C.c_void_p(0x100000), C.c_void_p(0x200000)
    cases = [
        ((0, 0, 4, 4, a, b, c, 1.0, -1.0), "need n >= 1"),
        ((0, 1, 0, 4, a, b, c, 1.0, -1.0), "need n >= 1"),
        ((0, 1, 4, 40000, a, b, c, 1.0, -1.0), "H, W <= 32768"),
        ((0, 1, 4, 4, None, b, c, 1.0, -1.0), "must be non-NULL"),
        ((0, 1, 4, 4, a, b, None, 1.0, -1.0), "must be non-NULL"),
        ((0, 1, 4, 4, a, b, c, -1.0, -1.0), "max_diff must be finite and >= 0"),
        ((0, 1, 4, 4, a, b, c, float("nan"), -1.0), "max_diff must be finite"),
        ((0, 1, 4, 4, a, b, c, 1.0, float("nan")), "invalid_disparity must be finite"),
        ((0, 1, 4, 4, a, b, b, 1.0, -1.0), "must not overlap right_disp"),                       # out == right
        ((0, 1, 4, 4, a, b, C.c_void_p(0x1000 + 8), 1.0, -1.0), "only as the same buffer"),     # out inside left
        ((0, 1, 4, 4, a, b, c, 1.0, -1.0, native.STREAM_ENGINE), "needs a caller stream"),
    ]
    for args, msg in cases:
        if len(args) == 9:
            args = args + (None,)
        assert f(*args) == -1, args
        assert msg in native.last_error(), (msg, native.last_error())


def test_pipeline_config_fields_and_defaults():
    import dataclasses
    from pipeline import DepthEstimationPipelineConfig
    c = DepthEstimationPipelineConfig()
    assert c.left_right_check is False and c.lr_max_diff == 1.0
    names = [f.name for f in dataclasses.fields(c)]
    assert names[:6] == ["image_shape", "min_disparity", "max_disparity", "invalid_disparity",
                         "stereo_matching_backend", "log_perf_time"]
    assert names[6:] == ["left_right_check", "lr_max_diff"]
    assert (c.image_shape, c.min_disparity, c.max_disparity, c.invalid_disparity) == ((384, 1280), 1, 64, -1.0)
    assert c.update(left_right_check=True, lr_max_diff=2.0).left_right_check is True and c.lr_max_diff == 2.0


NAN, INF = float("nan"), float("inf")
# (case, Y, D_L[Y], D_R[Y - t] (None: position not reached), max_diff, valid)
KNOWN = [
    ("t exactly at .5 rounds up", 5, 1.5, 1.5, 1.0, True),           # t = floor(2.0) = 2, yr = 3
    ("just below .5 rounds down", 5, 1.4999999, 1.4999999, 1.0, True),  # t = 1, yr = 4
    ("t == Y", 3, 2.5, 2.5, 1.0, True),                              # t = 3, yr = 0
    ("t > Y", 2, 2.5, None, 1.0, False),                             # t = 3
    ("-0.5 rounds to t = 0", 4, -0.5, -0.5, 1.0, True),
    ("negative t", 4, -0.6, None, 1.0, False),                       # t = floor(-0.1) = -1
    ("NaN D_L", 4, NAN, None, 1.0, False),
    ("+inf D_L", 4, INF, None, 1.0, False),
    ("-inf D_L", 4, -INF, None, 1.0, False),
    ("NaN D_R", 6, 2.0, NAN, 1.0, False),
    ("|diff| == max_diff", 6, 2.25, 1.25, 1.0, True),
    ("|diff| just above max_diff", 6, 2.25, 1.2499999, 1.0, False),
    ("|diff| == max_diff == 0", 6, 2.0, 2.0, 0.0, True),
    ("max_diff 0, tiny diff", 6, 2.0, 2.0000002, 0.0, False),
]


@pytest.mark.parametrize("case", KNOWN, ids=[k[0] for k in KNOWN])
def test_rule_known_answers(case):
    _, Y, dl_v, dr_v, max_diff, valid = case
    W = 8
    dl = np.full((1, W), NAN, np.float32)
    dr = np.full((1, W), 100.0, np.float32)          # far from everything: any other position fails the check
    dl[0, Y] = dl_v
    if dr_v is not None:
        t = int(np.floor(np.float32(dl_v) + np.float32(0.5)))
        dr[0, Y - t] = dr_v
    out = lr_rule(dl, dr, max_diff, invalid_disparity=-3.0)
    expect = np.full((1, W), -3.0, np.float32)
    if valid:
        expect[0, Y] = np.float32(dl_v)
    assert np.array_equal(out, expect), (out, expect)


def test_rule_on_a_consistent_pair_of_constant_maps():
    """A fronto-parallel plane at disparity 3: everything but the 3 left columns points back to itself."""
    dl = np.full((2, 10), 3.0, np.float32)
    out = lr_rule(dl, dl.copy())
    assert np.array_equal(out[:, :3], np.full((2, 3), -1.0, np.float32))
    assert np.array_equal(out[:, 3:], dl[:, 3:])
