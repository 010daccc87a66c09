"""Speckle filter and hole fill, the parts that need no GPU: the three C-ABI symbols, argument checks that return before
the device is touched, the new keyword arguments of the backend and the pipeline, and known answers of the CPU
reference (tests/postprocess_ref.py) that the GPU tests compare the kernels against."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import postprocess_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("smx_postprocess_workspace_bytes", "smx_filter_speckles", "smx_fill_invalid")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from cuda_depth import _native
    return _native


def test_the_three_symbols_are_declared_listed_and_exported(native):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stereo_mi355x.h")).read(), flags=re.S)
    lib = C.CDLL(native.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\b(int|size_t)\s+{name}\s*\(", header), name
        assert name in native.EXPORTS, name
        assert hasattr(lib, name), name
    assert native.LIB.smx_abi_version() == 4


def test_workspace_query(native):
    q = native.LIB.smx_postprocess_workspace_bytes
    assert q(1, 375, 1242) >= 2 * 4 * 375 * 1242 + 4 * 375
    assert q(32, 375, 1242) >= 32 * q(1, 375, 1242) - 32 * 3 * 256
    for n, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 32769, 4), (1, 4, 32769)):
        assert q(n, H, W) == 0, (n, H, W)


# fake device pointers: never dereferenced, every check returns first
IN, OUT, WS = 0x100000, 0x200000, 0x300000
WS_BYTES = 1 << 20


def _speckle_cases(native):
    S = native.STREAM_ENGINE
    good = dict(dev=0, n=1, H=4, W=4, i=IN, o=OUT, size=2, md=1.0, inv=-1.0, ws=WS, wsb=WS_BYTES, s=None)
    cases = [
        (dict(i=None), "must be non-NULL"),
        (dict(o=None), "must be non-NULL"),
        (dict(ws=None), "must be non-NULL"),
        (dict(n=0), "need n >= 1"),
        (dict(H=0), "1 <= H, W <= 32768"),
        (dict(W=0), "1 <= H, W <= 32768"),
        (dict(H=32769), "1 <= H, W <= 32768"),
        (dict(W=32769), "1 <= H, W <= 32768"),
        (dict(size=-1), "max_speckle_size must be >= 0"),
        (dict(md=-0.5), "max_diff must be finite and >= 0"),
        (dict(md=NAN), "max_diff must be finite"),
        (dict(md=INF), "max_diff must be finite"),
        (dict(inv=NAN), "invalid_disparity must be finite"),
        (dict(inv=-INF), "invalid_disparity must be finite"),
        (dict(wsb=native.LIB.smx_postprocess_workspace_bytes(1, 4, 4) - 1), "below smx_postprocess_workspace_bytes"),
        (dict(o=IN + 8), "other than as the same buffer"),
        (dict(ws=IN + 16), "workspace must not overlap"),
        (dict(ws=OUT - 16), "workspace must not overlap"),
        (dict(ws=WS + 4), "workspace must be 256-byte aligned"),
        (dict(ws=WS + 128, s=S), "workspace must be 256-byte aligned"),
        (dict(s=S), "needs a caller stream"),
    ]
    return good, cases


def test_filter_speckles_rejects_bad_arguments_without_a_device(native):
    good, cases = _speckle_cases(native)
    for change, msg in cases:
        a = {**good, **change}
        rc = native.LIB.smx_filter_speckles(a["dev"], a["n"], a["H"], a["W"], a["i"], a["o"], a["size"], a["md"],
                                            a["inv"], a["ws"], a["wsb"], a["s"])
        assert rc == -1, change
        assert msg in native.last_error(), (msg, native.last_error())


def test_fill_invalid_rejects_bad_arguments_without_a_device(native):
    good, cases = _speckle_cases(native)
    for change, msg in cases:
        if "size" in change or "md" in change:
            continue                                     # no such argument
        a = {**good, **change}
        rc = native.LIB.smx_fill_invalid(a["dev"], a["n"], a["H"], a["W"], a["i"], a["o"], a["inv"], a["ws"], a["wsb"],
                                         a["s"])
        assert rc == -1, change
        assert msg in native.last_error(), (msg, native.last_error())


def test_python_entries_reject_bad_scalars_before_the_device():
    import cuda_depth
    t = object()                                          # never reached: the scalars are checked first
    with pytest.raises(RuntimeError, match="max_speckle_size must be in"):
        cuda_depth.filter_speckles(t, max_speckle_size=-1)
    with pytest.raises(TypeError, match="max_speckle_size must be an int"):
        cuda_depth.filter_speckles(t, max_speckle_size=2.0)
    with pytest.raises(RuntimeError, match="max_diff must be finite and >= 0"):
        cuda_depth.filter_speckles(t, max_speckle_size=4, max_diff=-1.0)
    with pytest.raises(RuntimeError, match="invalid_disparity must be finite"):
        cuda_depth.filter_speckles(t, max_speckle_size=4, invalid_disparity=NAN)
    with pytest.raises(RuntimeError, match="invalid_disparity must be finite"):
        cuda_depth.fill_invalid(t, invalid_disparity=INF)


def test_backend_and_pipeline_keywords_and_defaults():
    from pipeline import DepthEstimationPipeline
    from pipeline.depth import CudaStereoMatchingBackend
    for cls in (CudaStereoMatchingBackend, DepthEstimationPipeline):
        p = inspect.signature(cls.__init__).parameters
        for name, default in (("speckle_max_size", 0), ("speckle_max_diff", 1.0), ("fill_invalid", False)):
            assert name in p, (cls, name)
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY, (cls, name)
            assert p[name].default == default and type(p[name].default) is type(default), (cls, name)


# ----------------------------------------------------------------------------- known answers of the reference
def _f(a):
    return np.array(a, np.float32)


def test_two_by_two_blob_at_limits_3_and_4():
    d = np.full((4, 4), -1.0, np.float32)
    d[1:3, 1:3] = 5.0
    assert np.array_equal(ref.filter_speckles(d, 3), d)                 # size 4 > 3: kept
    assert np.array_equal(ref.filter_speckles(d, 4), np.full((4, 4), -1.0, np.float32))   # size 4 <= 4: removed


def test_chain_is_one_region_by_transitivity():
    d = _f([[0.0, 0.9, 1.8, 2.7]])
    assert ref.region_sizes(d, 1.0, -1.0).tolist() == [[4, 4, 4, 4]]
    assert np.array_equal(ref.filter_speckles(d, 3), d)
    assert np.array_equal(ref.filter_speckles(d, 4), np.full((1, 4), -1.0, np.float32))
    assert ref.region_sizes(d, 0.85, -1.0).tolist() == [[1, 1, 1, 1]]


def test_diagonal_neighbours_are_not_linked():
    d = _f([[1.0, -1.0], [-1.0, 1.0]])
    assert ref.region_sizes(d, 1.0, -1.0).tolist() == [[1, 0], [0, 1]]
    assert np.array_equal(ref.filter_speckles(d, 1), np.full((2, 2), -1.0, np.float32))


@pytest.mark.parametrize("sep", [NAN, INF, -INF, -1.0])
def test_specials_split_regions(sep):
    d = _f([[2.0, 2.0, sep, 2.0, 2.0, 2.0]])
    assert ref.region_sizes(d, 1.0, -1.0).tolist() == [[2, 2, 0, 3, 3, 3]]
    out = ref.filter_speckles(d, 2)
    expect = _f([[-1.0, -1.0, sep, 2.0, 2.0, 2.0]])
    assert np.array_equal(out.view(np.uint32), expect.view(np.uint32))   # the separator is copied bit for bit


def test_nan_payload_and_negative_zero_marker():
    payload = np.array([0x7FC01234], np.uint32).view(np.float32)[0]
    d = _f([[payload, -0.0, 3.0, 3.0]])
    out = ref.filter_speckles(d, 5, 1.0, invalid_disparity=0.0)          # -0.0 == 0.0: not valid
    assert out.view(np.uint32).tolist() == [[0x7FC01234, np.float32(-0.0).view(np.uint32), 0, 0]]


def test_max_speckle_size_zero_is_a_copy():
    d = _f([[1.0, 5.0], [NAN, 9.0]])
    assert np.array_equal(ref.filter_speckles(d, 0).view(np.uint32), d.view(np.uint32))


def test_float32_link_test():
    # 1.0f - (-1e-9f) is 1.000000001 exactly but rounds to 1.0f in float32: linked (float64 would say not)
    d = _f([[-1e-9, 1.0]])
    assert float(d[0, 1]) - float(d[0, 0]) > 1.0
    assert ref.region_sizes(d, 1.0, -1.0).tolist() == [[2, 2]]
    d = _f([[-1e-7, 1.0]])                                # 1.0000001 rounds to 1.00000012f: not linked
    assert ref.region_sizes(d, 1.0, -1.0).tolist() == [[1, 1]]


def test_maps_are_independent():
    d = np.full((2, 2, 3), 4.0, np.float32)
    assert ref.region_sizes(d[0], 1.0, -1.0).max() == 6
    out = ref.filter_speckles(d, 6)                      # 6 per map, not 12
    assert np.all(out == -1.0)


def test_fill_row_rule_ties_and_borders():
    d = _f([[-1.0, 3.0, -1.0, -1.0, 2.0, -1.0]])
    assert ref.fill_invalid(d).tolist() == [[3.0, 3.0, 2.0, 2.0, 2.0, 2.0]]
    d = _f([[-0.0, -1.0, 0.0]])                           # tie: the left value wins
    assert ref.fill_invalid(d).view(np.uint32)[0, 1] == np.float32(-0.0).view(np.uint32)
    d = _f([[0.0, -1.0, -0.0]])
    assert ref.fill_invalid(d).view(np.uint32)[0, 1] == 0
    d = _f([[NAN, 4.0, INF]])
    assert ref.fill_invalid(d).tolist() == [[4.0, 4.0, 4.0]]


def test_fill_empty_rows():
    d = np.full((5, 3), -1.0, np.float32)
    d[1] = [5.0, 1.0, 7.0]
    d[3] = [2.0, 2.0, 9.0]
    out = ref.fill_invalid(d)
    assert out[0].tolist() == [5.0, 1.0, 7.0]             # empty first row: copies the row below
    assert out[2].tolist() == [2.0, 1.0, 7.0]             # empty middle row: min of the rows above and below
    assert out[4].tolist() == [2.0, 2.0, 9.0]             # empty last row: copies the row above
    d = _f([[-1.0, -1.0], [-0.0, -0.0], [-1.0, -1.0], [0.0, 0.0]])
    out = ref.fill_invalid(d)
    assert out.view(np.uint32)[2].tolist() == [np.float32(-0.0).view(np.uint32)] * 2   # the row above wins ties


def test_fill_middle_row_from_row_pass_result():
    d = _f([[-1.0, 6.0, -1.0], [-1.0, -1.0, -1.0], [8.0, -1.0, 1.0]])
    out = ref.fill_invalid(d)
    assert out.tolist() == [[6.0, 6.0, 6.0], [6.0, 1.0, 1.0], [8.0, 1.0, 1.0]]


def test_fill_all_invalid_map_is_copied():
    d = _f([[NAN, -1.0], [INF, -1.0]])
    out = ref.fill_invalid(d)
    assert np.array_equal(out.view(np.uint32), d.view(np.uint32))
