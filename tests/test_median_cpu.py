"""Weighted median, the parts that need no GPU: the two C-ABI symbols, argument checks that return before the device is
touched, the weight-table formula, the new keyword arguments of the backend and the pipeline, and hand-computed answers
of the CPU reference (tests/median_ref.py) that the GPU tests compare the kernel against."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import median_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("smx_median_workspace_bytes", "smx_weighted_median")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from cuda_depth import _native
    return _native


def test_the_two_symbols_are_declared_listed_and_exported(native):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stereo_mi355x.h")).read(), flags=re.S)
    lib = C.CDLL(native.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\b(int|size_t)\s+{name}\s*\(", header), name
        assert name in native.EXPORTS, name
        assert hasattr(lib, name), name
    assert native.LIB.smx_abi_version() == 4


def test_workspace_query(native):
    q = native.LIB.smx_median_workspace_bytes
    assert q(32, 375, 1242) >= 0
    for n, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 32769, 4), (1, 4, 32769), (-1, 4, 4)):
        assert q(n, H, W) == 0, (n, H, W)


# fake device pointers: never dereferenced, every check returns first
IN, HOLES, GUIDE, OUT, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
MAP_BYTES = 2 * 4 * 4 * 4                                # n = 2, H = W = 4


def _tables(radius=2, top=1023):
    return np.full(256, top, np.uint16), np.full((radius + 1) ** 2, top, np.uint16)


def _call(native, **change):
    rw, sw = _tables(change.pop("radius_tables", 2))
    a = dict(dev=0, n=2, H=4, W=4, i=IN, h=HOLES, g=GUIDE, o=OUT, r=2, rw=rw, sw=sw, inv=-1.0, ws=None, wsb=0, s=None)
    a.update(change)
    rwp = None if a["rw"] is None else a["rw"].ctypes.data
    swp = None if a["sw"] is None else a["sw"].ctypes.data
    return native.LIB.smx_weighted_median(a["dev"], a["n"], a["H"], a["W"], a["i"], a["h"], a["g"], a["o"], a["r"], rwp,
                                          swp, a["inv"], a["ws"], a["wsb"], a["s"])


def test_weighted_median_rejects_bad_arguments_without_a_device(native):
    big_rw, big_sw = _tables(2)
    big_rw[200] = 1024
    big_sw[8] = 1024
    cases = [
        (dict(i=None), "in, guide and out must be non-NULL"),
        (dict(g=None), "in, guide and out must be non-NULL"),
        (dict(o=None), "in, guide and out must be non-NULL"),
        (dict(rw=None), "range_weight and spatial_weight must be non-NULL"),
        (dict(sw=None), "range_weight and spatial_weight must be non-NULL"),
        (dict(n=0), "need n >= 1"),
        (dict(H=0), "1 <= H, W <= 32768"),
        (dict(W=0), "1 <= H, W <= 32768"),
        (dict(H=32769), "1 <= H, W <= 32768"),
        (dict(W=32769), "1 <= H, W <= 32768"),
        (dict(r=0, radius_tables=0), "radius must be in 1..15"),
        (dict(r=16, radius_tables=16), "radius must be in 1..15"),
        (dict(r=-1, radius_tables=1), "radius must be in 1..15"),
        (dict(rw=big_rw), "range_weight[200] = 1024 is above 1023"),
        (dict(sw=big_sw), "spatial_weight[8] = 1024 is above 1023"),
        (dict(inv=NAN), "invalid_disparity must be finite"),
        (dict(inv=INF), "invalid_disparity must be finite"),
        (dict(ws=None, wsb=64), "workspace is NULL"),
        (dict(o=IN), "out must not overlap in or guide"),
        (dict(o=IN + MAP_BYTES - 4), "out must not overlap in or guide"),
        (dict(o=GUIDE + 4), "out must not overlap in or guide"),
        (dict(o=GUIDE - MAP_BYTES + 4), "out must not overlap in or guide"),
        (dict(o=HOLES + 4), "out must not overlap holes other than as the same buffer"),
        (dict(ws=IN + 16, wsb=64), "the workspace must not overlap"),
        (dict(ws=HOLES + 16, wsb=64), "the workspace must not overlap"),
        (dict(ws=GUIDE + 16, wsb=64), "the workspace must not overlap"),
        (dict(ws=OUT - 16, wsb=64), "the workspace must not overlap"),
        (dict(ws=WS + 8, wsb=64), "workspace must be 256-byte aligned"),
        (dict(ws=WS + 128, wsb=0), "workspace must be 256-byte aligned"),
        (dict(s=native.STREAM_ENGINE), "needs a caller stream"),
    ]
    for change, msg in cases:
        rc = _call(native, **dict(change))
        assert rc == -1, change
        assert msg in native.last_error(), (change, msg, native.last_error())


def test_spatial_table_is_read_only_up_to_its_size(native):
    # radius 1 reads 4 spatial entries: a 1024 right behind them is not part of the table
    rw, sw = _tables(1)
    longer = np.concatenate([sw, np.array([1024], np.uint16)])
    rc = _call(native, r=1, sw=longer, s=native.STREAM_ENGINE)
    assert rc == -1 and "needs a caller stream" in native.last_error()


def test_python_entries_reject_bad_scalars_before_the_device():
    import cuda_depth
    t = object()                                          # never reached: the scalars are checked first
    with pytest.raises(RuntimeError, match="radius must be in 1..15"):
        cuda_depth.weighted_median(t, t, radius=0, sigma_color=10.0, sigma_space=5.0)
    with pytest.raises(RuntimeError, match="radius must be in 1..15"):
        cuda_depth.weighted_median(t, t, radius=16, sigma_color=10.0, sigma_space=5.0)
    with pytest.raises(TypeError, match="radius must be an int"):
        cuda_depth.weighted_median(t, t, radius=3.0, sigma_color=10.0, sigma_space=5.0)
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(RuntimeError, match="sigma_color must be finite and > 0"):
            cuda_depth.weighted_median(t, t, radius=3, sigma_color=bad, sigma_space=5.0)
        with pytest.raises(RuntimeError, match="sigma_space must be finite and > 0"):
            cuda_depth.median_weight_tables(3, 10.0, bad)
    with pytest.raises(RuntimeError, match="invalid_disparity must be finite"):
        cuda_depth.weighted_median(t, t, radius=3, sigma_color=10.0, sigma_space=5.0, invalid_disparity=NAN)


def test_weight_table_formula():
    import cuda_depth
    rw, sw = cuda_depth.median_weight_tables(1, 10.0, 5.0)
    assert rw.dtype == np.uint16 and rw.shape == (256,) and sw.dtype == np.uint16 and sw.shape == (4,)
    assert [int(rw[k]) for k in (0, 1, 10, 20, 40, 255)] == [1023, 1018, 620, 138, 0, 0]
    assert sw.tolist() == [1023, 1003, 1003, 983]                  # [|dy| * 2 + |dx|]
    assert np.all(np.diff(rw.astype(int)) <= 0)
    rw, sw = cuda_depth.median_weight_tables(15, 10.0, 5.0)
    assert sw.shape == (256,) and sw[0] == 1023 and sw[255] == 0   # exp(-9) * 1023 = 0.13
    assert sw[1] == sw[16] == 1003                                 # symmetric in dx and dy
    rw, _ = cuda_depth.median_weight_tables(2, 1e6, 1e6)
    assert np.all(rw == 1023)


def test_backend_and_pipeline_keywords_and_defaults():
    from pipeline import DepthEstimationPipeline
    from pipeline.depth import CudaStereoMatchingBackend
    for cls in (CudaStereoMatchingBackend, DepthEstimationPipeline):
        p = inspect.signature(cls.__init__).parameters
        for name, default in (("median_radius", 0), ("median_sigma_color", 10.0), ("median_sigma_space", 5.0)):
            assert name in p, (cls, name)
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY, (cls, name)
            assert p[name].default == default and type(p[name].default) is type(default), (cls, name)


# ----------------------------------------------------------------------------- known answers of the reference
def _f(a):
    return np.array(a, np.float32)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


ONES1 = (np.ones(256, np.uint16), np.ones(4, np.uint16))           # radius 1, every weight 1


def _both(d, g, radius, rw, sw, holes=None, inv=-1.0):
    """The vectorised reference, checked pixel by pixel against the plain one."""
    out = ref.weighted_median(d, g, radius, rw, sw, holes=holes, invalid_disparity=inv)
    for x in range(d.shape[0]):
        for y in range(d.shape[1]):
            e = ref.weighted_median_pixel(d, g, x, y, radius, rw, sw, holes=holes, invalid_disparity=inv)
            assert _bits(e) == _bits(out[x, y]), (x, y)
    return out


def test_key_order():
    vals = _f([-INF, -2.0, -1e-30, -0.0, 0.0, 1e-30, 3.0, INF])
    assert np.all(np.diff(ref.key(vals).astype(np.int64)) > 0)


def test_tie_at_exactly_half_takes_the_lower_value():
    d = _f([[1.0, 2.0, -1.0]])
    g = np.zeros_like(d)
    out = _both(d, g, 1, *ONES1)
    assert out.tolist() == [[1.0, 1.0, -1.0]]             # T = 2 and 2 * 1 >= 2 at the key of 1.0; -1.0 is not in F
    sw = np.array([2, 1, 1, 1], np.uint16)                # the centre weighs 2: (0, 1) has 1.0 (1) and 2.0 (2)
    assert _both(d, g, 1, ONES1[0], sw).tolist() == [[1.0, 2.0, -1.0]]


def test_negative_zero_sorts_below_positive_zero():
    d = _f([[-0.0, 0.0]])
    g = np.zeros_like(d)
    out = _both(d, g, 1, *ONES1)
    assert _bits(out).tolist() == [[0x80000000, 0x80000000]]        # tie: the smaller key, -0.0
    sw = np.array([3, 1, 1, 1], np.uint16)                # each centre outweighs the other sample
    assert _bits(_both(d, g, 1, ONES1[0], sw)).tolist() == [[0x80000000, 0]]


def test_zero_total_weight_copies_the_pixel():
    payload = np.array([0x7FC01234], np.uint32).view(np.float32)[0]
    d = _f([[3.0, 5.0], [7.0, payload]])
    g = _f([[0.0, 100.0], [200.0, 50.0]])
    rw = np.zeros(256, np.uint16)                         # no range weight at all: T = 0 everywhere
    out = _both(d, g, 1, rw, ONES1[1])
    assert np.array_equal(_bits(out), _bits(d))
    holes = np.full_like(d, -1.0)                         # every pixel is in F, still T = 0: NaN payload copied
    assert np.array_equal(_bits(_both(d, g, 1, rw, ONES1[1], holes=holes)), _bits(d))


def test_range_weight_follows_the_guide():
    d = _f([[1.0, 1.0, 9.0, 9.0, 9.0]])
    g = _f([[10.0, 10.0, 200.0, 200.0, 200.0]])
    rw = np.zeros(256, np.uint16)
    rw[0] = 1
    # r = 2: the centre (0, 1) sees 1, 1, 9, 9 unweighted (median 1) -- now only the pixels of equal guide count
    assert _both(d, g, 2, rw, np.ones(9, np.uint16)).tolist() == [[1.0, 1.0, 9.0, 9.0, 9.0]]
    rw[:] = 1
    rw[0] = 0                                             # only different guide values count; (0, 4) sees none: T = 0
    assert _both(d, g, 2, rw, np.ones(9, np.uint16)).tolist() == [[9.0, 9.0, 1.0, 1.0, 9.0]]


def test_range_index_truncates_and_saturates():
    gp = _f([0.0, 0.0, 0.0, 0.0, NAN, 0.0, 10.0])
    gq = _f([0.99, 254.99, 255.0, 1e30, 0.0, -INF, 8.5])
    assert ref.range_index(gp, gq).tolist() == [0, 254, 255, 255, 255, 255, 1]


def test_clipped_window_at_a_corner():
    d = _f([[5.0, 5.0, 0.0], [5.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    g = np.zeros_like(d)
    out = _both(d, g, 1, *ONES1)
    assert out[0, 0] == 5.0                               # 2 x 2 window: three 5s, one 0 (wrap-around would give 0)
    assert out[2, 2] == 0.0


def test_holes_equal_to_in_fills_the_non_valid_pixels():
    d = _f([[1.0, -1.0, 3.0, NAN, 3.0]])
    g = np.zeros_like(d)
    out = _both(d, g, 1, *ONES1, holes=d)
    assert out.tolist()[0][:3] == [1.0, 1.0, 3.0] and out[0, 3] == 3.0 and out[0, 4] == 3.0
    iso = _f([[-1.0, -1.0, -1.0]])                        # no valid sample anywhere: T = 0, copied
    assert _both(iso, np.zeros_like(iso), 1, *ONES1, holes=iso).tolist() == [[-1.0, -1.0, -1.0]]


def test_holes_mode_changes_only_the_filled_pixels():
    rng = np.random.default_rng(3)
    before = rng.integers(0, 8, (9, 11)).astype(np.float32)
    before[rng.random(before.shape) < 0.3] = -1.0
    filled = np.where(before == -1.0, 4.5, before).astype(np.float32)
    g = rng.uniform(0, 255, before.shape).astype(np.float32)
    rw, sw = rng.integers(0, 1024, 256).astype(np.uint16), rng.integers(0, 1024, 9).astype(np.uint16)
    out = _both(filled, g, 2, rw, sw, holes=before)
    keep = before != -1.0
    assert np.array_equal(_bits(out[keep]), _bits(filled[keep]))
    assert not np.array_equal(out[~keep], filled[~keep])


def test_maps_are_independent():
    d = np.stack([np.full((3, 3), 1.0, np.float32), np.full((3, 3), 2.0, np.float32)])
    d[0, 1, 1] = 2.0                                       # alone in map 0: the median is 1
    g = np.zeros_like(d)
    out = ref.weighted_median(d, g, 1, *ONES1)
    assert out[0, 1, 1] == 1.0 and np.all(out[1] == 2.0)
