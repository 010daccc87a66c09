"""Per-pixel confidence, the parts that need no GPU: the CPU reference (tests/confidence_ref.py) against a plain per-pixel
loop and hand-computed pixels, every C-ABI rejection of smx_confidence_map and smx_sgm_with_right_map (returned before
the device is touched), the Python and pipeline keyword checks, and a quality check: the WLS filter weighted by the
confidence beats the one with binary confidence on a scene with known disparity and injected outliers."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import confidence_ref as ref
import stereo_synthetic as syn
import wls_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("smx_confidence_map", "smx_sgm_with_right_map")
NAN, INF = float("nan"), float("inf")
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _both(d, right=None, guide=None, **kw):
    """The vectorised reference, checked bit for bit against the per-pixel loop."""
    out = ref.confidence_map(d, right, guide, **kw)
    loop = ref.confidence_map_loop(d, right, guide, **kw)
    assert np.array_equal(_bits(out), _bits(loop)), np.argwhere(_bits(out) != _bits(loop))[:5]
    return out


def _special_map(rng, shape, inv):
    d = (rng.integers(0, 6, shape) + rng.uniform(-0.6, 0.6, shape)).astype(np.float32)
    mask = rng.random(shape) < 0.3
    d[mask] = rng.choice(np.array([NAN, INF, -INF, inv, -0.0, 0.0, 1e-41, -2.0], np.float32), int(mask.sum()))
    return d


# ----------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("H,W,inv,radius", [(1, 1, -1.0, 1), (1, 13, -1.0, 2), (11, 1, 0.0, 3), (7, 12, -1.0, 2),
                                            (9, 8, 4.0, 15), (5, 6, -1.0, 1)])
def test_reference_matches_the_plain_loop_with_special_values(H, W, inv, radius):
    rng = np.random.default_rng(H * 100 + W)
    d = _special_map(rng, (H, W), inv)
    r = _special_map(rng, (H, W), inv)
    g = (rng.integers(0, 4, (H, W)) * 7.0).astype(np.float32)
    gm = rng.random((H, W))
    g[gm < 0.15] = NAN
    g[(gm >= 0.15) & (gm < 0.2)] = INF
    g[(gm >= 0.2) & (gm < 0.25)] = -0.0
    for right in (None, r):
        for guide in (None, g):
            for lr, ts in ((1.0, 10.0), (0.3, 2.5), (3e-39, 1e-40)):
                _both(d, right, guide, radius=radius, lr_scale=lr, texture_scale=ts, invalid_disparity=inv)


def test_border_indices_and_all_nan_windows():
    # row 0: t = Y at every column (points at column 0); row 1: t = Y + 1 (outside the row)
    W = 6
    d = np.array([np.arange(W), np.arange(W) + 1.0], np.float32) + F(0.25)
    r = np.full((2, W), 0.0, np.float32)
    r[0, 0] = 3.0
    got = _both(d, r, None, lr_scale=10.0)
    assert np.all(got[1] == 0)
    for Y in range(W):                                # t = Y: every pixel of row 0 reads D_R[0][0] = 3
        assert got[0, Y] == F(F(1) - F(F(abs(F(Y + 0.25) - F(3.0))) / F(10.0))), Y
    # an all-NaN guide window gives 0; a window with one value gives range 0
    g = np.full((5, 5), NAN, np.float32)
    g[0, 0] = 7.0
    ones = np.ones((5, 5), np.float32)
    c = _both(ones, None, g, radius=1)
    assert c[4, 4] == 0 and c[0, 0] == 0 and c[1, 1] == 0
    # +inf only in a window: inf - inf is NaN -> 0; +inf with a finite value: range inf -> 1
    g2 = np.full((3, 3), INF, np.float32)
    g2[2, 2] = 1.0
    c2 = _both(np.ones((3, 3), np.float32), None, g2, radius=1)
    assert c2[0, 0] == 0 and c2[1, 1] == 1 and c2[2, 2] == 1


def test_signed_zero_range_is_plus_zero():
    g = np.array([[-0.0, 0.0], [0.0, -0.0]], np.float32)
    c = _both(np.ones((2, 2), np.float32), None, g, radius=1)
    assert np.all(_bits(c) == 0)


def test_hand_computed_pixels():
    # one row, no guide: d = 5.3 -> t = 5, r = D_R[0][Y - 5]
    d = np.full((1, 8), -1.0, np.float32)
    r = np.full((1, 8), -1.0, np.float32)
    d[0, 7] = 5.3
    r[0, 2] = 5.0
    d[0, 6] = 5.6                                     # t = 6 -> column 0, invalid there -> 0
    d[0, 5] = 4.4                                     # t = 4 -> column 1, invalid -> 0
    got = _both(d, r, None, lr_scale=1.0)
    assert got[0, 7] == F(1.0) - F(F(5.3) - F(5.0))
    assert got[0, 6] == 0 and got[0, 5] == 0
    assert np.all(got[0, :5] == 0)
    # texture only: a 3x3 guide, radius 1, range at the centre 8 - 0
    g = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.float32)
    t = _both(np.ones((3, 3), np.float32), None, g, radius=1, texture_scale=10.0)
    assert t[1, 1] == F(0.8) and t[0, 0] == F(F(4.0) / F(10.0)) and t[2, 2] == F(0.4)
    # the product of the two terms
    both = _both(np.full((3, 3), 0.25, np.float32), np.full((3, 3), 0.0, np.float32), g, radius=1,
                 lr_scale=0.5, texture_scale=4.0)
    assert both[1, 1] == F(F(0.5) * F(1.0)) and both[0, 0] == F(F(0.5) * F(1.0))


def test_maps_are_independent_and_in_unit_range():
    rng = np.random.default_rng(3)
    n, H, W = 3, 17, 23
    d = _special_map(rng, (n, H, W), -1.0)
    r = _special_map(rng, (n, H, W), -1.0)
    g = rng.uniform(0, 30, (n, H, W)).astype(np.float32)
    batch = ref.confidence_map(d, r, g, radius=2)
    for i in range(n):
        assert np.array_equal(_bits(batch[i]), _bits(ref.confidence_map(d[i], r[i], g[i], radius=2)))
    assert np.all((batch >= 0) & (batch <= 1)) and not np.any(np.signbit(batch))


# ----------------------------------------------------------------------------- Python and pipeline checks
def test_python_entry_rejects_bad_scalars_before_the_device():
    import cuda_depth
    t = object()                                                  # never reached: the scalars are checked first
    for kw, msg in ((dict(radius=0), "radius must be in 1..15"), (dict(radius=16), "radius must be in 1..15"),
                    (dict(lr_scale=0.0), "lr_scale must be finite and > 0"), (dict(lr_scale=NAN), "lr_scale"),
                    (dict(lr_scale=INF), "lr_scale"), (dict(texture_scale=-1.0), "texture_scale"),
                    (dict(texture_scale=INF), "texture_scale"), (dict(invalid_disparity=NAN), "invalid_disparity")):
        with pytest.raises(RuntimeError, match=msg):
            cuda_depth.confidence_map(t, **kw)
    with pytest.raises(TypeError, match="radius must be an int"):
        cuda_depth.confidence_map(t, radius=2.0)
    with pytest.raises(TypeError, match="lr_scale must be a number"):
        cuda_depth.confidence_map(t, lr_scale=True)
    p = inspect.signature(cuda_depth.confidence_map).parameters
    assert [p[k].default for k in ("radius", "lr_scale", "texture_scale", "invalid_disparity", "out")] == \
        [2, 1.0, 10.0, -1.0, None]
    assert "right_out" in inspect.signature(cuda_depth.StereoSGM.compute).parameters


def test_backend_and_pipeline_keywords_and_defaults():
    from pipeline import DepthEstimationPipeline, DepthEstimationResult
    from pipeline.depth import CudaStereoMatchingBackend, SgmStereoMatchingBackend
    for cls in (CudaStereoMatchingBackend, SgmStereoMatchingBackend, DepthEstimationPipeline):
        p = inspect.signature(cls.__init__).parameters
        for name, default in (("confidence", False), ("confidence_lr_scale", 1.0), ("confidence_radius", 2),
                              ("confidence_texture_scale", 10.0)):
            assert name in p, (cls, name)
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY, (cls, name)
            assert p[name].default == default and type(p[name].default) is type(default), (cls, name)
    fields = list(DepthEstimationResult.__dataclass_fields__)
    assert fields[-1] == "confidence_map" and DepthEstimationResult.__dataclass_fields__["confidence_map"].default is None


def test_pipeline_keyword_validation():
    from pipeline.depth.map_postprocessing import MapPostprocessing
    m = MapPostprocessing()
    with pytest.raises(TypeError, match="confidence must be a bool"):
        m._init_postprocessing((8, 8), confidence=1)
    for kw, msg in ((dict(confidence_radius=16), "radius must be in 0..15"),
                    (dict(confidence_radius=-1), "radius must be in 0..15"),
                    (dict(confidence_lr_scale=0.0), "lr_scale"), (dict(confidence_texture_scale=NAN), "texture_scale")):
        with pytest.raises(RuntimeError, match=msg):
            m._init_postprocessing((8, 8), **kw)                      # checked even when off
        with pytest.raises(RuntimeError, match=msg):
            m._init_postprocessing((8, 8), confidence=True, **kw)
    with pytest.raises(TypeError, match="radius must be an int"):
        m._init_postprocessing((8, 8), confidence=True, confidence_radius=2.5)
    m._init_postprocessing((8, 8))
    assert not m._uses_guide() and m.confidence_map() is None
    m._init_postprocessing((8, 8), confidence=True)
    assert m._uses_guide()                                            # the texture term reads the left gray plane
    m._init_postprocessing((8, 8), confidence=True, confidence_radius=0)
    assert not m._uses_guide()                                        # LR term only


# ----------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from cuda_depth import _native
    return _native


def test_the_symbols_are_declared_listed_and_exported(native):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stereo_mi355x.h")).read(), flags=re.S)
    lib = C.CDLL(native.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in native.EXPORTS, name
        assert hasattr(lib, name), name
    assert native.LIB.smx_abi_version() == 4


# fake device pointers: never dereferenced, every check returns first
LEFT, RIGHT, GUIDE, OUT = 0x100000, 0x200000, 0x300000, 0x400000
MAP_BYTES = 2 * 4 * 4 * 4                                      # n = 2, H = W = 4


def _call(native, **change):
    a = dict(dev=0, n=2, H=4, W=4, l=LEFT, r=RIGHT, g=GUIDE, R=2, lr=1.0, ts=10.0, inv=-1.0, o=OUT, s=None)
    a.update(change)
    return native.LIB.smx_confidence_map(a["dev"], a["n"], a["H"], a["W"], a["l"], a["r"], a["g"], a["R"], a["lr"],
                                         a["ts"], a["inv"], a["o"], a["s"])


CONF_REJECTIONS = [
    (dict(l=None), "left_disp and out must be non-NULL"),
    (dict(o=None), "left_disp and out must be non-NULL"),
    (dict(n=0), "need n >= 1"),
    (dict(H=0), "1 <= H, W <= 32768"),
    (dict(W=32769), "1 <= H, W <= 32768"),
    (dict(H=32769), "1 <= H, W <= 32768"),
    (dict(R=0), "radius must be in 1..15 with a guide"),
    (dict(R=16), "radius must be in 1..15 with a guide"),
    (dict(lr=0.0), "lr_scale must be finite and > 0"),
    (dict(lr=-1.0), "lr_scale must be finite and > 0"),
    (dict(lr=NAN), "lr_scale must be finite and > 0"),
    (dict(lr=INF), "lr_scale must be finite and > 0"),
    (dict(ts=0.0), "texture_scale must be finite and > 0"),
    (dict(ts=NAN), "texture_scale must be finite and > 0"),
    (dict(ts=INF), "texture_scale must be finite and > 0"),
    (dict(inv=NAN), "invalid_disparity must be finite"),
    (dict(inv=-INF), "invalid_disparity must be finite"),
    (dict(o=LEFT), "out must not overlap left_disp, right_disp or guide"),
    (dict(o=LEFT + MAP_BYTES - 4), "out must not overlap"),
    (dict(o=RIGHT - MAP_BYTES + 4), "out must not overlap"),
    (dict(o=GUIDE + 8), "out must not overlap"),
    (dict(s=-1), "needs a caller stream"),
]


@pytest.mark.parametrize("change,msg", CONF_REJECTIONS, ids=[f"{i}" for i in range(len(CONF_REJECTIONS))])
def test_confidence_map_rejects_bad_arguments_without_a_device(native, change, msg):
    if change.get("s") == -1:
        change = dict(change, s=native.STREAM_ENGINE)
    rc = _call(native, **change)
    assert rc == -1, change
    assert msg in native.last_error(), (change, msg, native.last_error())


def test_accepted_arguments_reach_the_stream_check(native):
    """NULL right_disp or guide, any radius without a guide, inputs aliasing each other and out right behind an
    input pass every operand check (the engine-stream sentinel then stops the call before the device)."""
    for change in (dict(r=None), dict(g=None), dict(g=None, R=0), dict(g=None, R=99), dict(r=None, g=None),
                   dict(r=LEFT, g=LEFT), dict(o=LEFT + MAP_BYTES), dict(R=15), dict(R=1), dict(lr=1e-30, ts=3e38),
                   dict(n=1, H=32768, W=32768, l=1 << 40, r=2 << 40, g=3 << 40, o=4 << 40)):
        rc = _call(native, s=native.STREAM_ENGINE, **change)
        assert rc == -1 and "needs a caller stream" in native.last_error(), (change, native.last_error())


def _sgm_args(**over):
    a = dict(device_id=0, n=1, channels=3, dtype=0, H=8, W=16, left=0x10000, right=0x20000, min_disparity=0,
             num_disparities=8, paths=8, P1=10, P2=120, uniqueness=0, lr_max_diff=-1.0, subpixel=1,
             invalid_disparity=-1.0, out=0x40000, gray_left_out=None, right_out=0x80000, workspace=0x100000,
             workspace_bytes=1 << 30, stream=None)
    a.update(over)
    return list(a.values())


SGM_REJECTIONS = [
    (dict(right_out=None), "right_out must be non-NULL"),
    (dict(left=None), "must be non-NULL"),
    (dict(num_disparities=257), "num_disparities must be in 1..256"),
    (dict(right_out=0x10000 + 100), "must not overlap left, right or the workspace"),
    (dict(right_out=0x100000 + 64), "must not overlap left, right or the workspace"),
    (dict(right_out=0x40000 + 4), "right_out overlaps out or gray_left_out"),
    (dict(right_out=0x60000, gray_left_out=0x60000 + 8), "right_out overlaps out or gray_left_out"),
    (dict(out=0x80000 + 4), "right_out overlaps out or gray_left_out"),
    (dict(workspace=0x100000 + 8), "workspace must be 256-byte aligned"),
]


@pytest.mark.parametrize("over,msg", SGM_REJECTIONS, ids=[f"{i}" for i in range(len(SGM_REJECTIONS))])
def test_sgm_with_right_map_rejections(native, over, msg):
    rc = native.LIB.smx_sgm_with_right_map(*_sgm_args(**over))
    assert rc != native.SMX_OK
    assert msg in native.last_error(), native.last_error()


def test_sgm_with_right_map_reaches_the_stream_check(native):
    for over in (dict(), dict(gray_left_out=0x60000), dict(lr_max_diff=1.0)):
        rc = native.LIB.smx_sgm_with_right_map(*_sgm_args(stream=native.STREAM_ENGINE, **over))
        assert rc != native.SMX_OK and "needs a caller stream" in native.last_error(), native.last_error()


# ----------------------------------------------------------------------------- quality
def outlier_scene(seed=7, H=64, W=128, D=32):
    """A stereo_synthetic pair's left texture and band disparity, a left map with 0.2 px noise, 25 % invalid pixels and
    10 % outliers, and the right-view map of the ground truth (the outliers' right-view partners disagree)."""
    left, _, truth = syn.make_pair(H, W, D, 2, seed)
    rng = np.random.default_rng(seed)
    d = (truth + rng.uniform(-0.2, 0.2, (H, W))).astype(np.float32)
    out = rng.random((H, W)) < 0.10
    d[out] = (truth[out] + rng.choice([-1.0, 1.0], int(out.sum())) * rng.uniform(3.0, 12.0, int(out.sum())))
    d[rng.random((H, W)) < 0.25] = -1.0
    right = np.broadcast_to(truth[:, :1], (H, W)).astype(np.float32).copy()    # bands: constant along each row
    cols = np.arange(W)[None, :]
    right[cols + truth > W - 1] = -1.0                                         # no left partner in the image
    return d.astype(np.float32), right, left, truth, out


def test_confidence_weighted_wls_beats_binary_confidence():
    import cuda_depth
    d, right, guide, truth, out = outlier_scene()
    conf = ref.confidence_map(d, right, guide, radius=2, lr_scale=1.0, texture_scale=10.0)
    assert np.all(conf[out & (d != -1.0)] == 0), "every outlier disagrees with its right-view partner"
    good = (d != -1.0) & ~out
    assert np.mean(conf[good]) > 0.6
    lam, rw = cuda_depth.wls_tables(8000.0, 1.5, 3, 0.25)
    binary = wls_ref.wls_filter(d, guide, lam, rw)
    weighted = wls_ref.wls_filter(d, guide, lam, rw, confidence=conf)
    # scored: right of the largest disparity (to its left a pixel may point outside the image and get 0), where both
    # outputs are valid (on this texture the weighted filter leaves a few isolated pixels far from any confident one)
    scored = (binary != -1.0) & (weighted != -1.0)
    scored[:, :int(truth.max()) + 1] = False
    assert scored.mean() > 0.75 and (weighted == -1.0).mean() < 0.1
    mae_bin = float(np.abs(binary - truth)[scored].mean())
    mae_conf = float(np.abs(weighted - truth)[scored].mean())
    print(f"MAE wls binary confidence {mae_bin:.3f}, LR x texture confidence {mae_conf:.3f}")
    assert mae_conf < 0.7 * mae_bin, (mae_conf, mae_bin)
