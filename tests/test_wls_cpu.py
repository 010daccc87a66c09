"""Weighted least squares filter, the parts that need no GPU: the CPU reference (tests/wls_ref.py) against a plain
element-by-element version and hand-computed answers, the properties the rule promises, the table formulas, every C-ABI
rejection (returned before the device is touched), the new keyword arguments, and a quality check of the rule."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import postprocess_ref as post
import wls_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("smx_wls_workspace_bytes", "smx_wls_filter")
NAN, INF = float("nan"), float("inf")
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _both(d, g, lam, rw, **kw):
    """The vectorised reference, checked bit for bit against the element-by-element one."""
    out = ref.wls_filter(d, g, lam, rw, **kw)
    loop = ref.wls_filter_loop(d, g, lam, rw, **kw)
    assert np.array_equal(_bits(out), _bits(loop))
    return out


# ----------------------------------------------------------------------------- the reference
def test_reference_matches_the_plain_loop_with_special_values():
    rng = np.random.default_rng(1)
    for H, W, inv in ((1, 1, -1.0), (1, 9, -1.0), (8, 1, 0.0), (6, 11, -1.0), (9, 7, 5.0)):
        d = (rng.integers(0, 5, (H, W)) * 3.0 + rng.uniform(-0.5, 0.5, (H, W))).astype(np.float32)
        mask = rng.random((H, W)) < 0.3
        d[mask] = rng.choice(np.array([NAN, INF, -INF, inv, -0.0, 0.0], np.float32), int(mask.sum()))
        g = rng.uniform(0, 60, (H, W)).astype(np.float32)
        g[rng.random((H, W)) < 0.1] = NAN
        conf = rng.uniform(-0.5, 1.5, (H, W)).astype(np.float32)
        conf[rng.random((H, W)) < 0.1] = NAN
        lam = np.array([40.0, 10.0, 2.5], np.float32)
        rw = np.exp(-np.arange(256) / 8.0).astype(np.float32)
        _both(d, g, lam, rw, invalid_disparity=inv)
        _both(d, g, lam, rw, confidence=conf, min_weight=0.0, invalid_disparity=inv)


def test_three_pixel_line_by_hand():
    d = np.array([[3.0, -1.0, 7.0]], np.float32)                 # the middle pixel is invalid
    g = np.zeros_like(d)
    lam = np.array([1.0], np.float32)
    rw = np.ones(256, np.float32)
    # rows: s = 1, 1; b = 2, 3, 2.  U = (3, 0, 7), V = (1, 0, 1).
    # forward r0 = 1/2, e0 = 1/2; r1 = 1/(3 - 1/2) = 2/5, e1 = 2/5; r2 = 1/(2 - 2/5) = 5/8
    # U: y = (3/2, (0 + 3/2) 2/5 = 3/5, (7 + 3/5) 5/8 = 19/4); x2 = 19/4, x1 = 3/5 + 2/5 19/4 = 5/2, x0 = 3/2 + 5/4 = 11/4
    # V: y = (1/2, 1/5, 3/4); x = (3/4, 1/2, 3/4).  Columns have length 1: unchanged.  out = U / V = (11/3, 5, 19/3)
    out = _both(d, g, lam, rw, min_weight=0.0)
    expect = np.array([[F(11 / 4) / F(3 / 4), F(5 / 2) / F(1 / 2), F(19 / 4) / F(3 / 4)]], np.float32)
    assert np.array_equal(out, expect), out
    assert abs(out[0, 1] - 5.0) < 1e-6                         # the hole takes the mean of its two neighbours


def test_lambda_zero_is_the_identity_on_valid_pixels():
    rng = np.random.default_rng(2)
    d = rng.uniform(-50, 50, (13, 17)).astype(np.float32)
    d[rng.random(d.shape) < 0.3] = -1.0
    d[2, 3], d[4, 5], d[6, 7] = NAN, INF, 1e-40                  # a denormal value is valid and kept
    g = rng.uniform(0, 255, d.shape).astype(np.float32)
    rw = np.ones(256, np.float32)
    out = _both(d, g, np.zeros(3, np.float32), rw)
    valid = ref.valid_mask(d, -1.0)
    assert np.array_equal(_bits(out[valid]), _bits(d[valid]))
    assert np.all(out[~valid] == -1.0)


def test_zero_weight_guide_edge_decouples_exactly():
    rng = np.random.default_rng(3)
    H, W = 10, 16
    g = np.where(np.arange(W)[None, :] < 7, 20.0, 120.0).astype(np.float32) * np.ones((H, 1), np.float32)
    rw = np.exp(-np.arange(256) / 4.0).astype(np.float32)
    rw[100:] = 0.0                                                # the step of 100 grey levels has weight 0
    lam = np.array([500.0, 125.0], np.float32)
    d1 = rng.uniform(0, 30, (H, W)).astype(np.float32)
    d1[rng.random(d1.shape) < 0.3] = -1.0
    d2 = d1.copy()
    d2[:, 7:] = rng.uniform(-100, 100, (H, W - 7)).astype(np.float32)
    o1, o2 = ref.wls_filter(d1, g, lam, rw), ref.wls_filter(d2, g, lam, rw)
    assert np.array_equal(_bits(o1[:, :7]), _bits(o2[:, :7]))
    assert not np.array_equal(o1[:, 7:], o2[:, 7:])


def test_denormal_decay_from_one_confident_pixel():
    H, W = 3, 200
    d = np.full((H, W), -1.0, np.float32)
    d[1, 0] = 10.0
    g = np.zeros((H, W), np.float32)
    rw = np.full(256, 0.01, np.float32)                          # small weights: V falls by ~100x per pixel
    lam = np.array([1.0], np.float32)
    u, v = ref.planes(d, None, -1.0)
    (x,) = ref.solve_lines([v], g, lam[0], rw)
    row = x[1]
    tiny = (row > 0) & (row < np.finfo(np.float32).tiny)
    assert tiny.any(), "V reaches the denormal range"
    out = _both(d, g, lam, rw, min_weight=0.0)
    assert np.isfinite(out[1, :]).any()
    # where V is a denormal the output is still U / V, not invalid
    (xu, xv) = ref.solve_lines([u, v], g, lam[0], rw)
    dn = (xv[1] > 0) & (xv[1] < np.finfo(np.float32).tiny)
    assert dn.any()


def test_pivots_stay_positive_at_the_largest_lambda():
    N = 4000
    g = np.zeros((1, N), np.float32)
    rw = np.ones(256, np.float32)
    lam = F(2.0 ** 20)
    s = np.full(N - 1, lam, np.float32)
    e = F(0.0)
    piv = []
    for j in range(N):
        L = s[j - 1] if j > 0 else F(0)
        R = s[j] if j < N - 1 else F(0)
        b = F(F(F(1) + L) + R)
        den = b if j == 0 else F(b - F(L * e))
        piv.append(float(den))
        e = F(R * F(F(1) / den))
    assert min(piv) >= 0.5, min(piv)                             # exact: >= 1 + R_j; the last one >= 1
    f = np.random.default_rng(4).uniform(0, 64, (1, N)).astype(np.float32)
    (x,) = ref.solve_lines([f], g, lam, rw)
    assert np.all(np.isfinite(x))


def test_maps_are_independent():
    rng = np.random.default_rng(5)
    d = rng.uniform(0, 40, (3, 9, 12)).astype(np.float32)
    d[rng.random(d.shape) < 0.4] = -1.0
    g = rng.uniform(0, 255, d.shape).astype(np.float32)
    lam, rw = np.array([30.0, 7.5], np.float32), np.exp(-np.arange(256) / 10.0).astype(np.float32)
    both = ref.wls_filter(d, g, lam, rw)
    for i in range(3):
        assert np.array_equal(_bits(both[i]), _bits(ref.wls_filter(d[i], g[i], lam, rw)))


# ----------------------------------------------------------------------------- tables and keywords
def test_table_formulas():
    import cuda_depth
    lam, rw = cuda_depth.wls_tables(8000.0, 1.5, 3, 0.25)
    assert lam.dtype == np.float32 and lam.tolist() == [8000.0, 2000.0, 500.0]
    assert rw.dtype == np.float32 and rw.shape == (256,)
    assert rw[0] == 1.0 and rw[1] == F(math.exp(-1 / 1.5)) and rw[255] == F(math.exp(-255 / 1.5))
    lam, _ = cuda_depth.wls_tables(1000.0, 2.0, 8, 0.3)
    assert lam.tolist() == [F(1000.0 * 0.3 ** t) for t in range(8)]
    lam, _ = cuda_depth.wls_tables(2.0 ** 20, 1.0, 1, 1.0)
    assert lam.tolist() == [2.0 ** 20]


def test_python_entries_reject_bad_scalars_before_the_device():
    import cuda_depth
    t = object()                                                  # never reached: the scalars are checked first
    for kw, msg in ((dict(lam=-1.0), "lam must be finite"), (dict(lam=NAN), "lam must be finite"),
                    (dict(lam=2.0 ** 20 + 1), "lam must be finite"), (dict(sigma_color=0.0), "sigma_color"),
                    (dict(sigma_color=INF), "sigma_color"), (dict(iterations=0), "iterations must be in 1..8"),
                    (dict(iterations=9), "iterations must be in 1..8"), (dict(attenuation=0.0), "attenuation"),
                    (dict(attenuation=1.5), "attenuation"), (dict(min_weight=-1.0), "min_weight"),
                    (dict(min_weight=NAN), "min_weight"), (dict(invalid_disparity=NAN), "invalid_disparity")):
        with pytest.raises(RuntimeError, match=msg):
            cuda_depth.wls_filter(t, t, **kw)
    with pytest.raises(TypeError, match="iterations must be an int"):
        cuda_depth.wls_tables(10.0, 1.0, 3.0)
    with pytest.raises(TypeError, match="lam must be a number"):
        cuda_depth.wls_tables(True, 1.0)


def test_backend_and_pipeline_keywords_and_defaults():
    from pipeline import DepthEstimationPipeline
    from pipeline.depth import CudaStereoMatchingBackend, SgmStereoMatchingBackend
    for cls in (CudaStereoMatchingBackend, SgmStereoMatchingBackend, DepthEstimationPipeline):
        p = inspect.signature(cls.__init__).parameters
        for name, default in (("wls_lambda", 0.0), ("wls_sigma_color", 1.5), ("wls_iterations", 3)):
            assert name in p, (cls, name)
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY, (cls, name)
            assert p[name].default == default and type(p[name].default) is type(default), (cls, name)


def test_wls_excludes_fill_and_median():
    from pipeline.depth.map_postprocessing import MapPostprocessing
    m = MapPostprocessing()
    for kw in (dict(fill_invalid=True), dict(median_radius=3)):
        with pytest.raises(ValueError, match="wls_lambda"):
            m._init_postprocessing((8, 8), wls_lambda=100.0, **kw)
    with pytest.raises(RuntimeError, match="iterations must be in 1..8"):
        m._init_postprocessing((8, 8), wls_lambda=100.0, wls_iterations=0)
    with pytest.raises(RuntimeError, match="sigma_color"):
        m._init_postprocessing((8, 8), wls_sigma_color=-1.0)          # checked even when off
    m._init_postprocessing((8, 8), fill_invalid=True, median_radius=3)   # off: no conflict
    assert not m._uses_guide() or m._median_radius > 0
    m._init_postprocessing((8, 8), wls_lambda=100.0, speckle_max_size=10)
    assert m._uses_guide() and m._wls_tables[0].tolist() == [100.0, 25.0, 6.25]


# ----------------------------------------------------------------------------- C ABI
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
    q = native.LIB.smx_wls_workspace_bytes
    assert q(1, 375, 1242) == 3 * ((375 * 1242 * 4 + 255) // 256 * 256)
    assert q(2, 1, 1) == 3 * 256
    for n, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 32769, 4), (1, 4, 32769), (-1, 4, 4)):
        assert q(n, H, W) == 0, (n, H, W)


# fake device pointers: never dereferenced, every check returns first
IN, CONF, GUIDE, OUT, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
MAP_BYTES = 2 * 4 * 4 * 4                                      # n = 2, H = W = 4


def _call(native, **change):
    a = dict(dev=0, n=2, H=4, W=4, i=IN, c=CONF, g=GUIDE, o=OUT, T=2, lam=np.array([10.0, 2.5], np.float32),
             rw=np.ones(256, np.float32), mw=1e-3, inv=-1.0, ws=WS, wsb=3 * 256, s=None)
    a.update(change)
    lp = None if a["lam"] is None else a["lam"].ctypes.data
    rp = None if a["rw"] is None else a["rw"].ctypes.data
    return native.LIB.smx_wls_filter(a["dev"], a["n"], a["H"], a["W"], a["i"], a["c"], a["g"], a["o"], a["T"], lp, rp,
                                     a["mw"], a["inv"], a["ws"], a["wsb"], a["s"])


def test_wls_filter_rejects_bad_arguments_without_a_device(native):
    def lam_with(v):
        return np.array([10.0, v], np.float32)

    def rw_with(k, v):
        rw = np.ones(256, np.float32)
        rw[k] = v
        return rw

    cases = [
        (dict(i=None), "in, guide and out must be non-NULL"),
        (dict(g=None), "in, guide and out must be non-NULL"),
        (dict(o=None), "in, guide and out must be non-NULL"),
        (dict(lam=None), "lambdas and range_weight must be non-NULL"),
        (dict(rw=None), "lambdas and range_weight must be non-NULL"),
        (dict(n=0), "need n >= 1"),
        (dict(H=0), "1 <= H, W <= 32768"),
        (dict(W=32769), "1 <= H, W <= 32768"),
        (dict(T=0), "num_iterations must be in 1..8"),
        (dict(T=9, lam=np.ones(9, np.float32)), "num_iterations must be in 1..8"),
        (dict(lam=lam_with(NAN)), "lambdas[1] = nan is not finite in [0, 2^20]"),
        (dict(lam=lam_with(INF)), "lambdas[1] = inf"),
        (dict(lam=lam_with(-1.0)), "lambdas[1] = -1"),
        (dict(lam=lam_with(2.0 ** 20 + 128)), "lambdas[1]"),
        (dict(rw=rw_with(7, 1.0000001)), "range_weight[7]"),
        (dict(rw=rw_with(255, -0.5)), "range_weight[255] = -0.5 is not finite in [0, 1]"),
        (dict(rw=rw_with(0, NAN)), "range_weight[0] = nan"),
        (dict(mw=-1.0), "min_weight must be finite and >= 0"),
        (dict(mw=NAN), "min_weight must be finite and >= 0"),
        (dict(mw=INF), "min_weight must be finite and >= 0"),
        (dict(inv=NAN), "invalid_disparity must be finite"),
        (dict(inv=-INF), "invalid_disparity must be finite"),
        (dict(ws=None), "workspace is NULL or workspace_bytes"),
        (dict(wsb=3 * 256 - 1), "is below smx_wls_workspace_bytes = 768"),
        (dict(o=IN + 4), "out must not overlap confidence or guide, and overlap in only as the same buffer"),
        (dict(o=IN - MAP_BYTES + 4), "overlap in only as the same buffer"),
        (dict(o=CONF), "out must not overlap confidence or guide"),
        (dict(o=GUIDE + 8), "out must not overlap confidence or guide"),
        (dict(ws=IN + 16), "the workspace must not overlap"),
        (dict(ws=CONF - 16), "the workspace must not overlap"),
        (dict(ws=GUIDE + 16), "the workspace must not overlap"),
        (dict(ws=OUT - 16), "the workspace must not overlap"),
        (dict(ws=WS + 4), "workspace must be 256-byte aligned"),
        (dict(ws=WS + 128, s=native.STREAM_ENGINE), "workspace must be 256-byte aligned"),
        (dict(s=native.STREAM_ENGINE), "needs a caller stream"),
    ]
    for change, msg in cases:
        rc = _call(native, **dict(change))
        assert rc == -1, change
        assert msg in native.last_error(), (change, msg, native.last_error())


def test_accepted_aliasing_reaches_the_stream_check(native):
    """out == in, and in, confidence and guide sharing a buffer, pass every operand check (the engine-stream sentinel
    then stops the call before the device)."""
    for change in (dict(o=IN), dict(c=IN, g=IN), dict(c=None), dict(T=8, lam=np.full(8, 2.0 ** 20, np.float32)),
                   dict(rw=np.zeros(256, np.float32), mw=0.0)):
        rc = _call(native, s=native.STREAM_ENGINE, **change)
        assert rc == -1 and "needs a caller stream" in native.last_error(), (change, native.last_error())


def test_only_the_first_T_lambdas_are_read(native):
    lam = np.array([10.0, 2.5, NAN], np.float32)                 # T = 2: the NaN behind the table is not part of it
    rc = _call(native, lam=lam, s=native.STREAM_ENGINE)
    assert rc == -1 and "needs a caller stream" in native.last_error()


# ----------------------------------------------------------------------------- quality of the rule
def _scene(seed=6, H=60, W=90):
    """Piecewise-constant disparity with a guide whose steps coincide with the disparity edges, 30 % of the pixels
    invalid and 3 % outliers."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    region = (x >= 30).astype(int) + (x >= 65).astype(int) + 3 * ((y >= 25) & (x >= 15) & (x < 50)).astype(int)
    levels = np.array([8.0, 20.0, 33.0, 45.0, 0, 0, 0], np.float32)
    greys = np.array([40.0, 110.0, 180.0, 230.0, 0, 0, 0], np.float32)
    truth = levels[np.minimum(region, 3)].astype(np.float32)
    guide = (greys[np.minimum(region, 3)] + rng.uniform(-1.0, 1.0, (H, W))).astype(np.float32)
    d = truth + rng.normal(0, 0.3, (H, W)).astype(np.float32)
    out = rng.random((H, W)) < 0.03
    d[out] = rng.uniform(0, 60, int(out.sum()))
    d[rng.random((H, W)) < 0.3] = -1.0
    return d.astype(np.float32), guide, truth


def test_wls_beats_the_background_fill_on_a_piecewise_constant_scene():
    import cuda_depth
    d, guide, truth = _scene()
    lam, rw = cuda_depth.wls_tables(8000.0, 1.5, 3, 0.25)
    out = ref.wls_filter(d, guide, lam, rw)
    filled = post.fill_invalid(d)
    assert np.all(out != -1.0)
    mae_wls = float(np.abs(out - truth).mean())
    mae_fill = float(np.abs(filled - truth).mean())
    print(f"MAE wls {mae_wls:.3f}, fill {mae_fill:.3f}")
    assert mae_wls < 0.6 * mae_fill, (mae_wls, mae_fill)
