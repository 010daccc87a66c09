"""Motion-gated temporal filter, the parts that need no GPU: the CPU reference (tests/temporal_ref.py) against a plain
per-pixel loop over multi-frame sequences, every C-ABI rejection of smx_temporal_filter (returned before the device is
touched), the Python and pipeline keyword checks, and the filter's two promises on synthetic streams: it steadies a
static scene, and it passes a moved pixel's measurement through unchanged."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import stereo_sequences as seqs
import stereo_synthetic as syn
import temporal_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _special(rng, shape, values, frac):
    a = np.zeros(shape, np.float32)
    mask = rng.random(shape) < frac
    a[mask] = rng.choice(np.array(values, np.float32), int(mask.sum()))
    return a, mask


def _frame(rng, shape, inv, base_guide, specials=True):
    """A map near 5 px with jitter, holes and special values; a confidence with zeros, > 1 and specials; a guide that
    moves in some places and carries NaN / inf in a few."""
    d = (5.0 + rng.uniform(-1.5, 1.5, shape)).astype(np.float32)
    d[rng.random(shape) < 0.15] = inv
    c = rng.uniform(-0.3, 1.5, shape).astype(np.float32)
    g = (base_guide + rng.integers(-2, 3, shape)).astype(np.float32)
    g[rng.random(shape) < 0.1] += 40.0                                  # local motion
    if specials:
        for a, vals in ((d, [NAN, INF, -INF, inv, -0.0, 1e-41]), (c, [NAN, INF, -INF, 0.0, -0.0, 1e-41, 7.0]),
                        (g, [NAN, INF, -INF])):
            s, m = _special(rng, shape, vals, 0.04)
            a[m] = s[m]
    return d, c, g


def _sequence_check(shape, params, frames, seed, conf=True, specials=True):
    """The vectorised reference against the loop over `frames` calls with the state carried; returns the outputs."""
    rng = np.random.default_rng(seed)
    inv = params.get("invalid_disparity", -1.0)
    base = rng.integers(0, 200, shape).astype(np.float32)
    vec = ref.TemporalRef(shape, **params)
    outs = []
    for f in range(frames):
        d, c, g = _frame(rng, shape, inv, base, specials)
        cc = c if conf else None
        loop_D, loop_A = [], []
        loop_out = []
        for i in range(shape[0]):                                       # the loop is per map: streams are independent
            o, Dn, An = ref.temporal_step_loop(d[i], None if cc is None else cc[i], g[i], vec.G[i], vec.D[i], vec.A[i],
                                               **vec.params)
            loop_out.append(o)
            loop_D.append(Dn)
            loop_A.append(An)
        out = vec.apply(d, g, cc)
        assert np.array_equal(_bits(out), _bits(np.stack(loop_out))), (f, np.argwhere(_bits(out) != _bits(np.stack(loop_out)))[:5])
        assert np.array_equal(_bits(vec.D), _bits(np.stack(loop_D)))
        assert np.array_equal(_bits(vec.A), _bits(np.stack(loop_A))), f
        outs.append(out)
    return outs, vec


# ----------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("shape,radius", [((3, 7, 11), 0), ((3, 9, 5), 1), ((1, 1, 1), 1), ((1, 13, 1), 2),
                                          ((2, 5, 17), 7), ((3, 11, 9), 3)])
def test_reference_matches_the_loop_over_sequences(shape, radius):
    rng = np.random.default_rng(sum(shape) * 10 + radius)
    for trial in range(2):
        params = dict(motion_radius=radius, motion_threshold=float(rng.choice([0.0, 1.0, 3.5, 20.0])),
                      decay=float(rng.choice([1.0, 0.8, 0.31])), max_diff=float(rng.choice([0.0, 0.5, 1.0, 3.0])),
                      max_weight=float(rng.choice([0.5, 2.0, 8.0])), min_weight=float(rng.choice([0.0, 0.25, 1.0])),
                      invalid_disparity=float(rng.choice([-1.0, 0.0, 5.0])))
        for conf in (True, False):
            outs, vec = _sequence_check(shape, params, 5, 100 * trial + radius + conf, conf=conf)
            assert np.all(vec.A >= 0) and np.all(vec.A <= max(F(params["max_weight"]), F(1)))   # a reset sets A = w


def test_first_call_returns_the_valid_measurements():
    rng = np.random.default_rng(1)
    shape = (3, 9, 14)
    d, c, g = _frame(rng, shape, -1.0, np.zeros(shape, np.float32))
    filt = ref.TemporalRef(shape)
    out = filt.apply(d, g)
    valid = np.isfinite(d) & (d != -1.0)
    assert np.array_equal(_bits(out[valid]), _bits(d[valid]))
    assert np.all(out[~valid] == -1.0)
    assert np.array_equal(filt.A, np.where(valid, F(1), F(0)))


def test_hand_computed_pixel():
    # 1 x 1 streams, R = 0: e = |g - G| against T = threshold
    p = dict(motion_radius=0, motion_threshold=2.0, decay=0.5, max_diff=1.0, max_weight=3.0, min_weight=0.5)
    r = ref.TemporalRef((1, 1), **p)
    g = np.array([[10.0]], np.float32)
    assert r.apply(np.array([[4.0]], F), g)[0, 0] == 4.0 and r.A[0, 0] == 1.0
    # static, agree: a = 0.5, w = 1 -> (0.5 * 4 + 4.6) / 1.5
    out = r.apply(np.array([[4.6]], F), g + 2.0)
    assert out[0, 0] == F(F(F(F(0.5) * F(4.0)) + F(4.6)) / F(1.5)) and r.A[0, 0] == F(1.5)
    # moved (|g - G| = 2.5 > 2): reset to the measurement
    assert r.apply(np.array([[7.0]], F), g - 0.5)[0, 0] == 7.0 and r.A[0, 0] == 1.0
    # hold: invalid measurement, a = 0.5 >= min_weight
    assert r.apply(np.array([[-1.0]], F), g - 0.5)[0, 0] == 7.0 and r.A[0, 0] == F(0.5)
    # a = 0.25 < min_weight: invalid
    assert r.apply(np.array([[-1.0]], F), g - 0.5)[0, 0] == -1.0 and r.A[0, 0] == 0
    # confidence 0 at a valid pixel without history: the measurement with weight 0
    assert r.apply(np.array([[3.0]], F), g - 0.5, np.array([[0.0]], F))[0, 0] == 3.0 and r.A[0, 0] == 0
    # disagreement beyond max_diff resets
    r.apply(np.array([[3.0]], F), g - 0.5)
    assert r.apply(np.array([[4.5]], F), g - 0.5)[0, 0] == 4.5 and r.A[0, 0] == 1.0
    # with decay 0.5 the weight tends to 2; with decay 1 it grows by 1 per call up to max_weight
    for _ in range(30):
        r.apply(np.array([[4.5]], F), g - 0.5)
    assert F(1.99) < r.A[0, 0] <= F(2.0)
    r1 = ref.TemporalRef((1, 1), **dict(p, decay=1.0))
    weights = []
    for _ in range(5):
        r1.apply(np.array([[4.5]], F), g)
        weights.append(float(r1.A[0, 0]))
    assert weights == [1.0, 2.0, 3.0, 3.0, 3.0]


def test_window_sum_order_and_nonfinite_guides():
    # a NaN or an inf anywhere in the window: not static; R = 1 reaches one pixel away, clamped at the border
    H, W = 6, 7
    g = np.zeros((1, H, W), F)
    G = np.zeros((1, H, W), F)
    g[0, 2, 3] = NAN
    G[0, 5, 0] = INF
    m = ref.static_mask(g, G, 1, 0.0)[0]
    expect = np.ones((H, W), bool)
    expect[1:4, 2:5] = False
    expect[4:6, 0:2] = False
    assert np.array_equal(m, expect)
    # sums in the stated order: 1e8 + 1 + ... loses the ones in float32, so S = 1e8 <= 1e8 / 9 * 9 depends on order
    g2 = np.zeros((1, 3, 3), F)
    g2[0, 0, 0] = 1e8
    g2[0] += np.array([[0, 1, 1], [1, 1, 1], [1, 1, 1]], F)
    s = ref.motion_sum(g2, np.zeros_like(g2), 1)[0, 1, 1]
    r_rows = [F(F(F(g2[0, i, 0]) + g2[0, i, 1]) + g2[0, i, 2]) for i in range(3)]
    assert s == F(F(r_rows[0] + r_rows[1]) + r_rows[2])


def test_streams_are_independent_and_reset_one():
    rng = np.random.default_rng(4)
    shape = (3, 10, 12)
    base = rng.integers(0, 200, shape).astype(np.float32)
    frames = [_frame(rng, shape, -1.0, base) for _ in range(4)]
    batch = ref.TemporalRef(shape)
    alone = [ref.TemporalRef(shape[1:]) for _ in range(3)]
    for k, (d, c, g) in enumerate(frames):
        if k == 2:
            batch.reset([1])
            alone[1].reset()
        out = batch.apply(d, g, c)
        for i in range(3):
            assert np.array_equal(_bits(out[i]), _bits(alone[i].apply(d[i], g[i], c[i])))


# ----------------------------------------------------------------------------- the filter's promises
def _jitter_maps(frames, H=48, W=96, D=32, seed=3):
    """Truth plus +-0.4 jitter plus 10 % random holes each frame, and a static guide with fresh +-2 noise."""
    left, _, truth = syn.make_slanted_pair(H, W, D, 2, 1)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(frames):
        d = (truth + rng.uniform(-0.4, 0.4, truth.shape)).astype(np.float32)
        d[rng.random(truth.shape) < 0.10] = -1.0
        g = np.clip(left + rng.integers(-2, 3, left.shape), 0, 255).astype(np.float32)
        out.append((d, g))
    return out, truth


def test_static_stream_is_steadier():
    frames, truth = _jitter_maps(16)
    filt = ref.TemporalRef(truth.shape)
    raw, filtered = [], []
    for d, g in frames:
        raw.append(d)
        filtered.append(filt.apply(d, g))
    raw, filtered = np.stack(raw[4:]), np.stack(filtered[4:])            # after the warm-up
    s_raw, s_f = ref.temporal_std(raw), ref.temporal_std(filtered)
    t_raw, t_f = ref.toggle_rate(raw), ref.toggle_rate(filtered)
    mae_raw = float(np.abs(raw - truth)[raw != -1].mean())
    mae_f = float(np.abs(filtered - truth)[filtered != -1].mean())
    print(f"temporal std raw {s_raw:.4f} filtered {s_f:.4f}; toggles {t_raw:.4f} -> {t_f:.4f}; MAE {mae_raw:.4f} -> "
          f"{mae_f:.4f}")
    assert s_f < 0.7 * s_raw
    assert t_f < t_raw
    assert mae_f <= mae_raw


def test_moved_pixels_pass_the_measurement_through():
    frames, truth = _jitter_maps(4)
    filt = ref.TemporalRef(truth.shape)
    for d, g in frames:
        filt.apply(d, g)
    d, g = frames[-1]
    moved = np.roll(g, 5, axis=1)                                         # the texture shifted by 5 px
    prev = filt.G.copy()
    out = filt.apply(d, moved)
    still = ref.static_mask(moved, prev)
    assert (~still).mean() > 0.5, "the shift must move most of the image"
    valid = np.isfinite(d) & (d != -1.0)
    m = ~still & valid
    assert np.array_equal(_bits(out[m]), _bits(d[m]))
    assert np.all(out[~still & ~valid] == -1.0)


def test_synthetic_sequences():
    st = seqs.static_sequence(3, 40, 90, 32, 2, seed=5)
    assert len(st) == 3 and all(f[0].dtype == np.float32 and f[0].shape == (40, 90) for f in st)
    assert np.array_equal(st[0][2], st[2][2]) and not np.array_equal(st[0][0], st[1][0])
    assert np.all(np.abs(st[0][0] - st[1][0]) <= 4)
    mv = seqs.moving_sequence(3, 40, 96, 32, 2, seed=5, step=3)
    d_obj = np.float32(int(31 * 0.7))                                     # rows 5..14, 12 px wide, from column 48
    assert np.all(mv[0][2][5:15, 48:60] == d_obj) and np.all(mv[1][2][5:15, 51:63] == d_obj)
    assert np.all(mv[1][2][5:15, 48:51] != d_obj)
    assert np.all(np.abs(mv[1][0][5:15, 51:63] - mv[0][0][5:15, 48:60]) <= 4), "the texture moves with the object"


# ----------------------------------------------------------------------------- Python and pipeline checks
DEFAULTS = (("motion_radius", 1), ("motion_threshold", 4.0), ("decay", 0.8), ("max_diff", 1.0), ("max_weight", 8.0),
            ("min_weight", 0.25))
BAD = ((dict(motion_radius=-1), "motion_radius must be in 0..7"), (dict(motion_radius=8), "motion_radius must be in 0..7"),
       (dict(motion_threshold=-0.5), "motion_threshold must be finite and >= 0"),
       (dict(motion_threshold=INF), "motion_threshold must be finite and >= 0"),
       (dict(decay=0.0), r"decay must be in \(0, 1\]"), (dict(decay=1.5), r"decay must be in \(0, 1\]"),
       (dict(decay=NAN), "decay must be in"), (dict(max_diff=-1.0), "max_diff must be finite and >= 0"),
       (dict(max_diff=NAN), "max_diff"), (dict(max_weight=0.0), "max_weight must be finite and > 0"),
       (dict(max_weight=INF), "max_weight"), (dict(min_weight=-1e-3), "min_weight must be finite and >= 0"),
       (dict(min_weight=NAN), "min_weight"), (dict(invalid_disparity=NAN), "invalid_disparity must be finite"))


def test_python_class_defaults_and_validation():
    import cuda_depth
    p = inspect.signature(cuda_depth.TemporalFilter.__init__).parameters
    for name, default in DEFAULTS + (("invalid_disparity", -1.0), ("device", None)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert p[name].default == default and type(p[name].default) is type(default), name
    a = inspect.signature(cuda_depth.TemporalFilter.apply).parameters
    assert [a[k].default for k in ("confidence", "out")] == [None, None]
    assert inspect.signature(cuda_depth.TemporalFilter.reset).parameters["streams"].default is None
    for kw, msg in BAD:                                                   # checked before any device is touched
        with pytest.raises(RuntimeError, match=msg):
            cuda_depth.TemporalFilter(1, 8, 8, **kw)
    with pytest.raises(TypeError, match="motion_radius must be an int"):
        cuda_depth.TemporalFilter(1, 8, 8, motion_radius=1.0)
    with pytest.raises(TypeError, match="decay must be a number"):
        cuda_depth.TemporalFilter(1, 8, 8, decay=True)
    with pytest.raises(TypeError, match="n must be an int"):
        cuda_depth.TemporalFilter(1.0, 8, 8)
    for dims in ((0, 8, 8), (1, 0, 8), (1, 8, 32769)):
        with pytest.raises(RuntimeError, match="need n >= 1"):
            cuda_depth.TemporalFilter(*dims)
    with pytest.raises(RuntimeError, match="needs a GPU device"):
        cuda_depth.TemporalFilter(1, 8, 8, device="cpu")


def test_backend_and_pipeline_keywords_and_defaults():
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig, DepthEstimationResult
    from pipeline.depth import CudaStereoMatchingBackend, SgmStereoMatchingBackend
    for cls in (CudaStereoMatchingBackend, SgmStereoMatchingBackend, DepthEstimationPipeline):
        p = inspect.signature(cls.__init__).parameters
        for name, default in (("temporal", False),) + tuple(("temporal_" + k, v) for k, v in DEFAULTS):
            assert name in p, (cls, name)
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY, (cls, name)
            assert p[name].default == default and type(p[name].default) is type(default), (cls, name)
    assert callable(DepthEstimationPipeline.reset_temporal)
    assert not any("temporal" in f for f in DepthEstimationPipelineConfig.__dataclass_fields__)
    assert list(DepthEstimationResult.__dataclass_fields__)[-1] == "confidence_map"


def test_pipeline_keyword_validation():
    from pipeline.depth.map_postprocessing import MapPostprocessing
    m = MapPostprocessing()
    with pytest.raises(TypeError, match="temporal must be a bool"):
        m._init_postprocessing((8, 8), temporal=1)
    for kw, msg in BAD[:-1]:
        kw = {"temporal_" + k: v for k, v in kw.items()}
        with pytest.raises(RuntimeError, match=msg):
            m._init_postprocessing((8, 8), **kw)                          # checked even when off
        with pytest.raises(RuntimeError, match=msg):
            m._init_postprocessing((8, 8), temporal=True, **kw)
    m._init_postprocessing((8, 8))
    assert not m._uses_guide()
    m.reset_temporal()                                                    # nothing to forget yet
    m._init_postprocessing((8, 8), temporal=True)
    assert m._uses_guide()                                                # the filter reads the left gray plane


# ----------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from cuda_depth import _native
    return _native


def test_the_symbol_is_declared_listed_and_exported(native):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stereo_mi355x.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+smx_temporal_filter\s*\(", header)
    assert "smx_temporal_filter" in native.EXPORTS
    assert hasattr(C.CDLL(native.LIB_PATH), "smx_temporal_filter")
    assert native.LIB.smx_abi_version() == 4


# fake device pointers: never dereferenced, every check returns first
DISP, CONF, GUIDE, PREV, SD, SW, GOUT, OUT = (k * 0x100000 for k in range(1, 9))
MAP_BYTES = 2 * 4 * 4 * 4                                      # n = 2, H = W = 4


def _call(native, **change):
    a = dict(dev=0, n=2, H=4, W=4, d=DISP, c=CONF, g=GUIDE, G=PREV, D=SD, A=SW, go=GOUT, o=OUT, R=1, thr=4.0,
             decay=0.8, md=1.0, maxw=8.0, minw=0.25, inv=-1.0, s=None)
    a.update(change)
    return native.LIB.smx_temporal_filter(*a.values())


REJECTIONS = [
    (dict(d=None), "must be non-NULL"),
    (dict(g=None), "must be non-NULL"),
    (dict(G=None), "must be non-NULL"),
    (dict(D=None), "must be non-NULL"),
    (dict(A=None), "must be non-NULL"),
    (dict(o=None), "must be non-NULL"),
    (dict(n=0), "need n >= 1"),
    (dict(H=0), "1 <= H, W <= 32768"),
    (dict(W=32769), "1 <= H, W <= 32768"),
    (dict(R=-1), "motion_radius must be in 0..7"),
    (dict(R=8), "motion_radius must be in 0..7"),
    (dict(thr=-1.0), "motion_threshold must be finite and >= 0"),
    (dict(thr=NAN), "motion_threshold must be finite and >= 0"),
    (dict(thr=INF), "motion_threshold must be finite and >= 0"),
    (dict(decay=0.0), "decay must be in (0, 1]"),
    (dict(decay=-0.5), "decay must be in (0, 1]"),
    (dict(decay=1.0001), "decay must be in (0, 1]"),
    (dict(decay=NAN), "decay must be in (0, 1]"),
    (dict(md=-0.1), "max_diff must be finite and >= 0"),
    (dict(md=INF), "max_diff must be finite and >= 0"),
    (dict(maxw=0.0), "max_weight must be finite and > 0"),
    (dict(maxw=INF), "max_weight must be finite and > 0"),
    (dict(maxw=NAN), "max_weight must be finite and > 0"),
    (dict(minw=-1.0), "min_weight must be finite and >= 0"),
    (dict(minw=NAN), "min_weight must be finite and >= 0"),
    (dict(inv=NAN), "invalid_disparity must be finite"),
    (dict(inv=INF), "invalid_disparity must be finite"),
    # out: exactly disp or disjoint from it; disjoint from everything else
    (dict(o=DISP + 4), "out must not overlap disp other than as the same buffer"),
    (dict(o=DISP - MAP_BYTES + 4), "out must not overlap disp other than as the same buffer"),
    (dict(o=CONF), "out must not overlap an operand other than disp"),
    (dict(o=GUIDE + 8), "out must not overlap an operand other than disp"),
    (dict(o=PREV - 8), "out must not overlap an operand other than disp"),
    (dict(o=SD), "out must not overlap an operand other than disp"),
    (dict(o=SW + MAP_BYTES - 4), "out must not overlap an operand other than disp"),
    (dict(o=GOUT), "out must not overlap an operand other than disp"),
    # the state: disjoint from the inputs and from each other
    (dict(D=DISP), "the state buffers must not overlap an input"),
    (dict(D=CONF + 4), "the state buffers must not overlap an input"),
    (dict(A=GUIDE), "the state buffers must not overlap an input"),
    (dict(A=PREV + MAP_BYTES - 4), "the state buffers must not overlap an input"),
    (dict(A=SD + 4), "state_disp and state_weight overlap"),
    (dict(A=SD), "state_disp and state_weight overlap"),
    # guide_out: disjoint from guide, prev_guide and everything else
    (dict(go=GUIDE), "guide_out must not overlap another operand"),
    (dict(go=PREV + 4), "guide_out must not overlap another operand"),
    (dict(go=DISP), "guide_out must not overlap another operand"),
    (dict(go=CONF - 4), "guide_out must not overlap another operand"),
    (dict(go=SD), "guide_out must not overlap another operand"),
    (dict(go=SW + 8), "guide_out must not overlap another operand"),
    (dict(s=-1), "needs a caller stream"),
]


@pytest.mark.parametrize("change,msg", REJECTIONS, ids=[f"{i}" for i in range(len(REJECTIONS))])
def test_temporal_filter_rejects_bad_arguments_without_a_device(native, change, msg):
    if change.get("s") == -1:
        change = dict(change, s=native.STREAM_ENGINE)
    assert _call(native, **change) == -1, change
    assert msg in native.last_error(), (change, msg, native.last_error())


def test_accepted_arguments_reach_the_stream_check(native):
    """NULL confidence or guide_out, out = disp, inputs aliasing each other, operands right behind each other and the
    parameter bounds pass every check (the engine-stream sentinel then stops the call before the device)."""
    for change in (dict(c=None), dict(go=None), dict(c=None, go=None), dict(o=DISP), dict(c=DISP, g=DISP, G=DISP),
                   dict(g=PREV), dict(o=DISP + MAP_BYTES), dict(D=OUT + MAP_BYTES, A=OUT + 2 * MAP_BYTES),
                   dict(R=0), dict(R=7), dict(thr=0.0, decay=1.0, md=0.0, minw=0.0, maxw=1e-30),
                   dict(decay=1e-30, thr=3e38, md=3e38, maxw=3e38, minw=3e38, inv=0.0),
                   dict(n=1, H=32768, W=32768, d=1 << 40, c=2 << 40, g=3 << 40, G=4 << 40, D=5 << 40, A=6 << 40,
                        go=7 << 40, o=8 << 40)):
        rc = _call(native, s=native.STREAM_ENGINE, **change)
        assert rc == -1 and "needs a caller stream" in native.last_error(), (change, native.last_error())
