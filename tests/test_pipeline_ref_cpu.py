"""CPU tests of the reference chain of DepthEstimationPipeline.process() (pipeline_ref.PipelineRef) itself, on frames a few
dozen pixels wide: with every option off it is the matcher's reference, the rectification's mask reaches the map and the
confidence, filled pixels carry no confidence, the temporal filter's first frame is the chain without it, and the
combinations the pipeline refuses are refused."""
import numpy as np
import pytest

import rectify_ref
import sgm_ref
import stereo_sequences as seqs
import stereo_synthetic as syn
from median_ref import valid_mask
from oracle_lib import OracleConfig
from pipeline_ref import PipelineRef

H, W, DMAX = 24, 56, 15
Hi, Wi = 30, 66                                     # raw frames of the rectification cases
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frames(count, h, w, seed, u8=False):
    seq = seqs.static_sequence(count, h, w, DMAX + 1, 2, index=1, seed=seed)
    cast = (lambda a: a.astype(np.uint8)) if u8 else (lambda a: a)
    return [(cast(syn.gray_to_rgb(l)), cast(syn.gray_to_rgb(r))) for l, r, _ in seq]


def _qmap(seed, shift):
    """A slightly rotated and scaled map; `shift` columns to the right so that the left view's right columns reach past
    the raw frame."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a, s = rng.uniform(-0.01, 0.01), rng.uniform(0.97, 1.0)
    mx = s * (np.cos(a) * u - np.sin(a) * v) + rng.uniform(1, 3) + shift
    my = s * (np.sin(a) * u + np.cos(a) * v) + rng.uniform(1, 3)
    return rectify_ref.quantize_map(mx, my, (Hi, Wi))


def _rect():
    return _qmap(1, 10), _qmap(2, 0), (Hi, Wi)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("backend", ["cuda", "sgm"])
def test_every_option_off_is_the_matcher_reference(oracle, backend, u8):
    dmin = 2
    ref = PipelineRef((H, W), dmin, DMAX, -1.0, backend, oracle=oracle)
    for L, R in _frames(2, H, W, 5, u8):
        d, conf, rl, rr = ref.process(L, R)
        assert conf is None and rl is None and rr is None
        if backend == "cuda":
            want = oracle.run(OracleConfig(height=H, width=W, downscale_factor=2, min_disparity=dmin,
                                           max_disparity=DMAX), L.astype(F), R.astype(F))
        else:
            want, _ = sgm_ref.sgm_ref(L, R, dmin, DMAX - dmin + 1)
        assert np.array_equal(_bits(d), _bits(want))


def test_mixed_dtypes_are_matched_as_float32(oracle):
    """One uint8 and one float32 frame: both are taken as float32, so the rectified frames are float32 too."""
    (L, R), = _frames(1, Hi, Wi, 7, u8=True)
    ref = PipelineRef((H, W), 0, DMAX, -1.0, "sgm", rectification=_rect())
    d, _, rl, rr = ref.process(L, R.astype(F))
    assert rl.dtype == rr.dtype == np.float32
    ref_u8 = PipelineRef((H, W), 0, DMAX, -1.0, "sgm", rectification=_rect())
    _, _, rl8, _ = ref_u8.process(L, R)
    assert rl8.dtype == np.uint8
    assert not np.array_equal(rl, rl8.astype(F))                     # the float remap keeps the fractions


@pytest.mark.parametrize("temporal", [False, True])
@pytest.mark.parametrize("backend", ["cuda", "sgm"])
def test_outside_left_valid_is_invalid_with_zero_confidence(oracle, backend, temporal):
    inv = -7.5
    qL, qR, in_shape = _rect()
    outside = ~rectify_ref.valid_mask(qL, in_shape)
    assert 0 < outside.mean() < 0.5
    ref = PipelineRef((H, W), 0, DMAX, inv, backend, True, oracle=oracle, speckle_max_size=4, fill_invalid=True,
                      confidence=True, confidence_radius=1, temporal=temporal, rectification=(qL, qR, in_shape))
    for L, R in _frames(3, Hi, Wi, 11, u8=True):
        d, conf, rl, rr = ref.process(L, R)
        assert rl.shape == rr.shape == (3, H, W)
        assert (d[outside] == F(inv)).all()
        assert (conf[outside] == 0).all()
        assert (conf[~outside] > 0).any()
        assert valid_mask(d[~outside], inv).mean() > 0.5             # the fill made the inside dense


@pytest.mark.parametrize("backend", ["cuda", "sgm"])
@pytest.mark.parametrize("filt", [dict(fill_invalid=True), dict(fill_invalid=True, median_radius=2),
                                  dict(wls_lambda=50.0, wls_iterations=2)])
def test_filled_pixels_have_zero_confidence(oracle, backend, filt):
    inv = 0.0
    common = dict(oracle=oracle, speckle_max_size=12, confidence=True, confidence_radius=2)
    base = PipelineRef((H, W), 0, DMAX, inv, backend, True, **common)
    ref = PipelineRef((H, W), 0, DMAX, inv, backend, True, **common, **filt)
    for L, R in _frames(2, H, W, 13):
        d0, c0, _, _ = base.process(L, R)
        d, c, _, _ = ref.process(L, R)
        assert np.array_equal(_bits(c), _bits(c0)), "the confidence is taken before the fill and the filters"
        written = ~valid_mask(d0, inv) & valid_mask(d, inv)
        assert written.any()
        assert (c[written] == 0).all()
        assert (c[valid_mask(d0, inv)] > 0).any()


@pytest.mark.parametrize("confidence", [False, True])
@pytest.mark.parametrize("backend", ["cuda", "sgm"])
def test_first_temporal_frame_is_the_chain_without_it(oracle, backend, confidence):
    inv = -1.0
    common = dict(oracle=oracle, speckle_max_size=12, confidence=confidence, median_radius=1)
    plain = PipelineRef((H, W), 0, DMAX, inv, backend, True, **common)
    ref = PipelineRef((H, W), 0, DMAX, inv, backend, True, temporal=True, **common)
    frames = _frames(3, H, W, 17)
    for i, (L, R) in enumerate(frames + frames[:1]):
        if i == 3:
            ref.reset_temporal()
        base, _, _, _ = plain.process(L, R)
        d, _, _, _ = ref.process(L, R)
        if i in (0, 3):                                              # after construction / after reset_temporal()
            ok = valid_mask(base, inv)
            assert np.array_equal(_bits(d[ok]), _bits(base[ok]))
            assert (d[~ok] == F(inv)).all()
        elif i == 2:
            assert not np.array_equal(_bits(d), _bits(base)), "the history is carried across calls"


def test_refused_combinations(oracle):
    for bad in (dict(wls_lambda=10.0, fill_invalid=True), dict(wls_lambda=10.0, median_radius=2),
                dict(wls_lambda=10.0, fill_invalid=True, median_radius=1)):
        for backend in ("cuda", "sgm"):
            with pytest.raises(ValueError, match="wls_lambda"):
                PipelineRef((H, W), 0, DMAX, -1.0, backend, oracle=oracle, **bad)
    PipelineRef((H, W), 0, DMAX, -1.0, "sgm", fill_invalid=True, median_radius=2)       # allowed without WLS
