"""DepthEstimationPipeline.process() end to end against the CPU reference chain (pipeline_ref.PipelineRef), bit for bit:
the disparity map, the confidence map and, with a rectification, the rectified frames, after every frame of a short
sequence through one pipeline object.

The cases are a pairwise covering set of the factors below, generated deterministically (pairwise_cases); the test
test_every_pair_of_levels_is_covered checks it over CASES.  Each case runs
  1. two frames of static_sequence (fresh +-2 noise each, so the temporal history matters),
  2. one frame of moving_sequence (the moving object),
  3. reset_temporal(),
  4. the same moving_sequence frame generated with another noise seed (any history the reset left shows in the map).
Two full-size cases (375 x 1242, one per backend, LR check, speckles, confidence, WLS and temporal filter) run two frames
of static_sequence."""
import itertools

import numpy as np
import pytest

import rectify_ref
import stereo_sequences as seqs
import stereo_synthetic as syn
from pairwise import pairwise_cases
from pipeline_ref import PipelineRef

torch = pytest.importorskip("torch")

FACTORS = {
    "backend": ["cuda", "sgm"],
    "frames": ["u8", "f32", "mixed"],
    "lr": [False, True],
    "speckle": [0, 12],
    "filter": ["none", "fill", "median", "fill+median", "wls1", "wls3"],
    "confidence": ["off", "r0", "r2"],
    "rect": [False, True],
    "temporal": [False, True],
    "inv": [-1.0, 0.0, -7.5],
    "shape": ["48x120", "37x91"],
}
SHAPES = {"48x120": (48, 120, 0, 31), "37x91": (37, 91, 5, 28)}           # H, W, min_disparity, max_disparity
FILTERS = {"none": {}, "fill": dict(fill_invalid=True), "median": dict(median_radius=3),
           "fill+median": dict(fill_invalid=True, median_radius=2), "wls1": dict(wls_lambda=200.0, wls_iterations=1),
           "wls3": dict(wls_lambda=200.0, wls_iterations=3)}
CONFIDENCE = {"off": {}, "r0": dict(confidence=True, confidence_radius=0),
              "r2": dict(confidence=True, confidence_radius=2)}
TEMPORAL = dict(temporal_motion_radius=1, temporal_motion_threshold=4.0, temporal_decay=0.75, temporal_max_diff=1.0,
                temporal_max_weight=6.0, temporal_min_weight=0.25)


def _pairs(case):
    names = list(FACTORS)
    return {(a, case[a], b, case[b]) for i, a in enumerate(names) for b in names[i + 1:]}


CASES = pairwise_cases(FACTORS)


def _case_id(c):
    return "-".join([c["backend"], c["frames"], "lr" if c["lr"] else "nolr", f"sp{c['speckle']}", c["filter"],
                     f"conf_{c['confidence']}", "rect" if c["rect"] else "norect", "tf" if c["temporal"] else "notf",
                     f"inv{c['inv']:g}", c["shape"]])


def test_every_pair_of_levels_is_covered():
    covered = set().union(*(_pairs(c) for c in CASES))
    names = list(FACTORS)
    for x, a in enumerate(names):
        for b in names[x + 1:]:
            for la, lb in itertools.product(FACTORS[a], FACTORS[b]):
                assert (a, la, b, lb) in covered, (a, la, b, lb)
    assert len({_case_id(c) for c in CASES}) == len(CASES)


# ----------------------------------------------------------------------------- GPU side
@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def bits(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bitwise(got, expect, what):
    g, e = bits(got), bits(expect)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    bad = np.argwhere(g != e)
    assert bad.size == 0, f"{what}: {len(bad)} pixels differ, first at {tuple(bad[0])}: " \
                          f"{g.view(np.float32)[tuple(bad[0])]} vs {e.view(np.float32)[tuple(bad[0])]}"


def assert_frame(got, expect, what):
    got = got.cpu().numpy()
    assert got.dtype == expect.dtype, (what, got.dtype, expect.dtype)
    if expect.dtype == np.uint8:
        assert np.array_equal(got, expect), what
    else:
        assert_bitwise(got, expect, what)


def _qmap(H, W, Hi, Wi, seed, shift=0):
    """A smooth int32 map of 1/32-pixel raw coordinates, slightly rotated and scaled (rectify_ref's format); `shift`
    columns to the right."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a, s = rng.uniform(-0.01, 0.01), rng.uniform(0.97, 1.0)
    mx = s * (np.cos(a) * u - np.sin(a) * v) + rng.uniform(1, 3) + shift
    my = s * (np.sin(a) * u + np.cos(a) * v) + rng.uniform(1, 3)
    return rectify_ref.quantize_map(mx, my, (Hi, Wi))


def _cast(kind, left, right, f=0):
    """[H, W] gray views -> [3, H, W] frames of the case's dtype(s); mixed: the uint8 frame is the left one on even
    frames f and the right one on odd frames (the fallback to float32 for both, either way round)."""
    L, R = syn.gray_to_rgb(left), syn.gray_to_rgb(right)
    if kind == "u8":
        return L.astype(np.uint8), R.astype(np.uint8)
    if kind == "f32":
        return L, R
    return (L.astype(np.uint8), R) if f % 2 == 0 else (L, R.astype(np.uint8))


def _build(cd, oracle, backend, H, W, dmin, dmax, inv, lr, rect=None, **post):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=dmin, max_disparity=dmax,
                                        invalid_disparity=inv, stereo_matching_backend=backend, left_right_check=lr,
                                        lr_max_diff=1.0)
    rectification = None if rect is None else cd.StereoRectification(rect[0], rect[1], rect[2], (H, W))
    pipe = DepthEstimationPipeline(cfg, rectification=rectification, **post)
    ref = PipelineRef((H, W), dmin, dmax, inv, backend, lr, 1.0, oracle=oracle, rectification=rect, **post)
    return pipe, ref


def _check_frame(pipe, ref, L, R, what):
    res = pipe.process(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())
    got_d = res.disparity_map.clone()                               # persistent buffers: copy before the next frame
    got_c = None if res.confidence_map is None else res.confidence_map.clone()
    got_l, got_r = res.left_image.clone(), res.right_image.clone()
    d, c, rl, rr = ref.process(L, R)
    assert_bitwise(got_d, d, f"{what}: disparity")
    if c is None:
        assert got_c is None, what
    else:
        assert got_c is not None, what
        assert_bitwise(got_c, c, f"{what}: confidence")
    if rl is not None:
        assert_frame(got_l, rl, f"{what}: rectified left")
        assert_frame(got_r, rr, f"{what}: rectified right")
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_pipeline_matches_the_reference_chain(cd, oracle_omp, case):
    H, W, dmin, dmax = SHAPES[case["shape"]]
    inv = case["inv"]
    rect = None
    h, w = H, W
    if case["rect"]:
        h, w = H + 6, W + 10                                        # raw frames
        rect = (_qmap(H, W, h, w, 1, shift=10), _qmap(H, W, h, w, 2), (h, w))
    post = dict(speckle_max_size=case["speckle"], speckle_max_diff=1.0, **FILTERS[case["filter"]],
                **CONFIDENCE[case["confidence"]])
    if case["temporal"]:
        post.update(temporal=True, **TEMPORAL)
    pipe, ref = _build(cd, oracle_omp, case["backend"], H, W, dmin, dmax, inv, case["lr"], rect, **post)
    index = CASES.index(case)
    D = dmax + 1
    frames = [l_r[:2] for l_r in seqs.static_sequence(2, h, w, D, 2, index=index % 5, seed=100 + index)]
    moving = seqs.moving_sequence(1, h, w, D, 2, index=index % 5, seed=200 + index, step=3)[0][:2]
    again = seqs.moving_sequence(1, h, w, D, 2, index=index % 5, seed=300 + index, step=3)[0][:2]
    maps = []
    for f, (l, r) in enumerate(frames + [moving]):
        maps.append(_check_frame(pipe, ref, *_cast(case["frames"], l, r, f), f"frame {f}"))
    pipe.reset_temporal()
    ref.reset_temporal()
    maps.append(_check_frame(pipe, ref, *_cast(case["frames"], *again, 3), "frame after reset_temporal()"))
    valid = [np.isfinite(m) & (m != np.float32(inv)) for m in maps]
    assert all(v.any() for v in valid), "every frame has valid pixels"


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["cuda", "sgm"])
def test_full_size_chain(cd, oracle_omp, backend):
    """A KITTI-sized (C2) pair, 64 candidates, with the LR check, speckles, confidence, WLS and temporal filter, two frames
    through one pipeline."""
    H, W, dmin, dmax, inv = 375, 1242, 0, 63, -1.0
    post = dict(speckle_max_size=12, confidence=True, confidence_radius=2, wls_lambda=8000.0, wls_iterations=3,
                temporal=True, **TEMPORAL)
    pipe, ref = _build(cd, oracle_omp, backend, H, W, dmin, dmax, inv, True, **post)
    for f, (l, r, _) in enumerate(seqs.static_sequence(2, H, W, dmax + 1, 2, index=0, seed=7)):
        _check_frame(pipe, ref, *_cast("u8", l, r), f"{backend} C2 frame {f}")
