"""The NumPy twin of smx_intensity_pyramid and smx_track_camera_pyramid (tests/track_pyramid_ref.py) against what the
header promises, without a GPU: the pyramid's dimensions, clamping and NaN footprints; with every level 0 and
huber_delta = inf the tracker is the photometric twin bit for bit; a residual of exactly huber_delta weighs 1; and the
wall of tests/track_pyramid_cases.py, the case the pyramid is for: from a start eight pixels off the pyramid twin ends
below a tenth of the start error while the photometric twin stays above half of it."""
import numpy as np
import pytest

import track_cases as tc
import track_photo_cases as pc
import track_pyramid_cases as yc
import track_pyramid_ref as ty
import track_ref as tr

f32 = np.float32


@pytest.mark.parametrize("shape", yc.PYRAMID_SHAPES)
def test_level_dimensions_are_the_selected_grids(shape):
    H, W = shape
    pyr = yc.pyramid_expected(1, shape, 8)
    for l, p in enumerate(pyr):
        assert p.shape == (1, len(range(0, H, 1 << l)), len(range(0, W, 1 << l))) and p.dtype == np.float32
    assert ty.level_dims(H, W, 8) == [p.shape[1:] for p in pyr]
    assert pyr[7].shape[1:] == ((H + 127) // 128, (W + 127) // 128)
    flat = ty.flat(pyr)
    assert flat.size == sum(p.size for p in pyr) and yc.same_planes(flat[:H * W].reshape(1, H, W), pyr[0])


def test_the_reduce_weights_clamps_and_spreads_nans():
    # powers of two pass through the taps exactly; a constant plane stays constant at every level
    for shape in ((1, 1), (5, 1), (2, 3), (9, 14)):
        for p in ty.intensity_pyramid_ref(np.full(shape, 64.0, f32), 4):
            assert (p == 64.0).all()
    # impulses of 256: a level pixel sits on (2 x, 2 y), so an even place meets the taps 1 6 1 and an odd one 4 4
    a = np.zeros((9, 11), f32)
    a[4, 6] = 256.0
    want = np.zeros((5, 6), f32)
    want[1:4, 2:5] = np.outer([1, 6, 1], [1, 6, 1])
    assert np.array_equal(ty.reduce_ref(a), want)
    a = np.zeros((9, 11), f32)
    a[3, 6] = 256.0
    want = np.zeros((5, 6), f32)
    want[1:3, 2:5] = np.outer([4, 4], [1, 6, 1])
    assert np.array_equal(ty.reduce_ref(a), want)
    # clamping: the first column repeats to the left, so an impulse there weighs 1 + 4 + 6 of 16
    b = np.zeros((1, 8), f32)
    b[0, 0] = 16.0
    assert ty.reduce_ref(b)[0].tolist() == [11.0, 1.0, 0.0, 0.0]
    # a NaN spoils exactly the pixels whose 5 x 5 footprint holds it; the mask makes NaNs at level 0
    c = np.ones((12, 12), f32)
    c[5, 6] = np.nan
    bad = np.isnan(ty.reduce_ref(c))
    assert bad.sum() == 6 and bad[2:4, 2:5].all()
    z = np.full((4, 4), 2.0, f32)
    z[0, :] = (0.0, -1.0, np.inf, np.nan)
    lvl0 = ty.intensity_pyramid_ref(np.ones((4, 4), f32), 2, z)[0]
    assert np.isnan(lvl0[0]).all() and (lvl0[1:] == 1.0).all()


def test_default_levels():
    assert ty.default_levels(tr.DEFAULT_SCHEDULE, 3) == (2, 1, 0)
    assert ty.default_levels(((8, 1), (6, 1), (4, 1), (3, 1)), 3) == (2, 1, 2, 0)
    assert ty.default_levels(((8, 1), (4, 1)), 1) == (0, 0)


TRIPLES = [("outside", tc.FRAME_SHAPES[0], 0, False, False), ("left", tc.FRAME_SHAPES[0], 1, True, False),
           ("left", tc.FRAME_SHAPES[1], 1, False, True), ("outside", tc.FRAME_SHAPES[1], 0, True, False)]


@pytest.mark.parametrize("triple", TRIPLES)
def test_level_0_without_huber_is_the_photometric_twin(triple):
    v, s, k, c, m = triple
    got = yc.expected(v, s, k, c, m, schedule=tr.DEFAULT_SCHEDULE, schedule_levels=(0, 0, 0), levels=1)
    pc.assert_same(got, pc.expected(v, s, k, c, m), str(triple))
    deep = yc.expected(v, s, k, c, m, schedule=tr.DEFAULT_SCHEDULE, schedule_levels=(0, 0, 0), levels=3)
    pc.assert_same(deep, got, "the levels above are not read")


def test_the_levels_and_hubers_weight_take_part():
    v, s = "outside", tc.FRAME_SHAPES[0]
    plain = yc.expected(v, s, schedule_levels=(0, 0, 0))
    coarse = yc.expected(v, s)
    robust = yc.expected(v, s, huber_delta=yc.HUBER)
    assert coarse["info"][0] == 0 and robust["info"][0] == 0
    assert not np.array_equal(plain["pose"], coarse["pose"]) and not np.array_equal(coarse["pose"], robust["pose"])
    assert robust["sums"][31] < coarse["sums"][31]                  # some residual is past delta


def test_a_residual_of_exactly_delta_weighs_one():
    off = yc.huber_expected(np.inf)
    at = yc.huber_expected(3.0)
    past = yc.huber_expected(2.0)
    assert off["pinfo"].tolist() == [1, 0] and off["sums"][30] == 9.0 and off["sums"][31] == 1.0   # e = 3 exactly
    yc.assert_same(at, off, "|e| == huber_delta")
    assert past["sums"][31] == float(f32(2.0) / f32(3.0)) and past["sums"][30] == float((f32(2.0) / f32(3.0) * f32(3.0)) * f32(3.0))


def test_the_wall_is_tracked_from_eight_pixels_off_by_the_pyramid_only():
    """The conditions on the references that make the wall worth running on the device."""
    geo, photo, pyramid = yc.wall_expected()
    start, plain, coarse = yc.wall_errors()
    print(f"wall, start {yc.WALL_START_PX} px: {start[0]:.4f} m {start[1]:.2f} deg; photometric twin {plain[0]:.4f} m "
          f"{plain[1]:.2f} deg; pyramid twin {coarse[0]:.4f} m {coarse[1]:.2f} deg")
    assert geo["info"][0] == 1, "the geometric tracker loses a plane"
    assert photo["info"][0] == 0 and pyramid["info"][0] == 0
    assert coarse[0] < 0.1 * start[0]
    assert plain[0] > 0.5 * start[0]
    assert coarse[1] < 0.5 * start[1]
