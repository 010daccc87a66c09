"""The layout rule of the pooled planes in grid units and the staging by four-column groups, modelled in NumPy
(unit_planes_ref.py): what k_prologue.h writes and k_match_fast.h: fast_stage_units reads."""
import numpy as np
import pytest

import unit_planes_ref as up

WIDTHS = list(range(1, 41)) + [42, 43, 100, 168, 169, 170, 171, 172, 190, 621]


@pytest.mark.parametrize("w", WIDTHS)
def test_pitch_and_apron(w):
    pitch = up.unit_plane_pitch(w)
    assert pitch % 4 == 0 and w + 3 <= pitch < w + 3 + 4
    assert pitch == -(-(w + 3) // 4) * 4                     # round_up(w + 3, 4)
    rng = np.random.default_rng(w)
    pooled = rng.integers(0, 255 * 4 + 1, (5, w)).astype(np.float32) / np.float32(4)      # the K = 2 grid
    plane = up.unit_plane(pooled, 4)
    assert plane.shape == (5, pitch)
    assert np.array_equal(plane[:, :w].astype(np.float32), pooled * 4)
    if w >= 3:
        assert np.array_equal(plane[:, w:w + 3], plane[:, 0:3])
    for j in range(3):
        assert np.array_equal(plane[:, w + j], plane[:, j % w])
    # every 4-column group that starts in [0, w) lies inside the row and reads the cyclic continuation
    for c in range(w):
        assert c + 4 <= pitch
        assert np.array_equal(plane[:, c:c + 4], plane[:, :w][:, (c + np.arange(4)) % w])


@pytest.mark.parametrize("unit", [1, 4, 16, 64])
def test_unit_values_on_and_off_the_grid(unit):
    grid = np.arange(0, 255 * unit + 1, dtype=np.float32) / np.float32(unit)
    got = up.unit_value(grid, unit)
    assert np.array_equal(got, np.arange(0, 255 * unit + 1)) and int(got.max()) == 255 * unit <= 16320
    off = np.float32([0.3, 17.3, 254.99, 255.0 + 0.3])       # a caller who forces FAST_GRID: truncation, as the f32 staging did
    assert np.array_equal(up.unit_value(off, unit), np.trunc(np.float32(unit) * off).astype(np.uint16))


@pytest.mark.parametrize("w,h", [(1, 3), (2, 5), (3, 4), (5, 9), (40, 30), (169, 49), (171, 53), (190, 24)])
@pytest.mark.parametrize("cols", [64, 190, 194, 253, 256, 257, 320])
def test_staged_tile_equals_the_cyclic_gather(w, h, cols):
    rng = np.random.default_rng(1000 * w + cols)
    pooled = rng.integers(0, 256, (h, w)).astype(np.float32)
    plane = up.unit_plane(pooled, 1)
    units = plane[:, :w]
    for row0, col0 in ((-11, -11), (h - 3, -11 - 130), (13, 168 - 11 - 66), (0, 3 * w + 2), (-11, -11 - 99)):
        tile = up.stage_tile(plane, w, row0, col0, 30, cols)
        assert tile.shape[1] % 4 == 0 and cols <= tile.shape[1] < cols + 4
        # columns past `cols` receive what was loaded; the marches never read them
        assert np.array_equal(tile[:, :cols], up.gather_tile(units, row0, col0, 30, cols))


def test_tile_pitches_hold_the_rounded_up_rows():
    """k_match_fast.h: the left tile (190 or 64 columns at pitch 192) and the right tiles (pitch 256 / 288 / 320, columns up to
    the pitch) are written in whole groups of four: the pitches are multiples of 8 and at least the rounded-up column count."""
    for pitch, cols in ((192, 190), (192, 64), (256, 256), (256, 190 + 66), (288, 190 + 98), (320, 190 + 130), (320, 64 + 256)):
        assert pitch % 8 == 0 and ((cols + 3) & ~3) <= pitch
