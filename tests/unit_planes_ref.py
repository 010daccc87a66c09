"""NumPy model of the pooled planes in grid units (smx_common.h: unit_plane_pitch, MatchParams::Lu / Ru) and of the way the
fast kernels stage a tile from them (k_match_fast.h: fast_stage_units)."""
import numpy as np


def unit_plane_pitch(w):
    """Row pitch in u16 elements: w columns, a cyclic apron of three, rounded up to a multiple of 4 (8-byte rows)."""
    return (w + 3 + 3) & ~3


def unit_value(pooled, unit):
    """(unsigned short)(unit * pooled) in float32: the conversion truncates towards zero; the model covers [0, 65536)."""
    s = np.float32(unit) * np.asarray(pooled, np.float32)
    assert np.all((s >= 0) & (s < 65536)), "outside the model (the device conversion saturates there)"
    return np.trunc(s).astype(np.uint16)


def unit_plane(pooled, unit):
    """[h][w] float32 -> [h][pitch] u16: column w + j repeats column j % w (j = 0, 1, 2); the rest of the padding is zero."""
    h, w = pooled.shape
    plane = np.zeros((h, unit_plane_pitch(w)), np.uint16)
    plane[:, :w] = unit_value(pooled, unit)
    for j in range(3):
        plane[:, w + j] = plane[:, j % w]
    return plane


def stage_tile(plane, w, row0, col0, rows, cols):
    """A tile as the kernel stages it: lane l copies the four plane columns from wrap(col0 + 4 l) on to tile columns
    4 l .. 4 l + 3, for every lane with 4 l < cols; rows wrap cyclically.  Returns [rows][round_up(cols, 4)]."""
    h = plane.shape[0]
    out = np.zeros((rows, (cols + 3) & ~3), np.uint16)
    ridx = (row0 + np.arange(rows)) % h
    for l in range((cols + 3) // 4):
        c = (col0 + 4 * l) % w
        assert c + 4 <= plane.shape[1], "the 8-byte load leaves the row"
        out[:, 4 * l:4 * l + 4] = plane[ridx, c:c + 4]
    return out


def gather_tile(pooled_units, row0, col0, rows, cols):
    """The same tile by definition: tile (r, k) is the pooled pixel (wrap(row0 + r), wrap(col0 + k))."""
    h, w = pooled_units.shape
    return pooled_units[np.ix_((row0 + np.arange(rows)) % h, (col0 + np.arange(cols)) % w)]
