"""NumPy twin of the left-right consistency check (include/stereo_mi355x.h: smx_compute_lr_*, smx_lr_check)."""
import numpy as np


def lr_rule(dl: np.ndarray, dr: np.ndarray, max_diff: float = 1.0, invalid_disparity: float = -1.0) -> np.ndarray:
    """NumPy twin of the check: dl = left-referenced map, dr = right-referenced map, both [..., H, W] float32."""
    dl = np.asarray(dl, np.float32)
    dr = np.asarray(dr, np.float32)
    with np.errstate(invalid="ignore"):
        t = np.floor(dl + np.float32(0.5))
        Y = np.arange(dl.shape[-1])
        ok = np.isfinite(t) & (t >= 0) & (t <= Y)
        yr = Y - np.where(ok, t, 0).astype(np.int64)
        ok &= np.abs(dl - np.take_along_axis(dr, yr, -1)) <= np.float32(max_diff)
    return np.where(ok, dl, np.float32(invalid_disparity)).astype(np.float32)
