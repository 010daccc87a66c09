"""CPU model of the filtered exact-order route's approximate cost (k_match_filter.h), built from the oracle alone.

    A   the aggregated volume the reference order produces: the oracle on the real input at its real K.
    A~  what pass A / B of k_match_filter compute: the same aggregation on the pooled images rounded to the 1/u grid
        (u = K^2).  The rounded planes hold multiples of 1/u below 2^14, every tap, 3x3 cost and box sum of them is exact in
        float32 (below 2^24 units), so the oracle at K = 1 on those planes yields the kernel's integer sums divided by u and
        the same two rounded products.
    E   filter_error_bound_units(u) / u^3, in gray-level units; the units value comes from the library
        (tests/filter_bound_harness.cpp), not from a copy of its formula.

The kernel evaluates d exactly iff A~(d) >= max A~ - 2E; it is right iff the reference's winner m always passes, i.e. the
deficit (max A~ - A~(m)) / E never exceeds 2."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle_lib import OracleConfig


def round_to_grid(plane: np.ndarray, u: int) -> np.ndarray:
    """fast_stage<..., ROUND>: (unsigned short)(unit * v + 0.5f) in float32, as a gray level."""
    q = np.floor(np.float32(u) * plane.astype(np.float32) + np.float32(0.5))
    assert q.dtype == np.float32 and q.min() >= 0 and q.max() < 65536
    return (q / np.float32(u)).astype(np.float32)


class FilterModel(NamedTuple):
    exact: np.ndarray        # A   [h, w, Dd] float32
    approx: np.ndarray       # A~  [h, w, Dd] float32
    winner: np.ndarray       # the reference's arg-max [h, w]
    down_left: np.ndarray    # the pooled planes the oracle produced
    down_right: np.ndarray
    e_gray: float

    def error_ratio(self) -> float:
        """max |A~ - A| / E"""
        return float(np.abs(self.approx.astype(np.float64) - self.exact.astype(np.float64)).max() / self.e_gray)

    def deficit(self) -> np.ndarray:
        """(max_d A~ - A~(m)) / E per pixel"""
        at = self.approx.astype(np.float64)
        at_m = np.take_along_axis(at, self.winner[..., None].astype(np.int64), 2)[..., 0]
        return (at.max(axis=2) - at_m) / self.e_gray


def filter_model(oracle, left: np.ndarray, right: np.ndarray, K: int, Dd: int, e_units: float, dmin: int = 0) -> FilterModel:
    """left / right: the real input ([H, W] gray or [3, H, W] RGB); Dd pooled disparities from pooled dmin; e_units:
    filter_error_bound_units(K^2)."""
    u = K * K
    H, W = left.shape[-2:]
    cfg = OracleConfig(height=H, width=W, downscale_factor=K, min_disparity=dmin * K, max_disparity=(dmin + Dd) * K - 1)
    _, im = oracle.run(cfg, left, right, intermediates=True, volumes=True)
    dl, dr = im["down_left"], im["down_right"]
    h, w = dl.shape
    assert im["agg_volume"].shape == (h, w, Dd)
    cfg1 = OracleConfig(height=h, width=w, downscale_factor=1, min_disparity=dmin, max_disparity=dmin + Dd - 1)
    _, im1 = oracle.run(cfg1, round_to_grid(dl, u), round_to_grid(dr, u), intermediates=True, volumes=True)
    return FilterModel(im["agg_volume"], im1["agg_volume"], im["wta_index"], dl, dr, e_units / float(u) ** 3)
