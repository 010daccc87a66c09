"""CPU restatement of DepthEstimationPipeline.process() for the 'cuda' and 'sgm' backends, built only from the
references of the single steps.  The order of the steps and the operands of each are those the documentation states
(the DepthEstimationPipeline and MapPostprocessing docstrings), not read off the pipeline's code:

  0. both frames as the backend takes them: uint8 kept, everything else float32; two frames of different dtypes are
     both taken as float32;
  1. rectification (rectify_ref.remap of each frame through its map, constant border 0), if configured;
  2. the matcher: the map, the left gray plane (the guide of every later step) and, with left_right_check, the
     un-checked right-view map.
       cuda: the CPU oracle with the engine configuration the pipeline builds (shape and disparity range, every other
             field at its default), the guide its gray_left intermediate; with the LR check the right-view map is
             flip(oracle(flip R, flip L)) and the map lr_ref.lr_rule(map, right-view map);
       sgm:  sgm_ref's cost volume and aggregation, the map from its select (the LR check in it), the right-view map
             f32(dmin + iR) of its right-view winners (invalid_disparity where there are none), the guide its gray;
  3. the speckle filter (speckle_max_size > 0);
  4. the confidence (confidence=True) of the map as it stands, from the right-view map (LR check only) and the guide
     (confidence_radius > 0 only); 0 outside the rectification's left_valid;
  5. either the WLS filter (wls_lambda > 0), weighted by the confidence when there is one and binary otherwise, or the
     fill (fill_invalid) and the weighted median (median_radius > 0): the median of the filled map over the pixels the
     fill wrote, or without the fill over every valid pixel;
  6. invalid_disparity outside the rectification's left_valid;
  7. the temporal filter (temporal=True), guided by the same gray plane, weighted by the confidence when there is one,
     its history carried across process() calls until reset_temporal().

Nothing from pipeline/ is imported; the host-only table builders of cuda_depth are (their formulas are pinned by the
CPU tests of the median and the WLS filter)."""
from __future__ import annotations

from typing import Optional

import numpy as np

import confidence_ref
import median_ref
import postprocess_ref
import rectify_ref
import sgm_ref
import temporal_ref
import wls_ref
from lr_ref import lr_rule

F = np.float32
ENGINE_DOWNSCALE = 2            # the engine configuration's default downscale_factor, which the pipeline keeps
WLS_MIN_WEIGHT = 1e-3           # cuda_depth.wls_filter's default min_weight


def flip(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a)[..., ::-1])


def frame(a) -> np.ndarray:
    """A frame as the backends take it: uint8 kept, everything else float32."""
    a = np.asarray(a)
    return np.ascontiguousarray(a if a.dtype == np.uint8 else a.astype(F))


class PipelineRef:
    """The reference chain with the pipeline's keywords.  rectification: None or (left_map, right_map, in_shape), the
    int32 maps and raw shape of a cuda_depth.StereoRectification with its default border (constant 0).  oracle: an
    oracle_lib.Oracle (the 'cuda' backend only).  process(left, right) takes [C, H, W] numpy frames and returns
    (disparity, confidence or None, rectified left or None, rectified right or None), all new arrays."""

    def __init__(self, image_shape, min_disparity: int, max_disparity: int, invalid_disparity: float = -1.0,
                 backend: str = "cuda", left_right_check: bool = False, lr_max_diff: float = 1.0, *, oracle=None,
                 speckle_max_size: int = 0, speckle_max_diff: float = 1.0, fill_invalid: bool = False,
                 median_radius: int = 0, median_sigma_color: float = 10.0, median_sigma_space: float = 5.0,
                 wls_lambda: float = 0.0, wls_sigma_color: float = 1.5, wls_iterations: int = 3,
                 confidence: bool = False, confidence_lr_scale: float = 1.0, confidence_radius: int = 2,
                 confidence_texture_scale: float = 10.0, temporal: bool = False, temporal_motion_radius: int = 1,
                 temporal_motion_threshold: float = 4.0, temporal_decay: float = 0.8, temporal_max_diff: float = 1.0,
                 temporal_max_weight: float = 8.0, temporal_min_weight: float = 0.25, rectification=None,
                 sgm_paths: int = 8, sgm_p1: int = 10, sgm_p2: int = 120, sgm_uniqueness: int = 0):
        if backend not in ("cuda", "sgm"):
            raise ValueError(f"backend must be 'cuda' or 'sgm', got {backend!r}")
        if wls_lambda > 0 and (fill_invalid or median_radius > 0):
            raise ValueError("wls_lambda > 0 fills the map itself: it cannot be combined with fill_invalid=True or "
                             "median_radius > 0")
        if backend == "cuda" and oracle is None:
            raise ValueError("the 'cuda' backend needs the oracle")
        self.H, self.W = (int(v) for v in image_shape)
        self.dmin, self.dmax = int(min_disparity), int(max_disparity)
        self.inv = F(invalid_disparity)
        self.backend, self.lr, self.lr_max_diff = backend, bool(left_right_check), float(lr_max_diff)
        self.oracle = oracle
        self.speckle = (int(speckle_max_size), float(speckle_max_diff))
        self.fill = bool(fill_invalid)
        self.median_radius = int(median_radius)
        if self.median_radius > 0:
            import cuda_depth
            self.median_tables = cuda_depth.median_weight_tables(median_radius, median_sigma_color, median_sigma_space)
        self.wls_tables = None
        if wls_lambda > 0:
            import cuda_depth
            self.wls_tables = cuda_depth.wls_tables(wls_lambda, wls_sigma_color, wls_iterations)
        self.confidence = bool(confidence)
        self.conf_params = dict(radius=int(confidence_radius), lr_scale=float(confidence_lr_scale),
                                texture_scale=float(confidence_texture_scale))
        self.rect = None
        if rectification is not None:
            qL, qR, in_shape = rectification
            qL, qR = np.asarray(qL, np.int32), np.asarray(qR, np.int32)
            assert qL.shape == qR.shape == (self.H, self.W, 2)
            self.rect = (qL, qR, rectify_ref.valid_mask(qL, tuple(in_shape)))
        self.sgm = dict(paths=sgm_paths, P1=sgm_p1, P2=sgm_p2, uniqueness=sgm_uniqueness)
        self.temporal = None
        if temporal:
            self.temporal = temporal_ref.TemporalRef(
                (self.H, self.W), motion_radius=temporal_motion_radius, motion_threshold=temporal_motion_threshold,
                decay=temporal_decay, max_diff=temporal_max_diff, max_weight=temporal_max_weight,
                min_weight=temporal_min_weight, invalid_disparity=float(invalid_disparity))

    # ------------------------------------------------------------------ the matchers
    def _match_cuda(self, L, R):
        from oracle_lib import OracleConfig
        ocfg = OracleConfig(height=self.H, width=self.W, downscale_factor=ENGINE_DOWNSCALE,
                            min_disparity=self.dmin, max_disparity=self.dmax)
        L, R = L.astype(F), R.astype(F)                 # the engine's u8 entries compute on float(u8), which is exact
        d, im = self.oracle.run(ocfg, L, R, intermediates=True)
        right = None
        if self.lr:
            right = flip(self.oracle.run(ocfg, flip(R), flip(L)))
            d = lr_rule(d, right, self.lr_max_diff, self.inv)
        return d, im["gray_left"], right

    def _match_sgm(self, L, R):
        gl, gr = sgm_ref.gray(L), sgm_ref.gray(R)
        C = sgm_ref.cost_volume(sgm_ref.census(gl), sgm_ref.census(gr), self.dmin, self.dmax - self.dmin + 1)
        S = sgm_ref.aggregate(C, self.sgm["paths"], self.sgm["P1"], self.sgm["P2"])
        d = sgm_ref.select(S, self.dmin, self.sgm["uniqueness"], self.lr_max_diff if self.lr else -1.0, True,
                           float(self.inv))
        right = None
        if self.lr:
            iR = sgm_ref.right_wta(S, self.dmin)
            right = np.where(iR >= 0, (self.dmin + iR).astype(F), self.inv).astype(F)
        return d, gl, right

    # ------------------------------------------------------------------ the chain
    def process(self, left, right):
        L, R = frame(left), frame(right)
        if L.dtype != R.dtype:
            L, R = L.astype(F), R.astype(F)
        rect_l = rect_r = None
        if self.rect is not None:
            qL, qR, _ = self.rect
            L = rect_l = rectify_ref.remap(L[None], qL)[0]
            R = rect_r = rectify_ref.remap(R[None], qR)[0]
        assert L.shape[-2:] == (self.H, self.W), L.shape
        d, guide, right_map = (self._match_cuda if self.backend == "cuda" else self._match_sgm)(L, R)
        d = np.array(d, F)
        inv = float(self.inv)
        if self.speckle[0] > 0:
            d = postprocess_ref.filter_speckles(d, self.speckle[0], self.speckle[1], inv)
        conf = None
        if self.confidence:
            radius = self.conf_params["radius"]
            conf = confidence_ref.confidence_map(d, right_map, guide if radius > 0 else None, radius,
                                                 self.conf_params["lr_scale"], self.conf_params["texture_scale"], inv)
            if self.rect is not None:
                conf = np.where(self.rect[2], conf, F(0.0)).astype(F)
        if self.wls_tables is not None:
            d = wls_ref.wls_filter(d, guide, *self.wls_tables, confidence=conf, min_weight=WLS_MIN_WEIGHT,
                                   invalid_disparity=inv)
        elif self.median_radius > 0:
            if self.fill:
                d = median_ref.weighted_median(postprocess_ref.fill_invalid(d, inv), guide, self.median_radius,
                                               *self.median_tables, holes=d, invalid_disparity=inv)
            else:
                d = median_ref.weighted_median(d, guide, self.median_radius, *self.median_tables,
                                               invalid_disparity=inv)
        elif self.fill:
            d = postprocess_ref.fill_invalid(d, inv)
        if self.rect is not None:
            d = np.where(self.rect[2], d, self.inv).astype(F)
        if self.temporal is not None:
            d = self.temporal.apply(d, guide, conf)
        return d, conf, rect_l, rect_r

    def reset_temporal(self) -> None:
        if self.temporal is not None:
            self.temporal.reset()

    @property
    def left_valid(self) -> Optional[np.ndarray]:
        return None if self.rect is None else self.rect[2]
