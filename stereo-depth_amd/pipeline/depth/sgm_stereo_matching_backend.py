"""The 'sgm' stereo-matching backend of the pipeline: semi-global matching (cuda_depth.StereoSGM) in place of the
engine's multi-block matcher, with the same rectification and post-processing around it as the 'cuda' backend."""
from __future__ import annotations

from typing import Optional

import torch

import cuda_depth
from pipeline.depth.map_postprocessing import MapPostprocessing, device_frame
from pipeline.depth.stereo_matching import StereoMatching


class SgmStereoMatchingBackend(MapPostprocessing, StereoMatching):
    """Semi-global matching at full resolution over min_disparity..max_disparity (at most 256 candidates), with paths,
    P1, P2, uniqueness and subpixel as cuda_depth.StereoSGM takes them.  image_shape: (height, width) of the frames it
    matches (after rectification).  left_right_check=True: the in-kernel left-right check of StereoSGM with
    lr_max_diff.  The post-processing and rectification keywords are those of CudaStereoMatchingBackend; the guide of the
    weighted median, of the WLS filter and of the confidence's texture term is the left gray plane StereoSGM writes
    beside the map; with left_right_check, the confidence's LR term reads the right-view map StereoSGM writes too."""

    def __init__(self, image_shape=(384, 1280), min_disparity: int = 0, max_disparity: int = 127, *, paths: int = 8,
                 P1: int = 10, P2: int = 120, uniqueness: int = 0, subpixel: bool = True,
                 left_right_check: bool = False, lr_max_diff: float = 1.0, invalid_disparity: float = -1.0,
                 speckle_max_size: int = 0, speckle_max_diff: float = 1.0, fill_invalid: bool = False,
                 median_radius: int = 0, median_sigma_color: float = 10.0, median_sigma_space: float = 5.0,
                 wls_lambda: float = 0.0, wls_sigma_color: float = 1.5, wls_iterations: int = 3,
                 confidence: bool = False, confidence_lr_scale: float = 1.0, confidence_radius: int = 2,
                 confidence_texture_scale: float = 10.0, temporal: bool = False, temporal_motion_radius: int = 1,
                 temporal_motion_threshold: float = 4.0, temporal_decay: float = 0.8, temporal_max_diff: float = 1.0,
                 temporal_max_weight: float = 8.0, temporal_min_weight: float = 0.25,
                 rectification: Optional["cuda_depth.StereoRectification"] = None):
        self._image_shape = cuda_depth._shape2("image_shape", image_shape)
        self._init_postprocessing(
            self._image_shape, invalid_disparity=invalid_disparity, speckle_max_size=speckle_max_size,
            speckle_max_diff=speckle_max_diff, fill_invalid=fill_invalid, median_radius=median_radius,
            median_sigma_color=median_sigma_color, median_sigma_space=median_sigma_space, wls_lambda=wls_lambda,
            wls_sigma_color=wls_sigma_color, wls_iterations=wls_iterations, confidence=confidence,
            confidence_lr_scale=confidence_lr_scale, confidence_radius=confidence_radius,
            confidence_texture_scale=confidence_texture_scale, temporal=temporal,
            temporal_motion_radius=temporal_motion_radius, temporal_motion_threshold=temporal_motion_threshold,
            temporal_decay=temporal_decay, temporal_max_diff=temporal_max_diff,
            temporal_max_weight=temporal_max_weight, temporal_min_weight=temporal_min_weight,
            rectification=rectification)
        self._left_right_check = bool(left_right_check)
        self._sgm = cuda_depth.StereoSGM(min_disparity, max_disparity, paths=paths, P1=P1, P2=P2,
                                         uniqueness=uniqueness,
                                         lr_max_diff=float(lr_max_diff) if left_right_check else None,
                                         subpixel=subpixel, invalid_disparity=invalid_disparity)
        self._disparity: Optional[torch.Tensor] = None      # persistent output map

    def process(self, left_image: torch.Tensor, right_image: torch.Tensor) -> torch.Tensor:
        left, right = device_frame(left_image), device_frame(right_image)
        if left.dtype != right.dtype:                       # mixed inputs: fall back to float for both
            left, right = left.float(), right.float()
        left, right = self._rectify(left, right)
        if left.dim() != 3 or tuple(left.shape[-2:]) != self._image_shape:
            raise RuntimeError(f"frames must be [C,H,W] of the configured image_shape {self._image_shape}, got "
                               f"{tuple(left.shape)}")
        if self._disparity is None or self._disparity.device != left.device:
            self._disparity = torch.empty(self._image_shape, dtype=torch.float32, device=left.device)
        guide = self._guide_buffer(self._disparity) if self._uses_guide() else None
        right_map = None
        if self._confidence and self._left_right_check:
            right_map = self._right_map_buffer(self._image_shape, left.device)
        self._sgm.compute(left, right, out=self._disparity, gray_out=guide, right_out=right_map)
        self._finish(self._disparity, right_disp=right_map)
        return self._disparity
