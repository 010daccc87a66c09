"""The 'cuda' stereo-matching backend of the pipeline, over the MI355X engine.

Plays the role of /root/reference/src/python/pipeline/depth/cuda_stereo_matching_backend.py:7-17:
owns one native engine (here `cuda_depth` = the ctypes module over libstereo_mi355x.so) and feeds
it device-resident CHW frames.  The reference converts every frame to float32 before the call;
uint8 frames (what the cameras deliver) are handed over as they are -- the engine's RGB-u8 entry
does the same arithmetic on the bytes (float(u8) is exact), without the 4x larger copy.
"""
from __future__ import annotations

from typing import Optional

import torch

import cuda_depth
from pipeline.depth.map_postprocessing import MapPostprocessing, device_frame
from pipeline.depth.stereo_matching import StereoMatching


class CudaStereoMatchingBackend(MapPostprocessing, StereoMatching):
    """left_right_check=True: every map is left-right checked (StereoMatching.compute_disparity_map_batch_lr, one pair
    plus its mirrored twin per call, hence max_batch=2): pixels whose match in the right image does not point back to
    them within lr_max_diff pixels -- occlusions, the band left of min_disparity -- become invalid_disparity.
    speckle_max_size > 0: then the speckle filter (cuda_depth.filter_speckles) removes every region of speckle_max_size
    pixels or fewer whose 4-neighbours differ by at most speckle_max_diff.  fill_invalid=True: then the background hole
    fill (cuda_depth.fill_invalid) makes the map dense again.  Both run in place on the returned map, on the current
    stream, with a workspace allocated once; with the defaults neither runs.
    median_radius > 0: last, the image-guided weighted median (cuda_depth.weighted_median, tables from median_sigma_color
    and median_sigma_space), guided by the engine's own left gray plane.  With fill_invalid it filters only the pixels
    the fill wrote (the fill runs into a scratch map, the median writes the returned map); without, every valid pixel.
    With median_radius = 0 (the default) it does not run.
    wls_lambda > 0: after the speckle filter, the image-guided weighted least squares filter (cuda_depth.wls_filter,
    tables from wls_lambda, wls_sigma_color and wls_iterations, binary confidence), guided by the same gray plane; it
    fills the map itself, so fill_invalid=True or median_radius > 0 with it raise ValueError.  With wls_lambda = 0 (the
    default) it does not run.
    confidence=True (with confidence_lr_scale, confidence_radius, confidence_texture_scale): the per-pixel confidence
    of MapPostprocessing, confidence_map(); with left_right_check its LR term reads the engine's right-view map of the
    same call.
    temporal=True (with temporal_motion_radius, temporal_motion_threshold, temporal_decay, temporal_max_diff,
    temporal_max_weight, temporal_min_weight): the motion-gated temporal filter of MapPostprocessing, last, guided by the
    engine's left gray plane; reset_temporal() forgets its history.
    rectification (a cuda_depth.StereoRectification, default None): both raw frames are rectified on the current stream
    before matching (its out_shape must be the configuration's image size), and the pixels of the final map outside its
    left_valid mask become invalid_disparity."""

    def __init__(self, configuration: Optional["cuda_depth.StereoMatchingConfiguration"] = None, *,
                 left_right_check: bool = False, lr_max_diff: float = 1.0, invalid_disparity: float = -1.0,
                 speckle_max_size: int = 0, speckle_max_diff: float = 1.0, fill_invalid: bool = False,
                 median_radius: int = 0, median_sigma_color: float = 10.0, median_sigma_space: float = 5.0,
                 wls_lambda: float = 0.0, wls_sigma_color: float = 1.5, wls_iterations: int = 3,
                 confidence: bool = False, confidence_lr_scale: float = 1.0, confidence_radius: int = 2,
                 confidence_texture_scale: float = 10.0, temporal: bool = False, temporal_motion_radius: int = 1,
                 temporal_motion_threshold: float = 4.0, temporal_decay: float = 0.8, temporal_max_diff: float = 1.0,
                 temporal_max_weight: float = 8.0, temporal_min_weight: float = 0.25,
                 rectification: Optional["cuda_depth.StereoRectification"] = None):
        configuration = configuration or cuda_depth.StereoMatchingConfiguration()
        self._init_postprocessing(
            (configuration._values["height"], configuration._values["width"]), invalid_disparity=invalid_disparity,
            speckle_max_size=speckle_max_size, speckle_max_diff=speckle_max_diff, fill_invalid=fill_invalid,
            median_radius=median_radius, median_sigma_color=median_sigma_color, median_sigma_space=median_sigma_space,
            wls_lambda=wls_lambda, wls_sigma_color=wls_sigma_color, wls_iterations=wls_iterations,
            confidence=confidence, confidence_lr_scale=confidence_lr_scale, confidence_radius=confidence_radius,
            confidence_texture_scale=confidence_texture_scale, temporal=temporal,
            temporal_motion_radius=temporal_motion_radius, temporal_motion_threshold=temporal_motion_threshold,
            temporal_decay=temporal_decay, temporal_max_diff=temporal_max_diff,
            temporal_max_weight=temporal_max_weight, temporal_min_weight=temporal_min_weight,
            rectification=rectification)
        self._left_right_check = bool(left_right_check)
        self._lr_max_diff = float(lr_max_diff)
        self._invalid_disparity = float(invalid_disparity)
        if self._left_right_check:
            self._stereo_algo = cuda_depth.StereoMatching(configuration, max_batch=2)
        else:
            self._stereo_algo = cuda_depth.StereoMatching(configuration)

    def process(self, left_image: torch.Tensor, right_image: torch.Tensor) -> torch.Tensor:
        left, right = device_frame(left_image), device_frame(right_image)
        if left.dtype != right.dtype:                       # mixed inputs: fall back to float for both
            left, right = left.float(), right.float()
        left, right = self._rectify(left, right)
        right_map = None
        if self._left_right_check:
            if self._confidence:
                d = self._stereo_algo.dims
                right_map = self._right_map_buffer((1, d.H, d.W), left.device)
            disparity = self._stereo_algo.compute_disparity_map_batch_lr(
                left.unsqueeze(0), right.unsqueeze(0), right_out=right_map, max_diff=self._lr_max_diff,
                invalid_disparity=self._invalid_disparity)[0]
        else:
            disparity = self._stereo_algo.compute_disparity_map(left, right)
        self._finish(disparity, lambda guide: self._stereo_algo.intermediate(
            cuda_depth._native.STAGE_GRAY_LEFT, 0, out=guide), None if right_map is None else right_map[0])
        return disparity
