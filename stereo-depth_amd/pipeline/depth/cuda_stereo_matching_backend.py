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
from pipeline.depth.stereo_matching import StereoMatching


def _device_frame(image: torch.Tensor) -> torch.Tensor:
    """Contiguous, on the GPU, uint8 kept, everything else as float32."""
    image = image.cuda()
    if image.dtype != torch.uint8:
        image = image.float()
    return image.contiguous()


class CudaStereoMatchingBackend(StereoMatching):
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
    rectification (a cuda_depth.StereoRectification, default None): both raw frames are rectified on the current stream
    before matching (its out_shape must be the configuration's image size), and the pixels of the final map outside its
    left_valid mask become invalid_disparity."""

    def __init__(self, configuration: Optional["cuda_depth.StereoMatchingConfiguration"] = None, *,
                 left_right_check: bool = False, lr_max_diff: float = 1.0, invalid_disparity: float = -1.0,
                 speckle_max_size: int = 0, speckle_max_diff: float = 1.0, fill_invalid: bool = False,
                 median_radius: int = 0, median_sigma_color: float = 10.0, median_sigma_space: float = 5.0,
                 rectification: Optional["cuda_depth.StereoRectification"] = None):
        configuration = configuration or cuda_depth.StereoMatchingConfiguration()
        if rectification is not None:
            if not isinstance(rectification, cuda_depth.StereoRectification):
                raise TypeError("rectification must be a cuda_depth.StereoRectification")
            size = (configuration._values["height"], configuration._values["width"])
            if tuple(rectification.out_shape) != size:
                raise ValueError(f"rectification.out_shape {tuple(rectification.out_shape)} differs from the image "
                                 f"size {size}")
        self._rectification = rectification
        self._rectified: Optional[tuple] = None             # persistent output frames of the rectification
        self._left_right_check = bool(left_right_check)
        self._lr_max_diff = float(lr_max_diff)
        self._invalid_disparity = float(invalid_disparity)
        cuda_depth._check_speckle_size(speckle_max_size)
        cuda_depth._check_lr_scalars(speckle_max_diff, invalid_disparity)
        self._speckle_max_size = speckle_max_size
        self._speckle_max_diff = float(speckle_max_diff)
        self._fill_invalid = bool(fill_invalid)
        self._post_workspace: Optional[torch.Tensor] = None
        cuda_depth._int_arg("median_radius", median_radius)
        if median_radius != 0:                              # 0: off; otherwise 1..15 with finite, positive sigmas
            self._median_tables = cuda_depth.median_weight_tables(median_radius, median_sigma_color, median_sigma_space)
        else:
            cuda_depth._check_median_params(1, median_sigma_color, median_sigma_space)
        self._median_radius = median_radius
        self._median_guide: Optional[torch.Tensor] = None   # the left gray plane of the last call
        self._median_scratch: Optional[torch.Tensor] = None
        if self._left_right_check:
            self._stereo_algo = cuda_depth.StereoMatching(configuration, max_batch=2)
        else:
            self._stereo_algo = cuda_depth.StereoMatching(configuration)

    def process(self, left_image: torch.Tensor, right_image: torch.Tensor) -> torch.Tensor:
        left, right = _device_frame(left_image), _device_frame(right_image)
        if left.dtype != right.dtype:                       # mixed inputs: fall back to float for both
            left, right = left.float(), right.float()
        if self._rectification is not None:
            left, right = self._rectify(left, right)
        if self._left_right_check:
            disparity = self._stereo_algo.compute_disparity_map_batch_lr(
                left.unsqueeze(0), right.unsqueeze(0), max_diff=self._lr_max_diff,
                invalid_disparity=self._invalid_disparity)[0]
        else:
            disparity = self._stereo_algo.compute_disparity_map(left, right)
        if self._speckle_max_size > 0 or self._fill_invalid or self._median_radius > 0:
            self._postprocess(disparity)
        if self._rectification is not None:
            disparity.masked_fill_(~self._rectification.left_valid, self._invalid_disparity)
        return disparity

    def rectified_frames(self) -> Optional[tuple]:
        """(left, right) rectified frames of the last process() call (persistent buffers, overwritten by the next
        call), or None without rectification."""
        return self._rectified if self._rectification is not None else None

    def _rectify(self, left: torch.Tensor, right: torch.Tensor):
        shape = tuple(left.shape[:-2]) + tuple(self._rectification.out_shape)
        if self._rectified is None or self._rectified[0].dtype != left.dtype or tuple(self._rectified[0].shape) != shape:
            self._rectified = (torch.empty(shape, dtype=left.dtype, device=left.device),
                               torch.empty(shape, dtype=left.dtype, device=left.device))
        return self._rectification.rectify(left, right, out=self._rectified)

    def _postprocess(self, disparity: torch.Tensor) -> None:
        H, W = int(disparity.shape[-2]), int(disparity.shape[-1])
        if self._post_workspace is None and (self._speckle_max_size > 0 or self._fill_invalid):
            self._post_workspace = cuda_depth._postprocess_workspace(1, H, W, disparity.device)
        if self._speckle_max_size > 0:
            cuda_depth._launch_filter_speckles(disparity, disparity, 1, H, W, self._speckle_max_size,
                                               self._speckle_max_diff, self._invalid_disparity, self._post_workspace)
        if self._median_radius == 0:
            if self._fill_invalid:
                cuda_depth._launch_fill_invalid(disparity, disparity, 1, H, W, self._invalid_disparity,
                                                self._post_workspace)
            return
        if self._median_guide is None:
            self._median_guide = torch.empty_like(disparity)
            self._median_scratch = torch.empty_like(disparity)
        self._stereo_algo.intermediate(cuda_depth._native.STAGE_GRAY_LEFT, 0, out=self._median_guide)
        scratch = self._median_scratch
        if self._fill_invalid:                              # filled -> scratch; the median rewrites the filled pixels
            cuda_depth._launch_fill_invalid(disparity, scratch, 1, H, W, self._invalid_disparity, self._post_workspace)
            holes = disparity
        else:                                               # every valid pixel
            scratch.copy_(disparity)
            holes = None
        cuda_depth._launch_weighted_median(scratch, holes, self._median_guide, disparity, 1, H, W, self._median_radius,
                                           *self._median_tables, self._invalid_disparity,
                                           cuda_depth._median_workspace(1, H, W, disparity.device))
