"""What the stereo-matching backends share around their matcher: rectification of the raw frames before matching, and
the post-processing of the map after it (speckle filter, per-pixel confidence, background hole fill, image-guided
weighted median or weighted least squares filter, the rectification's validity mask, the temporal filter).  Every step
runs on the current stream with buffers allocated once."""
from __future__ import annotations

from typing import Callable, Optional

import torch

import cuda_depth


def device_frame(image: torch.Tensor) -> torch.Tensor:
    """Contiguous, on the GPU, uint8 kept, everything else as float32."""
    image = image.cuda()
    if image.dtype != torch.uint8:
        image = image.float()
    return image.contiguous()


class MapPostprocessing:
    """Mixin of the backends: _init_postprocessing() in the constructor, _rectify() before matching, _finish() after.
    The backends take uint8 frames as uint8 and every other dtype as float32; a pair of different dtypes is taken as
    float32 for both, before the rectification.
    speckle_max_size > 0: the speckle filter (cuda_depth.filter_speckles) removes every region of speckle_max_size
    pixels or fewer whose 4-neighbours differ by at most speckle_max_diff.  fill_invalid=True: then the background hole
    fill (cuda_depth.fill_invalid) makes the map dense again.  Both run in place on the map.
    median_radius > 0: last, the image-guided weighted median (cuda_depth.weighted_median, tables from median_sigma_color
    and median_sigma_space), guided by the left gray plane of the matcher.  With fill_invalid it filters only the pixels
    the fill wrote (the fill runs into a scratch map, the median writes the map); without, every valid pixel.
    wls_lambda > 0: after the speckle filter, the image-guided weighted least squares filter (cuda_depth.wls_filter with
    lam=wls_lambda, sigma_color=wls_sigma_color, iterations=wls_iterations and binary confidence: every valid pixel
    weighs 1), guided by the same left gray plane, in place.  It fills the map itself, so it excludes fill_invalid and
    the median (ValueError).
    confidence=True: after the speckle filter and before the fill, the median or the WLS filter, the per-pixel
    confidence of the map (cuda_depth.confidence_map) into a persistent buffer, confidence_map(): the LR term from the
    right-view map the matcher hands over (left_right_check only; otherwise the map is texture-only) with
    confidence_lr_scale, the texture term over the same left gray plane with confidence_radius (0: none) and
    confidence_texture_scale.  Removed speckles and, with a rectification, the pixels outside its left_valid mask get 0;
    the pixels the fill writes keep 0.  With wls_lambda > 0 the WLS filter weighs each pixel by it.
    rectification (a cuda_depth.StereoRectification, or None): both raw frames are rectified before matching (its
    out_shape must be image_size), and the pixels of the final map outside its left_valid mask become invalid_disparity.
    temporal=True: last, after the rectification's mask, the motion-gated temporal filter (cuda_depth.TemporalFilter with
    temporal_motion_radius, temporal_motion_threshold, temporal_decay, temporal_max_diff, temporal_max_weight and
    temporal_min_weight) in place on the map, guided by the same left gray plane, with its history carried from one
    process() call to the next; reset_temporal() forgets it.  With confidence=True the confidence map is the
    measurement's weight, so the pixels the fill or the WLS filter wrote (confidence 0) keep their history."""

    def _init_postprocessing(self, image_size: tuple, *, invalid_disparity: float = -1.0, speckle_max_size: int = 0,
                             speckle_max_diff: float = 1.0, fill_invalid: bool = False, median_radius: int = 0,
                             median_sigma_color: float = 10.0, median_sigma_space: float = 5.0,
                             wls_lambda: float = 0.0, wls_sigma_color: float = 1.5, wls_iterations: int = 3,
                             confidence: bool = False, confidence_lr_scale: float = 1.0, confidence_radius: int = 2,
                             confidence_texture_scale: float = 10.0, temporal: bool = False,
                             temporal_motion_radius: int = 1, temporal_motion_threshold: float = 4.0,
                             temporal_decay: float = 0.8, temporal_max_diff: float = 1.0,
                             temporal_max_weight: float = 8.0, temporal_min_weight: float = 0.25,
                             rectification: Optional["cuda_depth.StereoRectification"] = None) -> None:
        if rectification is not None:
            if not isinstance(rectification, cuda_depth.StereoRectification):
                raise TypeError("rectification must be a cuda_depth.StereoRectification")
            size = tuple(image_size)
            if tuple(rectification.out_shape) != size:
                raise ValueError(f"rectification.out_shape {tuple(rectification.out_shape)} differs from the image "
                                 f"size {size}")
        self._rectification = rectification
        self._rectified: Optional[tuple] = None             # persistent output frames of the rectification
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
        cuda_depth._check_wls_params(wls_lambda, wls_sigma_color, wls_iterations, 0.25)
        if wls_lambda > 0 and (self._fill_invalid or median_radius > 0):
            raise ValueError("wls_lambda > 0 fills the map itself: it cannot be combined with fill_invalid=True or "
                             "median_radius > 0")
        self._wls_tables = cuda_depth.wls_tables(wls_lambda, wls_sigma_color, wls_iterations) if wls_lambda > 0 else None
        self._wls_workspace: Optional[torch.Tensor] = None
        self._median_guide: Optional[torch.Tensor] = None   # the left gray plane of the last call
        self._median_scratch: Optional[torch.Tensor] = None
        if not isinstance(confidence, bool):
            raise TypeError("confidence must be a bool")
        cuda_depth._check_confidence_params(confidence_radius, confidence_lr_scale, confidence_texture_scale,
                                            invalid_disparity, radius_zero_ok=True)
        self._confidence = confidence
        self._confidence_lr_scale = float(confidence_lr_scale)
        self._confidence_radius = confidence_radius
        self._confidence_texture_scale = float(confidence_texture_scale)
        self._confidence_map: Optional[torch.Tensor] = None     # the confidence of the last call
        self._right_map: Optional[torch.Tensor] = None          # the matcher's right-view map (confidence, LR check)
        if not isinstance(temporal, bool):
            raise TypeError("temporal must be a bool")
        self._temporal_params = dict(motion_radius=temporal_motion_radius, motion_threshold=temporal_motion_threshold,
                                     decay=temporal_decay, max_diff=temporal_max_diff,
                                     max_weight=temporal_max_weight, min_weight=temporal_min_weight)
        cuda_depth._check_temporal_params(**self._temporal_params, invalid_disparity=invalid_disparity)
        self._temporal = temporal
        self._temporal_filter: Optional["cuda_depth.TemporalFilter"] = None   # created at the first frame

    def _guide_buffer(self, like: torch.Tensor) -> torch.Tensor:
        """The persistent [H, W] float32 buffer the matcher's left gray plane goes into (median_radius > 0 or
        wls_lambda > 0)."""
        if self._median_guide is None:
            self._median_guide = torch.empty_like(like)
            self._median_scratch = torch.empty_like(like)
        return self._median_guide

    def _uses_guide(self) -> bool:
        """Whether a post-processing step needs the left gray plane (the median, the WLS filter, the confidence's
        texture term or the temporal filter)."""
        return self._median_radius > 0 or self._wls_tables is not None or (self._confidence and
                                                                            self._confidence_radius > 0) or self._temporal

    def _right_map_buffer(self, shape: tuple, device: torch.device) -> torch.Tensor:
        """The persistent float32 buffer of `shape` the matcher's right-view map goes into (confidence=True with the
        left-right check)."""
        if self._right_map is None or tuple(self._right_map.shape) != tuple(shape) or self._right_map.device != device:
            self._right_map = torch.empty(shape, dtype=torch.float32, device=device)
        return self._right_map

    def confidence_map(self) -> Optional[torch.Tensor]:
        """The [H, W] float32 confidence of the last process() call (a persistent buffer, overwritten by the next call),
        or None with confidence=False."""
        return self._confidence_map if self._confidence else None

    def _rectify(self, left: torch.Tensor, right: torch.Tensor):
        """Both frames through the rectification (into persistent buffers), or unchanged without one."""
        if self._rectification is None:
            return left, right
        shape = tuple(left.shape[:-2]) + tuple(self._rectification.out_shape)
        if self._rectified is None or self._rectified[0].dtype != left.dtype or tuple(self._rectified[0].shape) != shape:
            self._rectified = (torch.empty(shape, dtype=left.dtype, device=left.device),
                               torch.empty(shape, dtype=left.dtype, device=left.device))
        return self._rectification.rectify(left, right, out=self._rectified)

    def rectified_frames(self) -> Optional[tuple]:
        """(left, right) rectified frames of the last process() call (persistent buffers, overwritten by the next
        call), or None without rectification."""
        return self._rectified if self._rectification is not None else None

    def _finish(self, disparity: torch.Tensor, write_guide: Optional[Callable[[torch.Tensor], None]] = None,
                right_disp: Optional[torch.Tensor] = None) -> None:
        """Post-processes the [H, W] map in place.  write_guide(buffer): writes the left gray plane into the guide
        buffer when a step needs it (None: the matcher already wrote _guide_buffer()).  right_disp: the matcher's
        un-checked [H, W] right-view map for the confidence's LR term, or None."""
        if self._speckle_max_size > 0 or self._fill_invalid or self._uses_guide() or self._confidence:
            self._postprocess(disparity, write_guide, right_disp)
        if self._rectification is not None:
            disparity.masked_fill_(~self._rectification.left_valid, self._invalid_disparity)
        if self._temporal:
            self._apply_temporal(disparity)

    def _apply_temporal(self, disparity: torch.Tensor) -> None:
        """The temporal filter on the finished [H, W] map, in place, guided by the left gray plane _postprocess wrote."""
        H, W = int(disparity.shape[-2]), int(disparity.shape[-1])
        f = self._temporal_filter
        if f is None or f.device != disparity.device or (f.H, f.W) != (H, W):
            f = self._temporal_filter = cuda_depth.TemporalFilter(1, H, W, device=disparity.device,
                                                                  invalid_disparity=self._invalid_disparity,
                                                                  **self._temporal_params)
        f.apply(disparity, self._median_guide, confidence=self._confidence_map if self._confidence else None,
                out=disparity)

    def reset_temporal(self) -> None:
        """Forgets the temporal filter's history: the next frame's map is returned as the other steps leave it."""
        if self._temporal_filter is not None:
            self._temporal_filter.reset()

    def _postprocess(self, disparity: torch.Tensor, write_guide, right_disp) -> None:
        H, W = int(disparity.shape[-2]), int(disparity.shape[-1])
        if self._post_workspace is None and (self._speckle_max_size > 0 or self._fill_invalid):
            self._post_workspace = cuda_depth._postprocess_workspace(1, H, W, disparity.device)
        if self._speckle_max_size > 0:
            cuda_depth._launch_filter_speckles(disparity, disparity, 1, H, W, self._speckle_max_size,
                                               self._speckle_max_diff, self._invalid_disparity, self._post_workspace)
        guide = None
        if self._uses_guide():
            guide = self._guide_buffer(disparity)
            if write_guide is not None:
                write_guide(guide)
        confidence = None
        if self._confidence:
            confidence = self._compute_confidence(disparity, right_disp, guide)
        if self._wls_tables is not None:
            if self._wls_workspace is None:
                self._wls_workspace = cuda_depth._wls_workspace(1, H, W, disparity.device)
            cuda_depth._launch_wls(disparity, confidence, guide, disparity, 1, H, W, *self._wls_tables, 1e-3,
                                   self._invalid_disparity, self._wls_workspace)
            return
        if self._median_radius == 0:
            if self._fill_invalid:
                cuda_depth._launch_fill_invalid(disparity, disparity, 1, H, W, self._invalid_disparity,
                                                self._post_workspace)
            return
        scratch = self._median_scratch
        if self._fill_invalid:                              # filled -> scratch; the median rewrites the filled pixels
            cuda_depth._launch_fill_invalid(disparity, scratch, 1, H, W, self._invalid_disparity, self._post_workspace)
            holes = disparity
        else:                                               # every valid pixel
            scratch.copy_(disparity)
            holes = None
        cuda_depth._launch_weighted_median(scratch, holes, guide, disparity, 1, H, W, self._median_radius,
                                           *self._median_tables, self._invalid_disparity,
                                           cuda_depth._median_workspace(1, H, W, disparity.device))

    def _compute_confidence(self, disparity: torch.Tensor, right_disp: Optional[torch.Tensor],
                            guide: Optional[torch.Tensor]) -> torch.Tensor:
        """The confidence of the [H, W] map as it stands (after the speckle filter) into the persistent buffer; 0 outside
        the rectification's left_valid mask."""
        if self._confidence_map is None or self._confidence_map.device != disparity.device:
            self._confidence_map = torch.empty_like(disparity)
        H, W = int(disparity.shape[-2]), int(disparity.shape[-1])
        radius = self._confidence_radius
        cuda_depth._launch_confidence(disparity, right_disp, guide if radius > 0 else None, self._confidence_map, 1, H,
                                      W, radius, self._confidence_lr_scale, self._confidence_texture_scale,
                                      self._invalid_disparity)
        if self._rectification is not None:
            self._confidence_map.masked_fill_(~self._rectification.left_valid, 0.0)
        return self._confidence_map
