"""Pipeline facade: the direct caller of the backend boundary.

Same public surface as /root/reference/src/python/pipeline/depth_estimation_pipeline.py:14-87
(`DepthEstimationPipelineConfig` with its six fields -- plus the opt-in left-right check -- and `update`, `DepthEstimationResult`,
`DepthEstimationPipelineContext`, `DepthEstimationPipeline.process / get_configuration`) for the
'cuda' and 'sgm' backends.  The right view is synthesised when process() gets none and the pipeline was given a
pipeline.synthesis.RightViewSynthesis (the network inside it is the caller's); without one
`right_image` is mandatory.  The traced-DNN backends are out of scope: their names raise.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Any, Optional, Tuple

import numpy as np
import torch

import cuda_depth
from helpers.torch_helpers import cuda_perf_clock
from pipeline.depth import AVAILABLE_DNN_BACKENDS, CudaStereoMatchingBackend, SgmStereoMatchingBackend, StereoMatching
from pipeline.synthesis import RightViewSynthesis

_BACKENDS = ("cuda", "sgm") + AVAILABLE_DNN_BACKENDS


@dataclasses.dataclass
class DepthEstimationPipelineConfig:
    """Field names and defaults: depth_estimation_pipeline.py:15-21 of the reference."""
    image_shape: Tuple[int, int] = (384, 1280)
    min_disparity: int = 1
    max_disparity: int = 64
    invalid_disparity: float = -1.0
    stereo_matching_backend: str = "cuda"          # one of "cuda", "sgm", "msnet2d", "msnet3d", "gwcnet"
    log_perf_time: bool = False
    # additions (no counterpart in the reference): left-right consistency check of the 'cuda' and 'sgm' backends --
    # pixels whose match in the right image does not point back to them within lr_max_diff pixels become
    # invalid_disparity
    left_right_check: bool = False
    lr_max_diff: float = 1.0

    def update(self, **changes: Any) -> "DepthEstimationPipelineConfig":
        """In-place update that rejects unknown fields (reference :23-28); returns self."""
        known = {f.name for f in dataclasses.fields(self)}
        unknown = [name for name in changes if name not in known]
        if unknown:
            raise RuntimeError(f"Unexpected keyword argument: '{unknown[0]}'.")
        for name, value in changes.items():
            setattr(self, name, value)
        return self

    def engine_configuration(self) -> "cuda_depth.StereoMatchingConfiguration":
        """What the pipeline hands to the native engine (reference :77-82): shape and disparity
        range; every other engine parameter keeps its default."""
        height, width = self.image_shape
        return cuda_depth.StereoMatchingConfiguration(height=height, width=width,
                                                      min_disparity=self.min_disparity,
                                                      max_disparity=self.max_disparity)


@dataclasses.dataclass
class DepthEstimationResult:
    left_image: torch.Tensor
    right_image: torch.Tensor
    disparity_map: torch.Tensor
    # reprojection_matrix given: the map's metric cloud (cuda_depth.PointCloud, new tensors), coloured from left_image,
    # voxel-downsampled with point_cloud_voxel_size > 0; None otherwise.  Keyword-only, so the positional order of the
    # earlier fields (confidence_map fourth) is unchanged.
    point_cloud: Optional["cuda_depth.PointCloud"] = dataclasses.field(default=None, kw_only=True)
    # render_model=True: the [H, W] disparity map of the fused volume seen from this frame's camera_pose, rendered after
    # the frame was integrated (TSDFVolume.render: a fresh tensor, invalid_disparity where no surface is hit); None
    # otherwise.  Keyword-only as well, and declared here: confidence_map stays the last field
    model_disparity_map: Optional[torch.Tensor] = dataclasses.field(default=None, kw_only=True)
    # track_camera=True: the camera-to-world pose [4, 4] float64 (numpy) the frame was given -- initial_pose for the first
    # frame, the tracked pose after it, the last good pose where tracking was lost -- and whether it was lost (the frame is
    # then not integrated); None otherwise.  Keyword-only as well
    camera_pose: Optional[Any] = dataclasses.field(default=None, kw_only=True)
    tracking_lost: Optional[bool] = dataclasses.field(default=None, kw_only=True)
    # follow_camera=True: how far the volume moved before this frame was integrated, in whole voxels (TSDFVolume.follow;
    # (0, 0, 0) for a frame that did not move it and without follow_camera), and with keep_spill=True what left it then
    # (TSDFVolume.shift's boxes, new volumes; empty otherwise).  Keyword-only as well
    volume_shift: Tuple[int, int, int] = dataclasses.field(default=(0, 0, 0), kw_only=True)
    spilled_volumes: list = dataclasses.field(default_factory=list, kw_only=True)
    # spill_store=: how many stored regions were merged back into the volume when this frame moved it
    # (TSDFSpillStore.follow); 0 otherwise.  Keyword-only as well
    restored_boxes: int = dataclasses.field(default=0, kw_only=True)
    # confidence=True: the [H, W] per-pixel confidence in [0, 1] of the map (a persistent buffer, like the map);
    # None otherwise
    confidence_map: Optional[torch.Tensor] = None


@dataclasses.dataclass
class DepthEstimationPipelineContext:
    disparity_map: torch.Tensor
    left_image: torch.Tensor
    right_image: torch.Tensor
    config: DepthEstimationPipelineConfig
    frame_index: int


def _check_sgm_keywords(paths: Any, p1: Any, p2: Any, uniqueness: Any) -> None:
    for name, v in (("sgm_paths", paths), ("sgm_p1", p1), ("sgm_p2", p2), ("sgm_uniqueness", uniqueness)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{name} must be an int")
    if paths not in (4, 8):
        raise ValueError(f"sgm_paths must be 4 or 8, got {paths}")
    if not 0 <= p1 <= p2 <= 191:
        raise ValueError(f"need 0 <= sgm_p1 <= sgm_p2 <= 191, got {p1}, {p2}")
    if not 0 <= uniqueness <= 99:
        raise ValueError(f"sgm_uniqueness must be in 0..99 (percent, 0: off), got {uniqueness}")


def _make_backend(config: DepthEstimationPipelineConfig, sgm: dict, **post: Any) -> StereoMatching:
    name = config.stereo_matching_backend
    if name == "cuda":
        return CudaStereoMatchingBackend(configuration=config.engine_configuration(),
                                         left_right_check=config.left_right_check, lr_max_diff=config.lr_max_diff,
                                         invalid_disparity=config.invalid_disparity, **post)
    if name == "sgm":
        return SgmStereoMatchingBackend(config.image_shape, config.min_disparity, config.max_disparity, **sgm,
                                        left_right_check=config.left_right_check, lr_max_diff=config.lr_max_diff,
                                        invalid_disparity=config.invalid_disparity, **post)
    if name in AVAILABLE_DNN_BACKENDS:
        raise RuntimeError(f"Stereo matching backend '{name}' (traced DNN) is not part of this build; use 'cuda'.")
    raise RuntimeError(f"Unsupported stereo matching backend: {name}")


class DepthEstimationPipeline:
    _track_camera = False                                            # off unless __init__ turns it on

    def __init__(self, config: Optional[DepthEstimationPipelineConfig] = None, *, speckle_max_size: int = 0,
                 speckle_max_diff: float = 1.0, fill_invalid: bool = False, median_radius: int = 0,
                 median_sigma_color: float = 10.0, median_sigma_space: float = 5.0, wls_lambda: float = 0.0,
                 wls_sigma_color: float = 1.5, wls_iterations: int = 3, confidence: bool = False,
                 confidence_lr_scale: float = 1.0, confidence_radius: int = 2, confidence_texture_scale: float = 10.0,
                 temporal: bool = False, temporal_motion_radius: int = 1, temporal_motion_threshold: float = 4.0,
                 temporal_decay: float = 0.8, temporal_max_diff: float = 1.0, temporal_max_weight: float = 8.0,
                 temporal_min_weight: float = 0.25,
                 rectification: Optional["cuda_depth.StereoRectification"] = None, sgm_paths: int = 8,
                 sgm_p1: int = 10, sgm_p2: int = 120, sgm_uniqueness: int = 0, reprojection_matrix=None,
                 point_cloud_depth_range: Tuple[float, float] = (0.0, math.inf), point_cloud_voxel_size: float = 0.0,
                 point_cloud_min_points: int = 1, point_cloud_min_confidence: float = 0.0,
                 tsdf_volume: Optional["cuda_depth.TSDFVolume"] = None,
                 right_view_synthesis: Optional[RightViewSynthesis] = None, render_model: bool = False,
                 track_camera: bool = False, initial_pose=None, tracking_args: Optional[dict] = None,
                 follow_camera: bool = False, follow_threshold: Optional[int] = None,
                 follow_anchor: Tuple[float, float, float] = (0.5, 0.5, 0.5), keep_spill: bool = False,
                 spill_store: Optional["cuda_depth.TSDFSpillStore"] = None):
        """speckle_max_size / speckle_max_diff / fill_invalid / median_radius / median_sigma_color / median_sigma_space:
        post-processing of the backend's map, after the left-right check if configured
        (CudaStereoMatchingBackend); with the defaults the map is returned as computed.  wls_lambda /
        wls_sigma_color / wls_iterations: wls_lambda > 0 runs the image-guided weighted least squares filter after the
        speckle filter in place of the fill and the median (combining them raises ValueError).  confidence /
        confidence_lr_scale / confidence_radius / confidence_texture_scale: confidence=True computes the per-pixel
        confidence of the map after the speckle filter (cuda_depth.confidence_map: the left-right term with
        config.left_right_check, the texture term over the left gray plane with confidence_radius > 0), returns it as
        DepthEstimationResult.confidence_map and weighs the WLS filter's pixels by it.  temporal / temporal_motion_radius /
        temporal_motion_threshold / temporal_decay / temporal_max_diff / temporal_max_weight / temporal_min_weight:
        temporal=True runs the motion-gated temporal filter (cuda_depth.TemporalFilter) last, in place on the map, with
        its history carried across process() calls (reset_temporal() forgets it); with confidence=True the confidence
        map is the measurement's weight.  rectification: a
        cuda_depth.StereoRectification whose out_shape is config.image_shape; the raw frames are rectified on the GPU
        before matching and the pixels outside its left_valid mask become invalid_disparity (None: frames are taken as
        rectified).  sgm_paths / sgm_p1 / sgm_p2 / sgm_uniqueness: the tuning of the 'sgm' backend (4 or 8 paths,
        0 <= P1 <= P2 <= 191, uniqueness 0..99 percent, 0 = off), which matches at image_shape over min_disparity..
        max_disparity with the same post-processing; checked whatever the backend.  reprojection_matrix /
        point_cloud_depth_range / point_cloud_voxel_size / point_cloud_min_points / point_cloud_min_confidence: with a 4x4
        reprojection matrix Q (cuda_depth.reprojection_matrix), the final map (after the temporal filter) is reprojected
        to metric 3D points last (cuda_depth.reproject_to_3d: depth_range, and with confidence=True the confidence map
        and min_confidence), coloured from the left frame it was computed on (the rectified one with rectification=),
        then voxel-downsampled when point_cloud_voxel_size > 0 (cuda_depth.voxel_downsample with min_points), and
        returned as DepthEstimationResult.point_cloud; None (the default) changes nothing.  tsdf_volume: a caller-owned
        cuda_depth.TSDFVolume on the pipeline's device (needs reprojection_matrix); every process() call then takes a
        camera_pose and integrates the final map into it, with point_cloud_depth_range, the confidence map and
        point_cloud_min_confidence when confidence=True, and colour from the left frame the map was computed on.
        right_view_synthesis: a pipeline.synthesis.RightViewSynthesis whose full_resolution is the frames' size; a
        process() call without a right image then generates one from the left frame, as the reference's pipeline does,
        and matches against it (None: such a call raises).  render_model: True (needs tsdf_volume) renders the volume,
        after the frame was integrated, from the frame's camera_pose at the frame's shape with the volume's defaults
        (TSDFVolume.render) and returns the disparity map as DepthEstimationResult.model_disparity_map: the denoised,
        hole-filled counterpart of disparity_map.  The reprojection matrix must then be one whose ray does not depend on
        the disparity (every cuda_depth.reprojection_matrix).  False (the default) changes nothing.  track_camera /
        initial_pose / tracking_args: track_camera=True (needs tsdf_volume and such a reprojection matrix) makes the
        pipeline find the poses itself, and process() then takes no camera_pose: the first frame is integrated at
        initial_pose [4, 4] (default the identity); every later frame is tracked against the volume rendered from the
        last pose (TSDFVolume.track with point_cloud_depth_range, the confidence map and point_cloud_min_confidence, and
        tracking_args on top; a photometric_weight > 0 among them passes the left frame the map was computed on as the
        photometric term's image, which needs a colour volume; pyramid_levels and huber_delta among them read that term
        coarse to fine from intensity pyramids), its twelve pose values and its lost flag are read back
        -- one small device-to-host copy, hence one synchronisation, per frame -- and it is integrated at the tracked
        pose unless it is lost.  The result
        carries camera_pose and tracking_lost; reset_tracking() forgets the last pose.  follow_camera /
        follow_threshold / follow_anchor / keep_spill: follow_camera=True (needs tsdf_volume) lets the volume follow the
        camera: before a frame is integrated the volume is shifted in whole voxels so that the frame's pose -- the
        tracked one with track_camera=True, else the caller's camera_pose -- stays at its anchor point
        (TSDFVolume.follow with follow_threshold, default min(dims) // 8, and follow_anchor), so the next frame's model
        view is rendered from the shifted volume; a lost frame does not move it.  The result carries volume_shift and,
        with keep_spill=True, what left the volume as spilled_volumes (TSDFVolume.shift(spill=True): the caller's to
        extract or drop; shift itself does not fuse them back).  The volume then holds a spare copy of its state
        (twice the memory).  False (the default) changes nothing.  spill_store: a cuda_depth.TSDFSpillStore (needs
        follow_camera=True); the volume then follows through the store (TSDFSpillStore.follow), which keeps what leaves
        and merges it back when the camera returns to a place it left; the result carries restored_boxes, and
        spilled_volumes as before with keep_spill=True.  None (the default) changes nothing."""
        self._config = DepthEstimationPipelineConfig() if config is None else config
        _check_sgm_keywords(sgm_paths, sgm_p1, sgm_p2, sgm_uniqueness)
        self._reprojection_matrix = None
        if tsdf_volume is not None:
            if not isinstance(tsdf_volume, cuda_depth.TSDFVolume):
                raise TypeError("tsdf_volume must be a cuda_depth.TSDFVolume")
            if reprojection_matrix is None:
                raise ValueError("tsdf_volume needs reprojection_matrix")
            if tsdf_volume.device != torch.device("cuda", torch.cuda.current_device()):
                raise ValueError(f"tsdf_volume must be on the pipeline's device cuda:{torch.cuda.current_device()}, "
                                 f"got {tsdf_volume.device}")
            cuda_depth.projection_matrix(reprojection_matrix)
        self._tsdf_volume = tsdf_volume
        if not isinstance(render_model, bool):
            raise TypeError("render_model must be a bool")
        if render_model:
            if tsdf_volume is None:
                raise ValueError("render_model needs tsdf_volume")
            q = cuda_depth._check_q(reprojection_matrix)
            if (q[:3, 2] != 0).any() or q[3, 0] != 0 or q[3, 1] != 0:
                raise ValueError("render_model needs a reprojection_matrix whose ray does not depend on the disparity "
                                 "(cuda_depth.reprojection_matrix builds one)")
        self._render_model = render_model
        if not isinstance(track_camera, bool):
            raise TypeError("track_camera must be a bool")
        if not track_camera and (initial_pose is not None or tracking_args is not None):
            raise ValueError("initial_pose and tracking_args need track_camera=True")
        self._track_camera = track_camera
        self._tracking_args = dict(tracking_args or {})
        self._initial_pose = self._last_pose = None
        if track_camera:
            if tsdf_volume is None:
                raise ValueError("track_camera needs tsdf_volume")
            q = cuda_depth._check_q(reprojection_matrix)
            if (q[:3, 2] != 0).any() or q[3, 0] != 0 or q[3, 1] != 0:
                raise ValueError("track_camera needs a reprojection_matrix whose ray does not depend on the disparity "
                                 "(cuda_depth.reprojection_matrix builds one)")
            pose = np.eye(4) if initial_pose is None else initial_pose
            cuda_depth.world_to_camera_poses(pose)
            self._initial_pose = cuda_depth._host_matrices("initial_pose", pose, False)[0]
        for name, flag in (("follow_camera", follow_camera), ("keep_spill", keep_spill)):
            if not isinstance(flag, bool):
                raise TypeError(f"{name} must be a bool")
        if follow_camera and tsdf_volume is None:
            raise ValueError("follow_camera needs tsdf_volume")
        if not follow_camera and (follow_threshold is not None or keep_spill
                                  or tuple(follow_anchor) != (0.5, 0.5, 0.5)):
            raise ValueError("follow_threshold, follow_anchor and keep_spill need follow_camera=True")
        if follow_threshold is not None and (isinstance(follow_threshold, bool) or not isinstance(follow_threshold, int)
                                             or follow_threshold < 1):
            raise ValueError(f"follow_threshold must be a positive int, got {follow_threshold!r}")
        if spill_store is not None:
            if not isinstance(spill_store, cuda_depth.TSDFSpillStore):
                raise TypeError("spill_store must be a cuda_depth.TSDFSpillStore")
            if not follow_camera:
                raise ValueError("spill_store needs follow_camera=True")
        self._follow_camera, self._keep_spill, self._spill_store = follow_camera, keep_spill, spill_store
        self._follow_threshold, self._follow_anchor = follow_threshold, tuple(follow_anchor)
        if right_view_synthesis is not None and not isinstance(right_view_synthesis, RightViewSynthesis):
            raise TypeError("right_view_synthesis must be a pipeline.synthesis.RightViewSynthesis")
        self._right_view_synthesis = right_view_synthesis
        if reprojection_matrix is not None:
            self._reprojection_matrix = cuda_depth._check_q(reprojection_matrix)
            cuda_depth._check_reproject_params(point_cloud_min_confidence, point_cloud_depth_range,
                                               self._config.invalid_disparity)
            if point_cloud_voxel_size != 0:
                cuda_depth._check_voxel_params(point_cloud_voxel_size, point_cloud_min_points)
        sgm = dict(paths=sgm_paths, P1=sgm_p1, P2=sgm_p2, uniqueness=sgm_uniqueness)
        self._stereo_matching = _make_backend(self._config, sgm, speckle_max_size=speckle_max_size,
                                              speckle_max_diff=speckle_max_diff, fill_invalid=fill_invalid,
                                              median_radius=median_radius, median_sigma_color=median_sigma_color,
                                              median_sigma_space=median_sigma_space, wls_lambda=wls_lambda,
                                              wls_sigma_color=wls_sigma_color, wls_iterations=wls_iterations,
                                              confidence=confidence, confidence_lr_scale=confidence_lr_scale,
                                              confidence_radius=confidence_radius,
                                              confidence_texture_scale=confidence_texture_scale, temporal=temporal,
                                              temporal_motion_radius=temporal_motion_radius,
                                              temporal_motion_threshold=temporal_motion_threshold,
                                              temporal_decay=temporal_decay, temporal_max_diff=temporal_max_diff,
                                              temporal_max_weight=temporal_max_weight,
                                              temporal_min_weight=temporal_min_weight,
                                              rectification=rectification)
        self._point_cloud_depth_range = point_cloud_depth_range
        self._point_cloud_voxel_size = point_cloud_voxel_size
        self._point_cloud_min_points = point_cloud_min_points
        self._point_cloud_min_confidence = point_cloud_min_confidence
        print(f"Using '{self._config.stereo_matching_backend}' as stereo matching backend.")

    def reset_temporal(self) -> None:
        """Forgets the temporal filter's history (temporal=True), e.g. at a cut in the stream; a no-op otherwise."""
        self._stereo_matching.reset_temporal()

    def reset_tracking(self) -> None:
        """Forgets the last pose (track_camera=True): the next frame is integrated at initial_pose without tracking, as
        the first one was; a no-op otherwise.  The volume is the caller's and is not touched."""
        self._last_pose = None

    def get_configuration(self) -> DepthEstimationPipelineConfig:
        return self._config

    def process(self, left_image: torch.Tensor, right_image: Optional[torch.Tensor] = None, *,
                camera_pose=None) -> DepthEstimationResult:
        """One frame.  The returned disparity map aliases the engine's persistent output buffer
        (stereo_matching.cc:42): clone it before processing the next frame if it must survive.  With rectification=,
        the result's left_image / right_image are the rectified frames the map was computed on (out_shape, same
        geometry as the map; persistent buffers too), not the raw frames passed in.  With confidence=True the result's
        confidence_map aliases a persistent buffer in the same way.  Frames are matched (and rectified) as uint8 when
        both are uint8 and as float32 otherwise: a uint8 frame beside a float32 one is converted to float32 first.
        Without a right_image, and with right_view_synthesis, the right view is generated from the left frame first and
        returned as the result's right_image ([3, H, W] float32 in 0..255, the synthesiser's persistent buffer).
        camera_pose: the left camera's camera-to-world pose [4, 4] for this frame, required with tsdf_volume and
        refused without one; the final map is integrated into the volume on the current stream."""
        if self._track_camera:
            if camera_pose is not None:
                raise ValueError("camera_pose must not be given with track_camera=True: the pipeline tracks it")
        elif (camera_pose is None) != (self._tsdf_volume is None):
            raise ValueError("camera_pose is required with tsdf_volume" if camera_pose is None
                             else "camera_pose needs a pipeline with tsdf_volume")
        if camera_pose is not None:
            cuda_depth.world_to_camera_poses(camera_pose)
        if right_image is None and self._right_view_synthesis is None:
            raise RuntimeError("right_image is required: right-view synthesis (Deep3D) is not part of this build.")
        left_on_device = left_image.cuda()
        if right_image is None:
            with cuda_perf_clock("Right view generation", self._config.log_perf_time):
                right_image = self._right_view_synthesis.process(left_on_device)
        with cuda_perf_clock("Stereo matching", self._config.log_perf_time):
            disparity = self._stereo_matching.process(left_on_device, right_image)
        rectified = getattr(self._stereo_matching, "rectified_frames", lambda: None)()
        if rectified is not None:
            left_on_device, right_image = rectified
        confidence = getattr(self._stereo_matching, "confidence_map", lambda: None)()
        cloud = None
        if self._reprojection_matrix is not None:
            cloud = self._point_cloud(disparity, left_on_device, confidence)
        lost = None
        if self._track_camera:
            camera_pose, lost = self._track(disparity, confidence, left_on_device)
        shift, spilled, restored = (0, 0, 0), [], 0
        if self._follow_camera and not lost and self._spill_store is not None:
            shift, spilled, restored = self._spill_store.follow(self._tsdf_volume, camera_pose,
                                                                threshold=self._follow_threshold,
                                                                anchor=self._follow_anchor)
            if not self._keep_spill:
                spilled = []
        elif self._follow_camera and not lost:
            shift, spilled = self._tsdf_volume.follow(camera_pose, threshold=self._follow_threshold,
                                                      anchor=self._follow_anchor, spill=self._keep_spill)
        if self._tsdf_volume is not None and not lost:
            self._tsdf_volume.integrate(disparity, self._reprojection_matrix, camera_pose,
                                        image=self._colour_source(left_on_device), confidence=confidence,
                                        min_confidence=self._point_cloud_min_confidence,
                                        depth_range=self._point_cloud_depth_range,
                                        invalid_disparity=self._config.invalid_disparity)
        model = None
        if self._render_model:
            model = self._tsdf_volume.render(self._reprojection_matrix, camera_pose, tuple(disparity.shape[-2:]),
                                             normals=False, colors=False,
                                             invalid_disparity=self._config.invalid_disparity).disparity
        return DepthEstimationResult(left_image=left_on_device, right_image=right_image, disparity_map=disparity,
                                     confidence_map=confidence, point_cloud=cloud, model_disparity_map=model,
                                     camera_pose=camera_pose if self._track_camera else None, tracking_lost=lost,
                                     volume_shift=shift, spilled_volumes=spilled, restored_boxes=restored)

    def _track(self, disparity: torch.Tensor, confidence: Optional[torch.Tensor], left: torch.Tensor):
        """(pose [4, 4] float64, lost) of this frame: initial_pose for the first frame, else the frame tracked against
        the volume seen from the last pose; the last pose moves on unless tracking was lost.  left: the frame the map was
        computed on, the image of the photometric term where tracking_args ask for one."""
        if self._last_pose is None:
            self._last_pose = self._initial_pose.copy()
            return self._last_pose.copy(), False
        args = dict(confidence=confidence, min_confidence=self._point_cloud_min_confidence,
                    depth_range=self._point_cloud_depth_range, invalid_disparity=self._config.invalid_disparity)
        args.update(self._tracking_args)
        if args.get("photometric_weight", 0.0) > 0 and args.get("image") is None:
            if left.dtype != torch.uint8 and not (left.dtype == torch.float32 and left.dim() == 2):
                raise ValueError("the photometric term needs uint8 frames or a float32 gray frame, got "
                                 f"{left.dtype} {tuple(left.shape)}")
            args["image"] = left.contiguous()
        found = self._tsdf_volume.track(disparity, self._reprojection_matrix, self._last_pose, **args)
        packed = torch.cat([found.pose.reshape(-1), found.lost.reshape(1).to(torch.float32)]).cpu().numpy()
        lost = bool(packed[16] != 0)
        if not lost:
            self._last_pose = packed[:16].reshape(4, 4).astype(np.float64)
        return self._last_pose.copy(), lost

    def _point_cloud(self, disparity: torch.Tensor, left: torch.Tensor,
                     confidence: Optional[torch.Tensor]) -> "cuda_depth.PointCloud":
        """The final map's cloud, coloured from `left` ([3, H, W] or [H, W]; other dtypes than uint8 as float32)."""
        cloud = cuda_depth.reproject_to_3d(disparity, self._reprojection_matrix, image=self._colour_source(left),
                                           confidence=confidence, min_confidence=self._point_cloud_min_confidence,
                                           depth_range=self._point_cloud_depth_range,
                                           invalid_disparity=self._config.invalid_disparity)
        if self._point_cloud_voxel_size > 0:
            cloud = cuda_depth.voxel_downsample(cloud, self._point_cloud_voxel_size,
                                                min_points=self._point_cloud_min_points)
        return cloud

    @staticmethod
    def _colour_source(left: torch.Tensor) -> torch.Tensor:
        """`left` ([3, H, W] or [H, W]) as a colour source: uint8 and float32 as they are, other dtypes as float32."""
        image = left if left.dtype in (torch.uint8, torch.float32) else left.float()
        return image.contiguous()
