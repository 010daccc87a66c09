"""CPU restatement of the second half of DepthEstimationPipeline.process(): what happens to the final map after
pipeline_ref.PipelineRef's chain (steps 1 to 8 of INTEGRATION.md, "The pipeline's steps in order"), built only from the
twins of the single steps, in the order the DepthEstimationPipeline docstring states:

  9. the cloud (a reprojection matrix): points3d_ref.reproject_ref of the final map with depth_range, with the confidence
     map and min_confidence only when the chain computes a confidence, coloured from the left frame the map was computed
     on -- the rectified one with a rectification, else the frame as the caller passed it (uint8 and float32 as they are,
     anything else as float32) -- then points3d_ref.voxel_ref when voxel_size > 0;
 10. the pose (a volume): the caller's, or with track_camera the first frame's initial_pose and after it
     raycast_ref.raycast_ref of the volume from the last pose over the default render range (0 .. the distance from the
     float32 eye to the farthest corner of the volume where it stands now), then track_ref.track_ref with the frame's
     arguments and tracking_args on top; a lost frame keeps the last pose;
 11. the follow (follow_camera, not for a lost frame): tsdf_window_ref.follow_ref of the pose's position; the spill boxes
     (keep_spill) and the shifted state are tsdf_window_ref.window_state of the state before the shift; offset and origin
     as TSDFVolume keeps them (origin = the first origin + offset * voxel_size in float64);
 12. the integration (not for a lost frame): tsdf_ref.integrate_ref with the same image, confidence, min_confidence,
     depth_range and invalid_disparity;
 13. the model map (render_model): raycast_ref of the state after the integration from the frame's pose.

Nothing from pipeline/ is imported, nor the TSDFVolume class."""
from __future__ import annotations

import math

import numpy as np

import points3d_ref
import raycast_ref as rc
import track_ref as tr
import tsdf_ref
import tsdf_window_ref as wr
from pipeline_ref import PipelineRef

F = np.float32
TRACK_MIN_PIVOT = 1e-3          # cuda_depth.track_camera's default min_pivot (track_ref's own default differs)
SPILL_MARGIN = 1                # TSDFVolume.shift's default margin
TRACK_KEYS = {"schedule", "max_distance", "depth_range", "min_inliers", "min_confidence", "invalid_disparity", "min_pivot",
              "rot_eps", "trans_eps", "confidence", "min_weight"}   # min_weight: of TSDFVolume.track's rendering


def colour_source(a) -> np.ndarray:
    """A left frame as a colour source: uint8 and float32 as they are, other dtypes as float32."""
    a = np.asarray(a)
    return np.ascontiguousarray(a if a.dtype in (np.uint8, np.float32) else a.astype(F))


def pose64(pose) -> np.ndarray:
    return np.array(pose, np.float64).reshape(4, 4)


class Pipeline3DRef:
    """The whole of process() with the pipeline's keywords.  chain: the PipelineRef of the first half (it knows
    invalid_disparity and whether there is a confidence).  volume: None or a dict of dims, voxel_size, origin and
    optionally truncation, max_weight, color -- the TSDFVolume the pipeline is given, empty.  process(left, right,
    camera_pose=None) returns a dict: disparity, confidence, left (the rectified left frame or None), cloud (dict of
    points, colors, indices, counts; None without Q), pose, lost (None unless tracked), shift, spilled (a list of states
    with offset and origin), model (or None) and state (tsdf, weight, color, offset, origin; arrays are copies)."""

    def __init__(self, chain: PipelineRef, *, reprojection_matrix=None, point_cloud_depth_range=(0.0, math.inf),
                 point_cloud_voxel_size: float = 0.0, point_cloud_min_points: int = 1,
                 point_cloud_min_confidence: float = 0.0, volume=None, render_model: bool = False,
                 track_camera: bool = False, initial_pose=None, tracking_args=None, follow_camera: bool = False,
                 follow_threshold=None, follow_anchor=(0.5, 0.5, 0.5), keep_spill: bool = False):
        self.chain = chain
        self.inv = float(chain.inv)
        self.Q = None if reprojection_matrix is None else np.asarray(reprojection_matrix, F).reshape(4, 4)
        self.depth_range = tuple(point_cloud_depth_range)
        self.voxel = (float(point_cloud_voxel_size), int(point_cloud_min_points))
        self.min_confidence = float(point_cloud_min_confidence)
        self.volume = None
        if volume is not None:
            assert self.Q is not None
            self.dims = tuple(int(v) for v in volume["dims"])
            self.vs = float(volume["voxel_size"])
            self.origin0 = tuple(float(v) for v in volume["origin"])
            self.truncation = float(volume.get("truncation", 3.0 * self.vs))
            self.max_weight = float(volume.get("max_weight", 64.0))
            self.offset = (0, 0, 0)
            self.volume = tsdf_ref.empty_state(self.dims, bool(volume.get("color", True)))
            self.P = tsdf_ref.projection(self.Q)
        assert volume is not None or not (render_model or track_camera or follow_camera)
        self.render_model, self.track, self.follow, self.keep_spill = render_model, track_camera, follow_camera, keep_spill
        self.initial_pose = pose64(np.eye(4) if initial_pose is None else initial_pose)
        self.tracking_args = dict(tracking_args or {})
        assert set(self.tracking_args) <= TRACK_KEYS, "TSDFVolume.track's other render arguments are not restated here"
        self.follow_threshold, self.follow_anchor = follow_threshold, tuple(follow_anchor)
        self.last_pose = None

    # ------------------------------------------------------------------ the volume where it stands
    @property
    def origin(self):
        return wr.origin_ref(self.origin0, self.offset, self.vs)

    def render_range(self, pose):
        """TSDFVolume.render's default depth_range: 0 .. the float64 distance from the float32 eye to the farthest corner."""
        lo = np.asarray(self.origin, np.float64)
        hi = lo + np.asarray(self.dims, np.float64) * self.vs
        corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        eye = rc.view_pose(pose)[0][:, 3].astype(np.float64)
        return (0.0, float(np.linalg.norm(corners - eye, axis=1).max()))

    def _raycast(self, pose, shape, min_weight=1.0):
        return rc.raycast_ref(self.volume, self.dims, self.origin, self.vs, self.Q, rc.view_pose(pose), shape,
                              min_weight=min_weight, depth_range=self.render_range(pose), invalid_disparity=self.inv)

    def _snapshot(self, state, offset):
        out = {k: None if v is None else v.copy() for k, v in state.items()}
        out["offset"], out["origin"] = tuple(offset), wr.origin_ref(self.origin0, offset, self.vs)
        return out

    # ------------------------------------------------------------------ the steps
    def _cloud(self, d, conf, src):
        points, colors, indices, offsets, _ = points3d_ref.reproject_ref(
            d[None], self.Q, image=src[None], confidence=None if conf is None else conf[None],
            min_confidence=self.min_confidence, depth_range=self.depth_range, invalid_disparity=self.inv)
        cloud = {"points": points, "colors": colors, "indices": indices, "counts": None}
        if self.voxel[0] > 0:
            points, colors, counts, _, _ = points3d_ref.voxel_ref(points, colors, offsets, self.voxel[0], self.voxel[1])
            cloud = {"points": points, "colors": colors, "indices": None, "counts": counts}
        return cloud

    def _track(self, d, conf):
        if self.last_pose is None:
            self.last_pose = self.initial_pose.copy()
            return self.last_pose.copy(), False
        args = dict(confidence=conf, min_confidence=self.min_confidence, depth_range=self.depth_range,
                    invalid_disparity=self.inv, min_pivot=TRACK_MIN_PIVOT)
        args.update(self.tracking_args)
        view = self._raycast(self.last_pose, d.shape, args.pop("min_weight", 1.0))
        model = tr.model_view(view["depth"][0], view["normals"][0], self.Q, self.last_pose)
        got = tr.track_ref(d, self.Q, rc.view_pose(self.last_pose)[0], model, **args)
        lost = bool(got["info"][0])
        if not lost:
            self.last_pose = np.vstack([got["pose"].astype(np.float64), [0.0, 0.0, 0.0, 1.0]])
        return self.last_pose.copy(), lost

    def _follow(self, pose):
        d = wr.follow_ref(pose[:3, 3].tolist(), self.origin, self.dims, self.vs, self.follow_threshold, self.follow_anchor)
        if d == (0, 0, 0):
            return d, []
        spilled = []
        if self.keep_spill:
            for start, size in wr.spill_boxes_ref(self.dims, d, SPILL_MARGIN):
                box = self._snapshot(wr.window_state(self.volume, start, size), [o + s for o, s in zip(self.offset, start)])
                box["dims"] = tuple(size)
                spilled.append(box)
        self.volume = wr.window_state(self.volume, d, self.dims)
        self.offset = tuple(o + c for o, c in zip(self.offset, d))
        return d, spilled

    def _colour_of(self, left, rect_l):
        """The colour source of the cloud and the volume: the left frame the map was computed on."""
        return colour_source(left if rect_l is None else rect_l)

    def _integrate(self, d, conf, src, pose) -> None:
        tsdf_ref.integrate_ref(self.volume, self.dims, self.origin, self.vs, self.truncation, self.max_weight, d[None],
                               self.Q, self.P, tsdf_ref.world_to_camera(pose),
                               image=src[None] if self.volume["color"] is not None else None,
                               confidence=None if conf is None else conf[None], min_confidence=self.min_confidence,
                               depth_range=self.depth_range, invalid_disparity=self.inv)

    def process(self, left, right, camera_pose=None) -> dict:
        d, conf, rect_l, _ = self.chain.process(left, right)
        out = {"disparity": d, "confidence": conf, "left": rect_l, "cloud": None, "pose": None, "lost": None,
               "shift": (0, 0, 0), "spilled": [], "model": None, "state": None}
        src = self._colour_of(left, rect_l)
        if self.Q is not None:
            out["cloud"] = self._cloud(d, conf, src)
        if self.volume is None:
            return out
        lost = None
        if self.track:
            assert camera_pose is None
            pose, lost = self._track(d, conf)
            out["pose"], out["lost"] = pose, lost
        else:
            pose = pose64(camera_pose)
        if self.follow and not lost:
            out["shift"], out["spilled"] = self._follow(pose)
        if not lost:
            self._integrate(d, conf, src, pose)
        if self.render_model:
            out["model"] = self._raycast(pose, d.shape)["disparity"][0]
        out["state"] = self._snapshot(self.volume, self.offset)
        return out

    def reset_temporal(self) -> None:
        self.chain.reset_temporal()

    def reset_tracking(self) -> None:
        self.last_pose = None
