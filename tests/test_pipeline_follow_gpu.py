"""DepthEstimationPipeline(follow_camera=True) on the device: along a path that leaves the volume's first window, a
pipeline whose volume follows the camera tracks every frame, reports its shifts and hands back what left; the same
pipeline without follow_camera loses the camera at the volume's edge -- the failure the option removes -- and is, result
by result, the pipeline built without the new keywords.  The frames' maps are the analytic scene's exact disparities
(tests/tsdf_follow_cases.py), not matched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import tsdf_follow_cases as fc                      # noqa: E402

FRAMES, START, STEP = 24, (0.0, 0.0, 1.0), (0.03, 0.0, 0.15)        # 3.45 m forward: past the first window's front face


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def run(cd, frames=FRAMES, colour=True, **keywords):
    """The results of the sequence's frames through a pipeline with `keywords`, and its volume."""
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    poses, maps, images = fc.path_frames(frames, START, STEP)
    cfg = DepthEstimationPipelineConfig(image_shape=(fc.FRAME_H, fc.FRAME_W), min_disparity=0, max_disparity=15,
                                        stereo_matching_backend="cuda")
    vol = cd.TSDFVolume(fc.PIPE_DIMS, fc.VS, fc.PIPE_ORIGIN, color=colour)
    pipe = DepthEstimationPipeline(cfg, reprojection_matrix=fc.q_matrix(cd), tsdf_volume=vol,
                                   point_cloud_depth_range=fc.DEPTH_RANGE, track_camera=True, initial_pose=poses[0],
                                   tracking_args=fc.TRACKING, **keywords)
    feed = iter([torch.from_numpy(m).cuda() for m in maps])
    pipe._stereo_matching.process = lambda left, right: next(feed)    # the maps are the sequence's, not matched
    results = []
    for img in images:
        frame = torch.from_numpy(img)
        res = pipe.process(frame, frame)
        results.append((res, int(vol.weight.count_nonzero().item()), vol.weight.sum().item()))
    return results, vol, poses


def test_a_following_volume_keeps_the_camera(cd):
    results, vol, poses = run(cd, follow_camera=True, follow_anchor=fc.PIPE_ANCHOR, keep_spill=True)
    assert [r.tracking_lost for r, _, _ in results] == [False] * FRAMES
    shifts = [r.volume_shift for r, _, _ in results]
    assert all(isinstance(s, tuple) and len(s) == 3 and all(type(c) is int for c in s) for s in shifts)
    moved = [s for s in shifts if s != (0, 0, 0)]
    assert len(moved) >= 2, f"the path must move the volume at least twice, got {shifts}"
    assert tuple(sum(s[a] for s in shifts) for a in range(3)) == vol.offset
    assert vol.offset[2] >= 20 and shifts[0] == (0, 0, 0)
    threshold = min(fc.PIPE_DIMS) // 8
    assert all(max(abs(c) for c in s) >= threshold for s in moved)
    for (res, _, _), s in zip(results, shifts):                       # keep_spill: one box per moved axis, else none
        assert len(res.spilled_volumes) == sum(c != 0 for c in s)
        assert all(isinstance(b, cd.TSDFVolume) and b.voxel_size == fc.VS for b in res.spilled_volumes)
    spilled = [b for res, _, _ in results for b in res.spilled_volumes]
    assert any(int(b.weight.count_nonzero().item()) > 0 for b in spilled), "what left the volume was measured space"
    # the tracked poses stay on the path: within two voxels (less than the truncation band) of the true positions
    # over 3.45 m -- a sanity bound on the sequence, not a statement of the tracker's accuracy
    err = max(np.linalg.norm(r.camera_pose[:3, 3] - p[:3, 3]) for (r, _, _), p in zip(results, poses))
    assert err < 2 * fc.VS, f"the tracked path is {err:.3f} m off"
    # the camera is still where the volume's anchor is
    anchor = np.asarray(vol.origin) + np.asarray(fc.PIPE_ANCHOR) * np.asarray(fc.PIPE_DIMS) * fc.VS
    assert np.abs((results[-1][0].camera_pose[:3, 3] - anchor) / fc.VS).max() < threshold + 0.5


def test_without_following_the_camera_is_lost_at_the_edge(cd):
    """Today's behaviour, which follow_camera removes: the volume stays, the camera leaves it."""
    results, vol, poses = run(cd, colour=False, follow_camera=False)
    assert vol.offset == (0, 0, 0) and vol.origin == fc.PIPE_ORIGIN
    front = fc.PIPE_ORIGIN[2] + fc.PIPE_DIMS[2] * fc.VS
    past = [f for f in range(FRAMES) if poses[f][2, 3] > front]
    assert past, "the path must leave the volume"
    failed = []
    for f in past:
        res, measured, total = results[f]
        failed.append(bool(res.tracking_lost) or (measured, total) == results[f - 1][1:])
    assert any(failed), "a frame past the volume's edge was tracked and integrated"
    assert all(r.volume_shift == (0, 0, 0) and r.spilled_volumes == [] for r, _, _ in results)


def test_defaults_are_unchanged(cd):
    """follow_camera=False is the pipeline built without the new keywords: the same poses, flags and volume."""
    frames = 8
    a, vol_a, _ = run(cd, frames, follow_camera=False)
    b, vol_b, _ = run(cd, frames)
    for (ra, ma, ta), (rb, mb, tb) in zip(a, b):
        assert ra.tracking_lost is rb.tracking_lost and np.array_equal(ra.camera_pose, rb.camera_pose)
        assert (ma, ta) == (mb, tb)
        assert ra.volume_shift == rb.volume_shift == (0, 0, 0) and ra.spilled_volumes == rb.spilled_volumes == []
        assert ra.model_disparity_map is None and ra.point_cloud is not None
    for name in ("tsdf", "weight", "color"):
        ta, tb = getattr(vol_a, name), getattr(vol_b, name)
        assert torch.equal(ta.view(torch.int32), tb.view(torch.int32)), name
    assert vol_a._spare is None and vol_a.offset == (0, 0, 0)


def test_argument_errors(cd):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    cfg = DepthEstimationPipelineConfig(image_shape=(fc.FRAME_H, fc.FRAME_W), min_disparity=0, max_disparity=15)
    Q = fc.q_matrix(cd)
    vol = cd.TSDFVolume(fc.PIPE_DIMS, fc.VS, fc.PIPE_ORIGIN, color=False)
    with pytest.raises(ValueError, match="follow_camera needs tsdf_volume"):
        DepthEstimationPipeline(cfg, reprojection_matrix=Q, follow_camera=True)
    with pytest.raises(ValueError, match="follow_camera=True"):
        DepthEstimationPipeline(cfg, reprojection_matrix=Q, tsdf_volume=vol, keep_spill=True)
    with pytest.raises(ValueError, match="follow_threshold"):
        DepthEstimationPipeline(cfg, reprojection_matrix=Q, tsdf_volume=vol, follow_camera=True, follow_threshold=0)
    with pytest.raises(TypeError, match="keep_spill"):
        DepthEstimationPipeline(cfg, reprojection_matrix=Q, tsdf_volume=vol, follow_camera=True, keep_spill=1)
    # with the caller's poses instead of tracked ones, the caller's pose is what the volume follows
    pipe = DepthEstimationPipeline(cfg, reprojection_matrix=Q, tsdf_volume=vol, follow_camera=True, follow_threshold=2,
                                   point_cloud_depth_range=fc.DEPTH_RANGE)
    poses, maps, images = fc.path_frames(3, START, (0.0, 0.0, 0.375))
    feed = iter([torch.from_numpy(m).cuda() for m in maps])
    pipe._stereo_matching.process = lambda left, right: next(feed)
    got = [pipe.process(torch.from_numpy(i), torch.from_numpy(i), camera_pose=p).volume_shift for i, p in zip(images, poses)]
    assert got == [(0, 0, -8), (0, 0, 3), (0, 0, 3)] and vol.offset == (0, 0, -2)
