"""DepthEstimationPipeline.process() as a whole against the composed CPU twins (pipeline3d_ref.Pipeline3DRef), bit for bit
after every frame: the disparity and confidence maps and the rectified left frame, the point cloud, the tracked pose and
its lost flag, the volume's shift and what it spilled, the model map and the volume itself.  One pipeline object per case
runs the case's frames with the real matcher; nothing is replaced.

The cases are pipeline3d_cases' pairwise covering set; tests/test_pipeline3d_ref_cpu.py checks on the CPU that they cover
every pair and that none is vacuous.  Each case runs four frames of a camera moving through a corridor, one flat frame
that cannot be tracked (and must change nothing), two more frames, then reset_tracking() and reset_temporal() and the
first view again.  One case is run a second time on a side stream.

There is no full-size case: raycast_ref and track_ref take minutes in NumPy at 375 x 1242, and the production sizes of
every stage are covered one by one in tests/test_scale_gpu.py.  No graph capture either: track_camera synchronises by
design."""
import numpy as np
import pytest

import pipeline3d_cases as pc
from test_pipeline_chain_gpu import assert_bitwise, assert_frame

torch = pytest.importorskip("torch")

FLAT_AT = pc.ORDER.index(pc.FLAT)
STREAM_CASE = next(i for i, c in enumerate(pc.CASES) if c["poses"] == "tracked" and c["follow"] == "spill")


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def assert_equal(got, expect, what):
    """Integer arrays (colours, indices, counts): the same dtype, shape and values."""
    got = got.cpu().numpy()
    assert got.dtype == expect.dtype and got.shape == expect.shape, (what, got.dtype, got.shape, expect.dtype, expect.shape)
    bad = np.argwhere(got != expect)
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first at {tuple(bad[0])}: " \
                          f"{got[tuple(bad[0])]} vs {expect[tuple(bad[0])]}"


def assert_state(vol, expect, what):
    """A TSDFVolume (the pipeline's, or a spilled box) against a reference state."""
    assert_bitwise(vol.tsdf, expect["tsdf"], f"{what}: tsdf")
    assert_bitwise(vol.weight, expect["weight"], f"{what}: weight")
    if expect["color"] is None:
        assert vol.color is None, what
    else:
        assert_equal(vol.color, expect["color"], f"{what}: color")
    assert vol.offset == expect["offset"] and all(type(c) is int for c in vol.offset), (what, vol.offset, expect["offset"])
    assert vol.origin == expect["origin"], (what, vol.origin, expect["origin"])


def build(cd, case):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    cfg = DepthEstimationPipelineConfig(image_shape=(pc.H, pc.W), min_disparity=pc.DMIN, max_disparity=pc.DMAX,
                                        invalid_disparity=case["inv"], stereo_matching_backend=case["backend"],
                                        left_right_check=case["lrconf"], lr_max_diff=pc.LR_MAX_DIFF)
    rectification = None
    if case["rect"]:
        left_map, right_map, in_shape = pc.rectification()
        rectification = cd.StereoRectification(left_map, right_map, in_shape, (pc.H, pc.W))
    vol = cd.TSDFVolume(**pc.volume_keywords(case))
    pipe = DepthEstimationPipeline(cfg, rectification=rectification, tsdf_volume=vol, **pc.chain_keywords(case),
                                   **pc.pipeline_keywords(case))
    return pipe, vol


def check_frame(pipe, vol, case, left, right, pose, expect, what):
    tracked = case["poses"] == "tracked"
    before = (vol.tsdf.clone(), vol.weight.clone(), None if vol.color is None else vol.color.clone(), vol.offset, vol.origin)
    res = pipe.process(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), camera_pose=pose)
    assert_bitwise(res.disparity_map, expect["disparity"], f"{what}: disparity")
    if expect["confidence"] is None:
        assert res.confidence_map is None, what
    else:
        assert_bitwise(res.confidence_map, expect["confidence"], f"{what}: confidence")
    if expect["left"] is not None:
        assert_frame(res.left_image, expect["left"], f"{what}: rectified left")
    cloud, want = res.point_cloud, expect["cloud"]
    assert cloud.points.shape[0] == want["points"].shape[0], (what, cloud.points.shape, want["points"].shape)
    assert_bitwise(cloud.points, want["points"], f"{what}: cloud points")
    assert_equal(cloud.colors, want["colors"], f"{what}: cloud colours")
    if want["counts"] is None:
        assert cloud.counts is None, what
        assert_equal(cloud.indices, want["indices"], f"{what}: cloud indices")
    else:
        assert_equal(cloud.counts, want["counts"], f"{what}: cloud counts")
    if tracked:
        assert res.tracking_lost is expect["lost"], (what, res.tracking_lost, expect["lost"])
        got = res.camera_pose
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (4, 4), what
        assert np.array_equal(got.view(np.uint64), expect["pose"].view(np.uint64)), f"{what}: pose\n{got}\n{expect['pose']}"
    else:
        assert res.tracking_lost is None and res.camera_pose is None, what
    shift = res.volume_shift
    assert isinstance(shift, tuple) and len(shift) == 3 and all(type(c) is int for c in shift), (what, shift)
    assert shift == expect["shift"], (what, shift, expect["shift"])
    assert len(res.spilled_volumes) == len(expect["spilled"]), (what, len(res.spilled_volumes))
    for b, (box, want_box) in enumerate(zip(res.spilled_volumes, expect["spilled"])):
        assert box.dims == want_box["dims"] and box.voxel_size == pc.VS, (what, b, box.dims)
        assert_state(box, want_box, f"{what}: spilled box {b}")
    if expect["model"] is None:
        assert res.model_disparity_map is None, what
    else:
        assert_bitwise(res.model_disparity_map, expect["model"], f"{what}: model map")
    assert_state(vol, expect["state"], f"{what}: volume")
    if expect["lost"]:                                               # what a lost frame must not touch
        assert torch.equal(vol.tsdf.view(torch.int32), before[0].view(torch.int32)), what
        assert torch.equal(vol.weight.view(torch.int32), before[1].view(torch.int32)), what
        assert before[2] is None or torch.equal(vol.color, before[2]), what
        assert (vol.offset, vol.origin) == before[3:] and shift == (0, 0, 0) and res.spilled_volumes == [], what
    return res


def run_case(cd, index):
    case, expected = pc.CASES[index], pc.expected(index)
    pipe, vol = build(cd, case)
    frames = pc.case_frames(case)
    last_pose = None
    for k, ((left, right), expect) in enumerate(zip(frames, expected)):
        if k == len(pc.ORDER):
            pipe.reset_tracking()
            pipe.reset_temporal()
        res = check_frame(pipe, vol, case, left, right, pc.given_pose(case, k), expect,
                          f"frame {k}" + (" (after the resets)" if k == len(pc.ORDER) else ""))
        if case["poses"] == "tracked":
            if k == FLAT_AT:
                assert res.tracking_lost and np.array_equal(res.camera_pose, last_pose), "a lost frame keeps the last pose"
            last_pose = res.camera_pose.copy()


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(pc.CASES)), ids=pc.IDS)
def test_pipeline_matches_the_composed_twins(cd, index):
    run_case(cd, index)


@pytest.mark.gpu
def test_the_same_bits_on_a_side_stream(cd):
    """A tracked, following, spilling case once more with everything enqueued on a side stream."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_case(cd, STREAM_CASE)
    torch.cuda.current_stream().wait_stream(side)
