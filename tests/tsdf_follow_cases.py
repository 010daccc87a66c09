"""Shared cases of the tests of a TSDF volume that follows the camera (tests/test_tsdf_window_gpu.py,
tests/test_pipeline_follow_gpu.py): an analytic corridor scene (tests/tsdf_ref.py), small exact frames of it along a
straight path, and volumes whose voxel size and origins are multiples of 0.125, so that every voxel centre is exact in
float32 however the volume's origin was reached."""
import functools

import numpy as np

import tsdf_ref as ref

VS = 0.125
FRAME_H, FRAME_W, FX, BASE = 60, 80, 50.0, 0.2                    # +-38 degrees wide: the walls are in view
CX, CY = (FRAME_W - 1) / 2.0, (FRAME_H - 1) / 2.0
DEPTH_RANGE = (0.2, 8.0)

# a large fixed volume and a small one inside it that follows the camera
BIG_DIMS, BIG_ORIGIN = (96, 32, 96), (-6.0, -2.0, 0.0)
SMALL_DIMS, SMALL_AT = (48, 32, 48), (24, 0, 0)                      # the small volume's first voxel in the large one
SMALL_ORIGIN = tuple(o + a * VS for o, a in zip(BIG_ORIGIN, SMALL_AT))

# the pipeline's volume: 4 x 3 x 4 m with the camera a metre inside its rear face
PIPE_DIMS, PIPE_ORIGIN, PIPE_ANCHOR = (32, 24, 32), (-2.0, -1.5, 0.0), (0.5, 0.5, 0.25)
# a frame of 60 x 80 leaves stride 4 some 300 samples, too few of them inliers: the schedule starts at stride 2
TRACKING = dict(schedule=((2, 5), (1, 10)), max_distance=0.3, min_inliers=100)
# render and track after a shift: a volume with the camera 1.5 m inside its rear face, and short steps
VIEW_ORIGIN, VIEW_START, VIEW_STEP = (-3.0, -2.0, 1.5), (0.0, 0.0, 3.0), (0.03, 0.0, 0.15)


def scene() -> ref.Scene:
    """A corridor: a ground plane 0.6 below the path, a wall on either side (what holds the camera sideways) and boxes
    on both sides of the path and across it, every 0.8 m from z = 2.4 to 12."""
    boxes = [((-1.5, -1.5, -1.0), (-1.3, 0.6, 14.0)), ((1.6, -1.5, -1.0), (1.8, 0.6, 14.0))]
    for k in range(12):
        z = 2.4 + 0.8 * k
        side = (-1.0, 0.9, -0.2, 1.5)[k % 4] + 0.12 * k                 # drifts right with the path
        top = (-0.3, 0.0, 0.2, -0.1)[k % 4]
        boxes.append(((side - 0.4, top, z), (side + 0.4, 0.6, z + 0.5)))
    return ref.Scene(ground_y=0.6, boxes=boxes)


def q_matrix(cd):
    return cd.reprojection_matrix(FX, CX, CY, BASE)


@functools.lru_cache(maxsize=None)
def path_frames(count, start=(0.0, 0.0, 3.0), step=(0.15, 0.0, 0.3), seed=29):
    """(poses [count, 4, 4] float64, exact disparity maps [count, H, W] f32, u8 RGB frames [count, 3, H, W]) of cameras
    that look along +z from start + f * step."""
    sc, rng = scene(), np.random.default_rng(seed)
    poses, maps, images = [], [], []
    for f in range(count):
        pose = np.eye(4)
        pose[:3, 3] = [s + f * d for s, d in zip(start, step)]
        poses.append(pose)
        maps.append(sc.render(pose, FRAME_H, FRAME_W, FX, CX, CY, BASE))
        images.append(rng.integers(0, 256, (3, FRAME_H, FRAME_W)).astype(np.uint8))
    return np.stack(poses), np.stack(maps), np.stack(images)
