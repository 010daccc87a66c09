"""Cases of the tests of DepthEstimationPipeline.process() as a whole (tests/test_pipeline3d_ref_cpu.py,
tests/test_pipeline3d_chain_gpu.py): stereo frames of a 3D scene, so that the real matcher's maps can be tracked and fused,
and a pairwise covering set of the pipeline's options.

The scene is tsdf_follow_cases' corridor, closed by a ceiling and an end wall so that every ray hits something.  A frame
is the scene seen from the left pose and from the right camera -- the left pose moved by the baseline along its x axis --
each pixel coloured by one procedural texture of the world point its ray hits: seeded value noise of the quantised world
coordinates in three octaves, three channels, rounded to 0..255.  Both views therefore agree wherever they see the same
surface.  Every frame gets fresh +-2 noise.  With a rectification the raw frames are the same views sampled through the
inverse of a mild affine map (a rotation of up to 0.01 rad, a scale of 0.97..1, a shift), so that rectifying them gives the
views back up to the remap's interpolation.  One frame of every sequence is a pair of flat gray images: nothing in it can
be matched to a depth, so no pixel becomes a point and the tracker must call it lost."""
import functools

import numpy as np

import rectify_ref
import tsdf_follow_cases as fc
import tsdf_ref
from pairwise import pairwise_cases
from pipeline3d_ref import Pipeline3DRef
from pipeline_ref import PipelineRef

F = np.float32
H, W = 48, 96
DMIN, DMAX = 0, 15
FX, BASE = 50.0, 0.4                                                 # d = 20 / Z: 15.6 at the nearest ground, 3.3 at 6 m
CX, CY = (W - 1) / 2.0, (H - 1) / 2.0
RAW_H, RAW_W = H + 6, W + 10                                         # raw frames of the rectified cases
VS = 0.25
DIMS = (16, 12, 36)                                                  # 4 x 3 x 9 m: the corridor's walls are 0.2 m inside
START = (0.0, 0.0, 1.0)
ANCHOR = (0.5, 0.5, 0.25)                                            # where the first camera stands in the volume
ORIGIN = tuple(s - a * n * VS for s, a, n in zip(START, ANCHOR, DIMS))
DEPTH_RANGE = (0.2, 6.5)
FRAMES = 6                                                           # poses of the path
FLAT = -1                                                            # stands for the untrackable frame in a sequence
STEP = (0.05, 0.0, 0.06)                                             # metres per frame
TURN = np.radians([0.3, 0.8, -0.2])                                  # rotation about x, y, z per frame
FOLLOW_THRESHOLD = 1                                                 # voxels: the volume moves once the camera is half a voxel off
LR_MAX_DIFF = 3.0                                                    # lr_max_diff of the cases with the LR check
LR_SCALE = 3.3                                                       # confidence_lr_scale: 3 px off is 0.09 < min_confidence 0.1
SUPERSAMPLE = 3                                                      # rays per pixel and axis
OCTAVES = ((0.72, 0.25), (0.24, 0.35), (0.08, 0.4))                    # the texture's (cell size in metres, share)
TRACKING = dict(schedule=((2, 5), (1, 10)), max_distance=0.15, min_inliers=100, min_weight=0.5)
TEMPORAL = dict(temporal_motion_radius=1, temporal_motion_threshold=4.0, temporal_decay=0.75, temporal_max_diff=1.0,
                temporal_max_weight=6.0, temporal_min_weight=0.25)
FILTERS = {"none": {}, "fill": dict(fill_invalid=True), "wls1": dict(wls_lambda=200.0, wls_iterations=1)}
VOXEL = dict(point_cloud_voxel_size=0.1, point_cloud_min_points=2)
FOLLOW = {"off": {}, "follow": dict(follow_camera=True, follow_threshold=FOLLOW_THRESHOLD, follow_anchor=ANCHOR),
          "spill": dict(follow_camera=True, follow_threshold=FOLLOW_THRESHOLD, follow_anchor=(0.4375, 0.5, 0.25),
                        keep_spill=True)}

FACTORS = {
    "backend": ["cuda", "sgm"],
    "frames": ["u8", "f32", "mixed"],
    "lrconf": [False, True],
    "filter": ["none", "fill", "wls1"],
    "temporal": [False, True],
    "rect": [False, True],
    "voxel": [False, True],
    "colour": [False, True],
    "poses": ["given", "tracked"],
    "follow": ["off", "follow", "spill"],
    "render": [False, True],
    "inv": [-1.0, -7.5],
}
CASES = pairwise_cases(FACTORS)


def case_id(c):
    return "-".join([c["backend"], c["frames"], "lrconf" if c["lrconf"] else "nolr", c["filter"],
                     "tf" if c["temporal"] else "notf", "rect" if c["rect"] else "norect",
                     "vox" if c["voxel"] else "novox", "rgb" if c["colour"] else "nocol", c["poses"],
                     c["follow"], "model" if c["render"] else "nomodel", f"inv{c['inv']:g}"])


IDS = [case_id(c) for c in CASES]


# ----------------------------------------------------------------------------- the scene and its views
def scene() -> tsdf_ref.Scene:
    base = fc.scene()
    boxes = [(tuple(lo), tuple(hi)) for lo, hi in base.boxes]
    boxes.append(((-1.5, -1.7, -1.0), (1.8, -1.5, 14.0)))             # a ceiling
    boxes.append(((-1.5, -1.7, 13.0), (1.8, 0.6, 14.0)))              # the corridor's end
    return tsdf_ref.Scene(ground_y=base.ground_y, boxes=boxes)


def q_matrix() -> np.ndarray:
    """cuda_depth.reprojection_matrix(FX, CX, CY, BASE), restated: float64, rounded once."""
    return np.array([[1.0, 0.0, 0.0, -CX], [0.0, 1.0, 0.0, -CY], [0.0, 0.0, 0.0, FX], [0.0, 0.0, 1.0 / BASE, 0.0]],
                    np.float64).astype(F)


def _hash(ix, iy, iz, salt):
    """0..255 from three int64 lattice coordinates (a multiply-xorshift mix in wrapping uint64 arithmetic)."""
    with np.errstate(over="ignore"):
        h = (ix.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) ^ iy.astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F)
             ^ iz.astype(np.uint64) * np.uint64(0x165667B19E3779F9) ^ np.uint64(salt) * np.uint64(0xD6E8FEB86659FD93))
        h ^= h >> np.uint64(32)
        h *= np.uint64(0xD6E8FEB86659FD93)
        h ^= h >> np.uint64(29)
    return (h & np.uint64(0xFF)).astype(np.float64)


def texture(points, seed=0) -> np.ndarray:
    """[N, 3] float64 in 0..255: value noise of the world points [N, 3], constant over cells of 0.72, 0.24 and 0.08 m (the
    lattices are offset so that no face of the scene lies on a cell boundary)."""
    p = np.asarray(points, np.float64) + np.array([0.0137, 0.0291, 0.0173])
    out = np.zeros((p.shape[0], 3))
    for octave, (size, share) in enumerate(OCTAVES):
        cell = np.floor(p / size).astype(np.int64)
        for ch in range(3):
            out[:, ch] += share * _hash(cell[:, 0], cell[:, 1], cell[:, 2], 1 + seed * 16 + octave * 3 + ch)
    return out


def view(pose, u, v) -> np.ndarray:
    """[3, ...] float64 colours, rounded, of the scene through the pixels (u, v) (any shape, fractional allowed) of the
    camera at the camera-to-world pose: the mean of the texture at SUPERSAMPLE x SUPERSAMPLE rays spread evenly over the
    pixel's square, so that the two views of a surface agree where its texture is finer than a pixel as well."""
    m = np.asarray(pose, np.float64)
    total = np.zeros(u.shape + (3,))
    sub = (np.arange(SUPERSAMPLE) + 0.5) / SUPERSAMPLE - 0.5
    for dv in sub:
        for du in sub:
            dc = np.stack([(u + du - CX) / FX, (v + dv - CY) / FX, np.ones_like(u)], axis=-1).reshape(-1, 3)
            dw = dc @ m[:3, :3].T
            lam = scene().ray_depth(m[:3, 3], dw)
            assert np.isfinite(lam).all(), "the scene is closed"
            total += texture(m[:3, 3] + lam[:, None] * dw).reshape(u.shape + (3,))
    return np.moveaxis(np.rint(total / SUPERSAMPLE ** 2), -1, 0)


def right_pose(pose) -> np.ndarray:
    m = np.array(pose, np.float64)
    m[:3, 3] += BASE * m[:3, 0]
    return m


def rotation(angles) -> np.ndarray:
    ax, ay, az = angles
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return rz @ ry @ rx


@functools.lru_cache(maxsize=None)
def path(frames=FRAMES) -> np.ndarray:
    """[frames, 4, 4] float64: the true left poses, STEP and TURN further each frame."""
    poses = []
    for f in range(frames):
        m = np.eye(4)
        m[:3, :3] = rotation(f * TURN)
        m[:3, 3] = [s + f * d for s, d in zip(START, STEP)]
        poses.append(m)
    out = np.stack(poses)
    out.setflags(write=False)
    return out


def affine(seed, shift):
    """(a, s, tx, ty) of a mild raw-from-rectified map: x = s (cos a u - sin a v) + tx, y = s (sin a u + cos a v) + ty."""
    rng = np.random.default_rng(seed)
    a, s = rng.uniform(-0.01, 0.01), rng.uniform(0.97, 1.0)
    return a, s, rng.uniform(1, 3) + shift, rng.uniform(1, 3)


def qmap(params) -> np.ndarray:
    """The int32 map [H, W, 2] of 1/32-pixel raw coordinates (rectify_ref's format) of affine()'s parameters."""
    a, s, tx, ty = params
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return rectify_ref.quantize_map(s * (np.cos(a) * u - np.sin(a) * v) + tx, s * (np.sin(a) * u + np.cos(a) * v) + ty,
                                    (RAW_H, RAW_W))


RECT_LEFT, RECT_RIGHT = affine(1, 10), affine(2, 0)                  # the left map reaches past the raw frame's right edge


def rectification():
    """(left map, right map, raw shape), as PipelineRef and cuda_depth.StereoRectification take them."""
    return qmap(RECT_LEFT), qmap(RECT_RIGHT), (RAW_H, RAW_W)


def _pixels(params):
    """(u, v) of the view that every pixel of a frame shows: the frame's own grid, or with affine() parameters the
    rectified coordinates of the raw frame's pixels."""
    if params is None:
        v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        return u, v
    a, s, tx, ty = params
    y, x = np.meshgrid(np.arange(RAW_H, dtype=np.float64), np.arange(RAW_W, dtype=np.float64), indexing="ij")
    x, y = (x - tx) / s, (y - ty) / s
    return np.cos(a) * x + np.sin(a) * y, -np.sin(a) * x + np.cos(a) * y


@functools.lru_cache(maxsize=None)
def clean_pair(f, rect):
    """The noise-free float64 views [3, h, w] of frame f: (left, right)."""
    pose = path()[f]
    left = view(pose, *_pixels(RECT_LEFT if rect else None))
    right = view(right_pose(pose), *_pixels(RECT_RIGHT if rect else None))
    return left, right


def frames(kind, rect, seed, order):
    """[(left, right)] of the frames `order` (indices into path(); FLAT stands for the flat pair) as [3, h, w] arrays of
    the case's dtype(s): integer-valued float32 or uint8; mixed: the uint8 frame is the left one at even positions and
    the right one at odd positions."""
    rng = np.random.default_rng(seed)
    out = []
    for k, f in enumerate(order):
        if f == FLAT:
            shape = (3, RAW_H, RAW_W) if rect else (3, H, W)
            l = r = np.full(shape, 128.0, F)
        else:
            l, r = (np.clip(a + rng.integers(-2, 3, a.shape), 0, 255).astype(F) for a in clean_pair(f, rect))
        if kind == "u8":
            l, r = l.astype(np.uint8), r.astype(np.uint8)
        elif kind == "mixed":
            l, r = (l.astype(np.uint8), r) if k % 2 == 0 else (l, r.astype(np.uint8))
        out.append((np.ascontiguousarray(l), np.ascontiguousarray(r)))
    return out


# ----------------------------------------------------------------------------- a case's keywords and its reference run
ORDER = (0, 1, 2, 3, FLAT, 4, 5)                                     # the sequence: the flat pair is an extra frame
AFTER_RESET = 0                                                      # then the resets and the first view again, with new noise


def chain_keywords(case):
    kw = dict(FILTERS[case["filter"]])
    if case["lrconf"]:
        kw.update(confidence=True, confidence_radius=2, confidence_lr_scale=LR_SCALE)
    if case["temporal"]:
        kw.update(temporal=True, **TEMPORAL)
    return kw


def pipeline_keywords(case):
    """The 3D keywords of DepthEstimationPipeline and Pipeline3DRef but for the volume (tsdf_volume= / volume=)."""
    kw = dict(reprojection_matrix=q_matrix(), point_cloud_depth_range=DEPTH_RANGE, render_model=case["render"],
              **FOLLOW[case["follow"]])
    if case["lrconf"]:
        kw.update(point_cloud_min_confidence=0.1)
    if case["voxel"]:
        kw.update(VOXEL)
    if case["poses"] == "tracked":
        kw.update(track_camera=True, initial_pose=np.array(path()[0]), tracking_args=dict(TRACKING))
    return kw


def volume_keywords(case):
    return dict(dims=DIMS, voxel_size=VS, origin=ORIGIN, color=case["colour"])


def case_frames(case):
    """The case's frames: ORDER, then the one processed after reset_tracking() and reset_temporal()."""
    index = CASES.index(case)
    return frames(case["frames"], case["rect"], 500 + index, ORDER + (AFTER_RESET,))


def given_pose(case, k):
    """The caller's pose of the case's k-th frame (None when the pipeline tracks): the true one; the flat frame is
    given the pose before it."""
    if case["poses"] == "tracked":
        return None
    order = ORDER + (AFTER_RESET,)
    return np.array(path()[order[k] if order[k] != FLAT else order[k - 1]])


def true_pose(k):
    """The true left pose of the k-th frame of a case (the flat frame: None)."""
    order = ORDER + (AFTER_RESET,)
    return None if order[k] == FLAT else np.array(path()[order[k]])


def build_reference(case, oracle) -> Pipeline3DRef:
    chain = PipelineRef((H, W), DMIN, DMAX, case["inv"], case["backend"], case["lrconf"], LR_MAX_DIFF, oracle=oracle,
                        rectification=rectification() if case["rect"] else None, **chain_keywords(case))
    return Pipeline3DRef(chain, volume=volume_keywords(case), **pipeline_keywords(case))


@functools.lru_cache(maxsize=None)
def expected(index):
    """The reference's results of case `index`, frame by frame (shared by the tests; read only): ORDER's frames, then
    the frame after reset_tracking() and reset_temporal()."""
    import oracle_lib
    case = CASES[index]
    ref = build_reference(case, oracle_lib.get(parallel=True))
    out = []
    for k, (l, r) in enumerate(case_frames(case)):
        if k == len(ORDER):
            ref.reset_tracking()
            ref.reset_temporal()
        out.append(ref.process(l, r, camera_pose=given_pose(case, k)))
    return out
