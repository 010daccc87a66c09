"""The cases that tests/test_track_photo_rule_cpu.py (the library's rule compiled for the host), tests/test_track_photo_cpu.py
(the twin's own properties) and tests/test_track_photo_gpu.py (the kernels) hold against the NumPy twin
(tests/track_photo_ref.py).  The triples are tests/track_cases.py's with intensity planes added: a smooth function of the
pixel plus noise, NaNs sprinkled into both planes; the model views are the volume's renderings, with misses next to hits.
Then one textured fronto-parallel plane with analytic model planes (the geometric tracker loses it), and hand-made frames
of a few pixels for the edges of the tap rule.  Every twin result is computed once and shared."""
import functools

import numpy as np

import raycast_cases as cases
import raycast_ref as rc
import track_cases as tc
import track_photo_ref as tp
import track_ref as tr

f32 = np.float32
WEIGHT = 0.01                                                        # metres per intensity unit
MAX_DIFFERENCE = 30.0


def smooth(shape, rng, nan_fraction=0.01):
    """An intensity plane: a smooth function of the pixel about the image centre (so that a frame and a model view of
    the same focal length roughly agree), noise of two units, and NaNs."""
    H, W = shape
    v, u = np.meshgrid(np.arange(H) - (H - 1) / 2.0, np.arange(W) - (W - 1) / 2.0, indexing="ij")
    a = 128.0 + 40.0 * np.sin(0.21 * u + 0.3) + 30.0 * np.cos(0.17 * v) + 10.0 * np.sin(0.05 * u * v)
    a = (a + rng.normal(0.0, 2.0, shape)).astype(f32)
    a[rng.random(shape) < nan_fraction] = np.nan
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def frame_intensity(shape, k=0):
    return smooth(shape, np.random.default_rng(500 + 7 * k + shape[0]))


@functools.lru_cache(maxsize=None)
def model(view, misses=False, shape=tc.MODEL_SHAPE):
    """track_cases.model (scaled_model at another shape) with an intensity plane."""
    m = dict(tc.model(view, misses) if shape == tc.MODEL_SHAPE else tc.scaled_model(view, shape, misses))
    m["intensity"] = smooth(shape, np.random.default_rng(700 + len(view)))
    return m


@functools.lru_cache(maxsize=None)
def _expected(view, shape, k, confidence, misses, schedule, weight, extra):
    d, Q, _, conf = tc.frame(view, shape, k, confidence)
    kw = dict(tc.PARAMS)
    kw.update(dict(extra))
    if confidence:
        kw.setdefault("min_confidence", 0.1)
    kw.setdefault("max_difference", MAX_DIFFERENCE)
    return tp.track_photo_ref(d, Q, tc.start_pose(view), model(view, misses), frame_intensity(shape, k), weight,
                              confidence=conf, schedule=schedule, **kw)


def expected(view, shape, k=0, confidence=False, misses=False, schedule=tr.DEFAULT_SCHEDULE, weight=WEIGHT, **extra):
    """The twin's result for one triple (shared; read only)."""
    return _expected(view, shape, k, confidence, misses, tuple(tuple(p) for p in schedule), weight, tc._freeze(extra))


def assert_same(got, want, what):
    """track_cases.assert_same, and the photometric count, its complement and the rms by bit pattern."""
    tc.assert_same(got, want, what)
    assert np.array_equal(np.asarray(got["pinfo"], np.int64), np.asarray(want["pinfo"], np.int64)), \
        f"{what}: photometric info {got['pinfo']} != {want['pinfo']}"
    assert np.array_equal(np.asarray(got["prms"], f32).reshape(1).view(np.uint32),
                          np.asarray(want["prms"], f32).reshape(1).view(np.uint32)), \
        f"{what}: photometric rms {got['prms']} {want['prms']}"


@functools.lru_cache(maxsize=None)
def frame_image(shape, k=0):
    """uint8 RGB [3, H, W]: the smooth plane rounded, with the channels a few units apart."""
    g = np.nan_to_num(smooth(shape, np.random.default_rng(600 + 7 * k + shape[0])), nan=128.0)
    img = np.stack([np.clip(np.rint(g) + o, 0, 255) for o in (4, 0, -6)]).astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def rendered_model(view):
    """The model view with the volume's colours: the twin's rendering, its colours [3, Hm, Wm] uint8 and their intensity."""
    Qm = cases.q_of("kitti", tc.MODEL_SHAPE)
    out = rc.raycast_ref(cases.fused_state(), cases.DIMS, cases.ORIGIN, cases.VS, Qm, rc.view_pose(tc.model_pose(view)),
                         tc.MODEL_SHAPE, depth_range=cases.DEPTH_RANGE)
    m = tr.model_view(out["depth"][0], out["normals"][0], Qm, tc.model_pose(view))
    m["colors"] = out["colors"][0]
    m["intensity"] = tp.intensity_planes_ref(out["colors"], 3)[0]
    return m


@functools.lru_cache(maxsize=None)
def rendered_expected(view, shape, k=0):
    """The twin's result for frame_image(shape, k) against rendered_model(view); the volume's colours are noise, so the
    threshold lets every difference through."""
    d, Q, _, _ = tc.frame(view, shape, k)
    return tp.track_photo_ref(d, Q, tc.start_pose(view), rendered_model(view),
                              tp.intensity_planes_ref(frame_image(shape, k)[None], 3)[0], WEIGHT, max_difference=255.0,
                              **tc.PARAMS)


# ---- the deep tree: one iteration at stride 1 on track_cases.scaled_frame ---------------------------------------------------
# The combine adds a triple's group partials in 16 chunks of len = padded groups / 16 (k_track_body.h with k_track_photo.h's
# constants).  (shape, len): 94, 257, 20 and 33 group partials, so one leaf of eight, four leaves of eight under the
# stack, a pair and a tree of four per chunk
TREE_CASES = (((300, 257), 8), ((1027, 193), 32), ((80, 193), 2), ((176, 130), 4))
TREE_SHAPES = tuple(s for s, _ in TREE_CASES)
TREE_LENS = {2, 4, 8, 32}
CHUNKS, STACK = 16, 7                                                # k_track_photo.h


def tree_len(shape):
    groups, padded = tc.track_grid(shape, 1)["groups"], 1
    while padded < groups:
        padded *= 2
    return padded // CHUNKS if padded > CHUNKS else 1


@functools.lru_cache(maxsize=None)
def tree_intensity(shape):
    """The model view's smooth plane seen at the frame's shape (scaled_q: the frame sees the model view's field)."""
    return smooth(shape, np.random.default_rng(800 + shape[0]))


@functools.lru_cache(maxsize=None)
def tree_model():
    m = dict(tc.model(tc.TREE_VIEW))
    H, W = tc.MODEL_SHAPE
    m["intensity"] = smooth((H, W), np.random.default_rng(801))
    return m


@functools.lru_cache(maxsize=None)
def tree_expected(shape):
    d, Q = tc.scaled_frame(shape)
    return tp.track_photo_ref(d, Q, tc.start_pose(tc.TREE_VIEW), tree_model(), tree_intensity(shape), WEIGHT,
                              confidence=tc.wide_confidence(shape), schedule=((1, 1),), max_difference=200.0, keep_tiles=True,
                              **tc.PARAMS)


# ---- the plane ----------------------------------------------------------------------------------------------------------------
PLANE_Z = 2.0
PLANE_SHAPES = tc.FRAME_SHAPES
PLANE_PARAMS = dict(max_distance=0.3, depth_range=(0.1, 4.0), min_inliers=50, min_pivot=1e-3)


def texture(X, Y):
    return 128.0 + 50.0 * np.sin(3.1 * X + 0.4 * Y) + 40.0 * np.sin(-0.7 * X + 2.6 * Y) + 20.0 * np.sin(1.9 * X * Y + 1.0)


def plane_model_pose():
    """The model camera looks along +z of the world: the plane's normal is (0, 0, -1) exactly, so the third entry of
    every geometric row is 0 and the third pivot of the geometric system is 0 in any arithmetic."""
    m = np.eye(4)
    m[:3, 3] = [0.1, -0.05, -0.5]
    return m


def plane_true_pose():
    """The model pose moved by 3.7 cm and 1.15 degrees about the optical axis, in the model camera's frame."""
    a = 0.01
    R = np.array([[1 - a * a, -2 * a, 0.0], [2 * a, 1 - a * a, 0.0], [0.0, 0.0, 1 + a * a]]) / (1 + a * a)
    d = np.eye(4)
    d[:3, :3], d[:3, 3] = R, [0.03, -0.02, 0.01]
    return plane_model_pose() @ d


@functools.lru_cache(maxsize=None)
def plane_model():
    """The analytic model view: depth PLANE_Z at every pixel, the normal toward the camera, the texture at the pixel's
    point of the plane."""
    Hm, Wm = tc.MODEL_SHAPE
    Qm = cases.q_of("kitti", tc.MODEL_SHAPE)
    q = Qm.astype(np.float64)
    v, u = np.meshgrid(np.arange(Hm, dtype=np.float64), np.arange(Wm, dtype=np.float64), indexing="ij")
    X = (q[0, 0] * u + q[0, 3]) / q[2, 3] * PLANE_Z
    Y = (q[1, 1] * v + q[1, 3]) / q[2, 3] * PLANE_Z
    normals = np.zeros((3, Hm, Wm), f32)
    normals[2] = -1.0
    m = tr.model_view(np.full((Hm, Wm), PLANE_Z, f32), normals, Qm, plane_model_pose())
    m["intensity"] = texture(X, Y).astype(f32)
    return m


@functools.lru_cache(maxsize=None)
def plane_frame(shape):
    """(disp, Q, intensity) of the frame that sees the plane from plane_true_pose()."""
    H, W = shape
    Q = cases.q_of("kitti", shape)
    q = Q.astype(np.float64)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(q[0, 0] * u + q[0, 3]) / q[2, 3], (q[1, 1] * v + q[1, 3]) / q[2, 3], np.ones_like(u)], -1)
    rel = np.linalg.inv(plane_model_pose()) @ plane_true_pose()     # frame camera -> model camera
    rm = ray @ rel[:3, :3].T
    lam = (PLANE_Z - rel[2, 3]) / rm[..., 2]                        # the frame camera's depth of the hit
    hit = rel[:3, 3] + rm * lam[..., None]
    disp = ((q[2, 3] / lam - q[3, 3]) / q[3, 2]).astype(f32)
    inten = texture(hit[..., 0], hit[..., 1]).astype(f32)
    disp.setflags(write=False)
    inten.setflags(write=False)
    return disp, Q, inten


def plane_start():
    return rc.view_pose(plane_model_pose())[0]


@functools.lru_cache(maxsize=None)
def plane_expected(shape, weight=WEIGHT):
    """(the geometric twin's result, the photometric twin's)."""
    d, Q, inten = plane_frame(shape)
    m = plane_model()
    geo = tr.track_ref(d, Q, plane_start(), m, **PLANE_PARAMS)
    photo = tp.track_photo_ref(d, Q, plane_start(), m, inten, weight, max_difference=40.0, **PLANE_PARAMS)
    return geo, photo


# ---- the edges of the tap rule: one frame pixel against a 4 x 5 model view, by hand ----------------------------------------------
EDGE_MODEL_SHAPE = (4, 5)
EDGE_PARAMS = dict(max_distance=2.0, depth_range=(0.1, 4.0), min_inliers=1, min_pivot=0.0)
EDGE_NAMES = ("inside", "x0_at_wm_minus_2", "x0_at_wm_minus_1", "tap_without_depth", "tap_with_nan_intensity",
              "difference_at_threshold", "difference_above_threshold", "row_not_finite")


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """(disp [1, 1], Q, start pose [3, 4], model dict, frame intensity [1, 1], weight, max_difference, photometric
    inliers expected): the frame's one pixel is the ray u' = X/Z, v' = Y/Z of Q; both cameras sit at the origin, so it
    projects to the model pixel (x, y) = (u', v') exactly for small integers and halves."""
    Hm, Wm = EDGE_MODEL_SHAPE
    x, y = {"x0_at_wm_minus_2": (3.0, 1.5), "x0_at_wm_minus_1": (4.0, 1.5)}.get(name, (1.5, 1.5))
    # model: focal length 1, principal point 0, so that pixel (x, y) is the ray (x, y, 1); baseline 1
    Qm = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], f32)
    # frame: its pixel (0, 0) is the ray (x, y, 1), depth 2 at disparity 0.5
    Q = np.array([[1, 0, 0, x], [0, 1, 0, y], [0, 0, 0, 1], [0, 0, 1, 0]], f32)
    depth = np.full((Hm, Wm), 2.0, f32)
    normals = np.zeros((3, Hm, Wm), f32)
    normals[2] = -1.0
    v, u = np.meshgrid(np.arange(Hm, dtype=f32), np.arange(Wm, dtype=f32), indexing="ij")
    inten = (16.0 * u + 4.0 * v * v).astype(f32)                     # exact in float32, with a gradient in x and y
    weight, max_difference, frame_value, count = 0.25, 8.0, 0.0, 1
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    if name == "x0_at_wm_minus_1":
        count = 0
    if name == "tap_without_depth":
        depth[y0 + 1, x0] = np.nan                                   # not the pixel the geometric rule reads
        count = 0
    if name == "tap_with_nan_intensity":
        inten[y0, x0 + 1] = np.nan
        count = 0
    if count or name in ("tap_without_depth", "tap_with_nan_intensity"):
        ax, ay = f32(x - x0), f32(y - y0)
        bx, by = f32(1) - ax, f32(1) - ay
        clean = (16.0 * u + 4.0 * v * v).astype(f32)
        Im = by * (bx * clean[y0, x0] + ax * clean[y0, x0 + 1]) + ay * (bx * clean[y0 + 1, x0] + ax * clean[y0 + 1, x0 + 1])
        frame_value = float(Im) + 3.0
        if name == "difference_at_threshold":
            frame_value = float(Im) + 8.0                            # |e| == max_difference exactly: accepted
        if name == "difference_above_threshold":
            frame_value, count = float(Im) + 8.5, 0
    if name == "row_not_finite":
        weight, count = 3e38, 0                                      # lambda * e overflows: the seven values are not all finite
    m = tr.model_view(depth, normals, Qm, np.eye(4))
    m["intensity"] = inten
    start = np.eye(4, dtype=f32)[:3]
    return (np.full((1, 1), 0.5, f32), Q, start, m, np.full((1, 1), frame_value, f32), weight, max_difference, count)


@functools.lru_cache(maxsize=None)
def edge_expected(name):
    disp, Q, start, m, inten, weight, max_difference, _ = edge_case(name)
    return tp.track_photo_ref(disp, Q, start, m, inten, weight, max_difference=max_difference, schedule=((1, 1),),
                              **EDGE_PARAMS)
