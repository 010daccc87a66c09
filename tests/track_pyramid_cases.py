"""The cases that tests/test_track_pyramid_rule_cpu.py (the library's rule compiled for the host),
tests/test_track_pyramid_cpu.py (the twin's own properties) and tests/test_track_pyramid_gpu.py (the kernels) hold against
the NumPy twin (tests/track_pyramid_ref.py): the triples of tests/track_photo_cases.py with pyramids of their planes, the
planes of the pyramid tests, a textured wall seen from starts several pixels off -- the case the pyramid is for -- and
hand-made frames of one pixel for the edges of the tap rule at level 1 and for Huber's threshold.  Every twin result is
computed once and shared."""
import functools

import numpy as np

import track_cases as tc
import track_photo_cases as pc
import track_photo_ref as tp
import track_pyramid_ref as ty
import track_ref as tr

f32 = np.float32
LEVELS = 3
SCHEDULE = ((4, 2), (2, 2), (1, 3))                                  # with the levels (2, 1, 0)
SCHEDULE_LEVELS = (2, 1, 0)
HUBER = 6.0                                                          # three sigma of the planes' noise of two units


def frozen(a):
    a.setflags(write=False)
    return a


# ---- planes for the pyramid ---------------------------------------------------------------------------------------------------
# 1 x 1 up to more than two tiles of 64 output columns; (67, 131): level 1 is 34 x 66, three tiles down and two across
PYRAMID_SHAPES = ((1, 1), (1, 7), (2, 3), (5, 1), (33, 45), (37, 70), (67, 131), (3, 1030))


@functools.lru_cache(maxsize=None)
def pyramid_planes(n, shape, masked=False):
    """(planes [n, H, W] with 2 % NaNs and an infinity, mask_depth or None): the mask holds 0, negative values, inf and
    NaN among depths of about 2."""
    H, W = shape
    rng = np.random.default_rng(900 + 13 * n + H + 3 * W)
    a = rng.uniform(0.0, 255.0, (n, H, W)).astype(f32)
    if H * W > 8:
        a[rng.random(a.shape) < 0.02] = np.nan
        a.reshape(-1)[(H * W) // 2] = np.inf
    mask = None
    if masked:
        mask = rng.uniform(1.0, 3.0, (n, H, W)).astype(f32)
        r = rng.random(mask.shape)
        for k, v in enumerate((0.0, -1.5, np.inf, -np.inf, np.nan)):
            mask[(r >= 0.02 * k) & (r < 0.02 * (k + 1))] = v
        if H * W > 8:
            mask.reshape(-1)[:5] = (0.0, -1.5, np.inf, -np.inf, np.nan)
    return frozen(a), None if mask is None else frozen(mask)


@functools.lru_cache(maxsize=None)
def pyramid_expected(n, shape, levels, masked=False):
    planes, mask = pyramid_planes(n, shape, masked)
    return ty.intensity_pyramid_ref(planes, levels, mask)


def same_planes(got, want):
    """Finite values by bit pattern, everything else by kind and place."""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    if got.shape != want.shape:
        return False
    fin = np.isfinite(want)
    return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isfinite(got), fin) and
            np.array_equal(got[fin].view(np.uint32), want[fin].view(np.uint32)) and
            np.array_equal(np.signbit(got[~fin & ~np.isnan(want)]), np.signbit(want[~fin & ~np.isnan(want)])))


# ---- the triples of track_photo_cases with pyramids ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def frame_pyramid(shape, k=0, levels=LEVELS):
    return ty.intensity_pyramid_ref(pc.frame_intensity(shape, k), levels)


@functools.lru_cache(maxsize=None)
def _model(view, misses, levels, clean):
    m = dict(pc.model(view, misses))
    if clean:
        m["intensity"] = pc.smooth(tc.MODEL_SHAPE, np.random.default_rng(700 + len(view)), nan_fraction=0.0)
    m["pyramid"] = ty.intensity_pyramid_ref(m["intensity"], levels, m["depth"])
    return m


def model(view, misses=False, levels=LEVELS, clean=False):
    """track_photo_cases.model with the pyramid of its intensity plane, masked by its depth.  That plane's sprinkled NaNs
    leave few finite pixels two levels up (a level-2 pixel stands on 13 x 13 pixels); clean: the plane without them, so
    that the coarse levels' terms are many."""
    return _model(view, misses, levels, clean)


@functools.lru_cache(maxsize=None)
def _expected(view, shape, k, confidence, misses, schedule, schedule_levels, levels, huber_delta, weight, clean, extra):
    d, Q, _, conf = tc.frame(view, shape, k, confidence)
    kw = dict(tc.PARAMS)
    kw.update(dict(extra))
    if confidence:
        kw.setdefault("min_confidence", 0.1)
    kw.setdefault("max_difference", pc.MAX_DIFFERENCE)
    return ty.track_pyramid_ref(d, Q, tc.start_pose(view), model(view, misses, levels, clean), frame_pyramid(shape, k, levels),
                                weight,
                                schedule_levels=schedule_levels, huber_delta=huber_delta, confidence=conf, schedule=schedule,
                                **kw)


def expected(view, shape, k=0, confidence=False, misses=False, schedule=SCHEDULE, schedule_levels=SCHEDULE_LEVELS,
             levels=LEVELS, huber_delta=np.inf, weight=pc.WEIGHT, clean=False, **extra):
    """The twin's result for one triple (shared; read only)."""
    return _expected(view, shape, k, confidence, misses, tuple(tuple(p) for p in schedule), tuple(schedule_levels), levels,
                     float(huber_delta), weight, clean, tc._freeze(extra))


assert_same = pc.assert_same

# ---- the wall -----------------------------------------------------------------------------------------------------------------
# A textured wall 2 m ahead of a camera of 120 px focal length, 96 x 128 pixels; the frame's camera stands WALL_START_PX
# pixels of the wall's image to the side of the model view's and is turned 1.15 degrees about the optical axis.  Geometry
# leaves exactly those three directions free, and the start is outside the basin of one-pixel texture.
WALL_SHAPE = (96, 128)
WALL_Z, WALL_F, WALL_BASELINE = 2.0, 120.0, 0.2
WALL_START_PX = 8.0
WALL_LEVELS = 3
WALL_SCHEDULE, WALL_SCHEDULE_LEVELS = tr.DEFAULT_SCHEDULE, (2, 1, 0)
WALL_PARAMS = dict(max_distance=0.3, depth_range=(0.1, 4.0), min_inliers=50, min_pivot=1e-3)
WALL_WEIGHT, WALL_MAX_DIFFERENCE, WALL_HUBER = 0.01, 255.0, 20.0
WALL_WAVELENGTHS_PX = (5.0, 7.0, 10.0, 14.0, 20.0, 28.0, 40.0, 56.0)
WALL_AMPLITUDES = (8.0, 9.0, 10.0, 11.0, 12.0, 14.0, 16.0, 18.0)


def wall_q():
    H, W = WALL_SHAPE
    from raycast_cases import reprojection
    return reprojection(WALL_F, (W - 1) / 2.0 + 0.25, (H - 1) / 2.0 - 0.5, WALL_BASELINE)


@functools.lru_cache(maxsize=None)
def _wall_waves():
    rng = np.random.default_rng(4242)
    ang, phase = rng.uniform(0.0, np.pi, 8), rng.uniform(0.0, 2 * np.pi, 8)
    k = 2 * np.pi * WALL_F / (WALL_Z * np.array(WALL_WAVELENGTHS_PX))     # radians per metre on the wall
    return k * np.cos(ang), k * np.sin(ang), phase


def wall_texture(X, Y):
    kx, ky, phase = _wall_waves()
    out = np.full(np.shape(X), 128.0)
    for a, cx, cy, ph in zip(WALL_AMPLITUDES, kx, ky, phase):
        out = out + a * np.sin(cx * X + cy * Y + ph)
    return out


def wall_model_pose():
    return pc.plane_model_pose()


def wall_true_pose(start_px=WALL_START_PX):
    """The model pose moved sideways by start_px pixels of the wall's image and turned 1.15 degrees about the axis."""
    a, s = 0.01, start_px * WALL_Z / WALL_F
    R = np.array([[1 - a * a, -2 * a, 0.0], [2 * a, 1 - a * a, 0.0], [0.0, 0.0, 1 + a * a]]) / (1 + a * a)
    d = np.eye(4)
    d[:3, :3], d[:3, 3] = R, [0.8 * s, -0.6 * s, 0.01]
    return wall_model_pose() @ d


def _rays(Q, shape):
    H, W = shape
    q = Q.astype(np.float64)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([(q[0, 0] * u + q[0, 3]) / q[2, 3], (q[1, 1] * v + q[1, 3]) / q[2, 3], np.ones_like(u)], -1)


@functools.lru_cache(maxsize=None)
def wall_model():
    """The analytic model view with its intensity plane and that plane's pyramid."""
    Hm, Wm = WALL_SHAPE
    Q = wall_q()
    ray = _rays(Q, WALL_SHAPE)
    normals = np.zeros((3, Hm, Wm), f32)
    normals[2] = -1.0
    m = tr.model_view(np.full((Hm, Wm), WALL_Z, f32), normals, Q, wall_model_pose())
    m["intensity"] = frozen(wall_texture(ray[..., 0] * WALL_Z, ray[..., 1] * WALL_Z).astype(f32))
    m["pyramid"] = ty.intensity_pyramid_ref(m["intensity"], WALL_LEVELS, m["depth"])
    return m


@functools.lru_cache(maxsize=None)
def wall_frame(start_px=WALL_START_PX):
    """(disp with noise of 0.25 px, Q, intensity, the intensity's pyramid) of the frame that sees the wall from
    wall_true_pose(start_px)."""
    Q = wall_q()
    q = Q.astype(np.float64)
    rel = np.linalg.inv(wall_model_pose()) @ wall_true_pose(start_px)     # frame camera -> model camera
    rm = _rays(Q, WALL_SHAPE) @ rel[:3, :3].T
    lam = (WALL_Z - rel[2, 3]) / rm[..., 2]                          # the frame camera's depth of the hit
    hit = rel[:3, 3] + rm * lam[..., None]
    rng = np.random.default_rng(77)
    disp = ((q[2, 3] / lam - q[3, 3]) / q[3, 2] + rng.normal(0.0, 0.25, WALL_SHAPE)).astype(f32)
    inten = wall_texture(hit[..., 0], hit[..., 1]).astype(f32)
    return frozen(disp), Q, frozen(inten), ty.intensity_pyramid_ref(inten, WALL_LEVELS)


def wall_start():
    import raycast_ref as rc
    return rc.view_pose(wall_model_pose())[0]


@functools.lru_cache(maxsize=None)
def wall_expected(start_px=WALL_START_PX):
    """(the geometric twin's result, the photometric twin's, the pyramid twin's) on the default schedule."""
    d, Q, inten, pyr = wall_frame(start_px)
    m = wall_model()
    geo = tr.track_ref(d, Q, wall_start(), m, schedule=WALL_SCHEDULE, **WALL_PARAMS)
    photo = tp.track_photo_ref(d, Q, wall_start(), m, inten, WALL_WEIGHT, max_difference=WALL_MAX_DIFFERENCE,
                               schedule=WALL_SCHEDULE, **WALL_PARAMS)
    pyramid = ty.track_pyramid_ref(d, Q, wall_start(), m, pyr, WALL_WEIGHT, schedule_levels=WALL_SCHEDULE_LEVELS,
                                   huber_delta=WALL_HUBER, max_difference=WALL_MAX_DIFFERENCE, schedule=WALL_SCHEDULE,
                                   **WALL_PARAMS)
    return geo, photo, pyramid


def wall_errors(start_px=WALL_START_PX):
    """((metres, degrees) of the start, of the photometric twin's end, of the pyramid twin's end)."""
    _, photo, pyramid = wall_expected(start_px)
    true = wall_true_pose(start_px)
    return tr.pose_error(wall_start(), true), tr.pose_error(photo["pose"], true), tr.pose_error(pyramid["pose"], true)


# ---- the edges of the tap rule at level 1: one frame pixel against an 8 x 10 model view, by hand -------------------------------
EDGE_MODEL_SHAPE = (8, 10)                                           # level 1: 4 x 5
EDGE_LEVELS = 2
EDGE_PARAMS = dict(max_distance=2.0, depth_range=(0.1, 4.0), min_inliers=1, min_pivot=0.0)
EDGE_NAMES = ("inside", "x0_at_wl_minus_2", "x0_at_wl_minus_1", "tap_with_nan")
EDGE_COUNTS = {"inside": 1, "x0_at_wl_minus_2": 1, "x0_at_wl_minus_1": 0, "tap_with_nan": 0}


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """(disp [1, 1], Q, start pose [3, 4], model dict with its pyramid, frame pyramid, weight, max_difference): as
    track_photo_cases.edge_case, the frame's one pixel projects to the model pixel (x, y) exactly, which is
    (x / 2, y / 2) at level 1, read by a pair of stride 2."""
    Hm, Wm = EDGE_MODEL_SHAPE
    x, y = {"x0_at_wl_minus_2": (6.0, 3.0), "x0_at_wl_minus_1": (8.0, 3.0)}.get(name, (3.0, 3.0))
    Qm = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], f32)
    Q = np.array([[1, 0, 0, x], [0, 1, 0, y], [0, 0, 0, 1], [0, 0, 1, 0]], f32)
    depth = np.full((Hm, Wm), 2.0, f32)
    normals = np.zeros((3, Hm, Wm), f32)
    normals[2] = -1.0
    v, u = np.meshgrid(np.arange(Hm, dtype=f32), np.arange(Wm, dtype=f32), indexing="ij")
    inten = (16.0 * u + 4.0 * v * v).astype(f32)
    if name == "tap_with_nan":
        inten[3, 5] = np.nan                                         # under level-1 pixels (2, 1) and (2, 2), not (1, 1)
    m = tr.model_view(depth, normals, Qm, np.eye(4))
    m["intensity"] = inten
    m["pyramid"] = ty.intensity_pyramid_ref(inten, EDGE_LEVELS, depth)
    if name == "tap_with_nan":
        lvl = m["pyramid"][1]
        assert np.isfinite(lvl[1, 1]) and np.isnan(lvl[1, 2]) and np.isnan(lvl[2, 2])
    frame = ty.intensity_pyramid_ref(np.full((1, 1), 40.0, f32), EDGE_LEVELS)
    return np.full((1, 1), 0.5, f32), Q, np.eye(4, dtype=f32)[:3], m, frame, 0.25, 1000.0


@functools.lru_cache(maxsize=None)
def edge_expected(name):
    disp, Q, start, m, frame, weight, max_difference = edge_case(name)
    return ty.track_pyramid_ref(disp, Q, start, m, frame, weight, schedule_levels=(1,), max_difference=max_difference,
                                schedule=((2, 1),), **EDGE_PARAMS)


# ---- Huber's threshold: track_photo_cases' one-pixel frame, whose residual is 3 exactly ------------------------------------------

@functools.lru_cache(maxsize=None)
def huber_case():
    """track_photo_cases.edge_case("inside") with pyramids of one level: e = 3.0f exactly."""
    disp, Q, start, m, inten, weight, max_difference, _ = pc.edge_case("inside")
    m = dict(m)
    m["pyramid"] = ty.intensity_pyramid_ref(m["intensity"], 1, m["depth"])
    return disp, Q, start, m, ty.intensity_pyramid_ref(inten, 1), weight, max_difference


@functools.lru_cache(maxsize=None)
def huber_expected(delta):
    disp, Q, start, m, frame, weight, max_difference = huber_case()
    return ty.track_pyramid_ref(disp, Q, start, m, frame, weight, huber_delta=delta, max_difference=max_difference,
                                schedule=((1, 1),), **pc.EDGE_PARAMS)
