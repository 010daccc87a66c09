"""The triples that tests/test_track_rule_cpu.py (the library's rule compiled for the host) and tests/test_track_gpu.py
(the kernels) both hold against the NumPy twin (tests/track_ref.py).  The volume is raycast_cases.fused_state(); the model
views are its 33 x 45 renderings (the twin's here; the GPU tests render them with the library and check the bits are
these); the frames are renderings of the same volume by the raycast twin from poses a few centimetres and about a degree
away, at 37 x 70 (wider than one 64-column tile, no multiple of it or of the 4 tile rows) and 33 x 45, with disparity noise,
5 % invalid, 1 % NaN and 1 % outlier pixels.  Every twin result is computed once and shared."""
import functools

import numpy as np

import raycast_cases as cases
import raycast_ref as rc
import track_ref as tr
import tsdf_ref as ref

f32 = np.float32
FRAME_SHAPES = ((37, 70), (33, 45))
MODEL_SHAPE = cases.SHAPE
MODEL_VIEWS = ("outside", "left")
VIEWS = {"outside": cases.VIEWS["outside"], "left": ref.look_at((-0.2, 0.05, -0.4), (0.05, 0.1, 1.6))}
DEPTH_RANGE = (0.1, 3.5)
MAX_DISTANCE = 0.15
MIN_INLIERS = 50
PARAMS = dict(max_distance=MAX_DISTANCE, depth_range=DEPTH_RANGE, min_inliers=MIN_INLIERS, min_pivot=1e-3)


def displaced(pose, k=0):
    """pose moved by a few centimetres and about a degree (k picks one of a few displacements)."""
    ang = np.radians([[0.7, -0.6, 0.5], [-0.5, 0.8, 0.3], [0.4, 0.5, -0.8]][k % 3])
    shift = np.array([[0.03, -0.02, 0.025], [-0.025, 0.02, 0.03], [0.02, 0.03, -0.02]][k % 3])
    K = np.array([[0, -ang[2], ang[1]], [ang[2], 0, -ang[0]], [-ang[1], ang[0], 0]])
    R = np.eye(3) + K + K @ K / 2
    u, _, vt = np.linalg.svd(R)
    out = np.array(pose, np.float64)
    out[:3, :3] = out[:3, :3] @ (u @ vt)
    out[:3, 3] += shift
    return out


def model_pose(view):
    return VIEWS[view]


@functools.lru_cache(maxsize=None)
def model(view, misses=False):
    """track_ref.model_view of the twin's rendering of the volume from `view` (misses: a view that hit nothing)."""
    Qm = cases.q_of("kitti", MODEL_SHAPE)
    out = rc.raycast_ref(cases.fused_state(), cases.DIMS, cases.ORIGIN, cases.VS, Qm, rc.view_pose(model_pose(view)),
                         MODEL_SHAPE, depth_range=cases.DEPTH_RANGE)
    depth, normals = out["depth"][0], out["normals"][0]
    if misses:
        depth, normals = np.full_like(depth, np.nan), np.zeros_like(normals)
    return tr.model_view(depth, normals, Qm, model_pose(view))


@functools.lru_cache(maxsize=None)
def frame(view, shape, k=0, confidence=False):
    """(disp [H, W] f32, Q, true pose, confidence [H, W] or None) of a noisy frame near `view`."""
    H, W = shape
    rng = np.random.default_rng(100 + 7 * k + H)
    Q = cases.q_of("kitti", shape)
    pose = displaced(model_pose(view), k)
    d = rc.raycast_ref(cases.fused_state(), cases.DIMS, cases.ORIGIN, cases.VS, Q, rc.view_pose(pose), shape,
                       depth_range=cases.DEPTH_RANGE)["disparity"][0].copy()
    hit = d != -1.0
    d[hit] += rng.normal(0, 0.02, int(hit.sum())).astype(f32)
    r = rng.random((H, W))
    d[r < 0.05] = -1.0
    d[(r >= 0.05) & (r < 0.06)] = np.nan
    out = (r >= 0.06) & (r < 0.07)
    d[out] = rng.uniform(1.0, 40.0, int(out.sum())).astype(f32)
    conf = None
    if confidence:
        conf = rng.uniform(0.2, 1.0, (H, W)).astype(f32)
        c = rng.random((H, W))
        conf[c < 0.03] = 0.0
        conf[(c >= 0.03) & (c < 0.05)] = np.nan
        conf[(c >= 0.05) & (c < 0.10)] = 0.05                      # below the min_confidence the tests pass
    d.setflags(write=False)
    return d, Q, pose, conf


def start_pose(view):
    """pose_in [3, 4] f32: tracking starts from the model's pose."""
    return rc.view_pose(model_pose(view))[0]


def _freeze(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def _expected(view, shape, k, confidence, misses, schedule, extra):
    d, Q, _, conf = frame(view, shape, k, confidence)
    kw = dict(PARAMS)
    kw.update(dict(extra))
    if confidence:
        kw.setdefault("min_confidence", 0.1)
    return tr.track_ref(d, Q, start_pose(view), model(view, misses), confidence=conf, schedule=schedule, **kw)


def expected(view, shape, k=0, confidence=False, misses=False, schedule=tr.DEFAULT_SCHEDULE, **extra):
    """The twin's result for one triple (shared; read only)."""
    return _expected(view, shape, k, confidence, misses, tuple(tuple(p) for p in schedule), _freeze(extra))


def assert_same(got, want, what):
    """got / want: dicts of pose [3, 4], info [4], rms, sums [30]; floats compare by bit pattern."""
    assert np.array_equal(np.asarray(got["info"], np.int64), np.asarray(want["info"], np.int64)), \
        f"{what}: info {got['info']} != {want['info']}"
    g, e = np.ascontiguousarray(got["pose"], f32).view(np.uint32), np.ascontiguousarray(want["pose"], f32).view(np.uint32)
    assert np.array_equal(g.reshape(-1), e.reshape(-1)), f"{what}: pose\n{got['pose']}\n{want['pose']}"
    assert np.array_equal(np.asarray(got["rms"], f32).reshape(1).view(np.uint32),
                          np.asarray(want["rms"], f32).reshape(1).view(np.uint32)), f"{what}: rms {got['rms']} {want['rms']}"
    if got.get("sums") is not None:
        gs = np.ascontiguousarray(got["sums"], np.float64).view(np.uint64)
        es = np.ascontiguousarray(want["sums"], np.float64).view(np.uint64)
        assert np.array_equal(gs, es), f"{what}: sums differ at {np.flatnonzero(gs != es)}"


# ---- a short sequence for the pipeline: five frames of the volume along a small trajectory, then an empty frame -----------
SEQ_SHAPE = (48, 96)
SEQ_RANGE = (0.0, 4.0)
SEQ_ARGS = dict(max_distance=0.15, min_inliers=50)


def render_range(pose):
    """TSDFVolume.render's default depth_range for a pose: 0 .. the distance from the (float32) eye to the volume's
    farthest corner, in float64."""
    lo = np.asarray(cases.ORIGIN, np.float64)
    hi = lo + np.asarray(cases.DIMS, np.float64) * cases.VS
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    eye = rc.view_pose(pose)[0][:, 3].astype(np.float64)
    return (0.0, float(np.linalg.norm(corners - eye, axis=1).max()))


@functools.lru_cache(maxsize=None)
def sequence():
    """(Q, frames [6, H, W] f32, true poses): frames 0..4 see the fused volume from a trajectory of steps of a few
    centimetres and a degree; frame 5 is all invalid, hence untrackable."""
    Q = cases.q_of("kitti", SEQ_SHAPE)
    poses = [VIEWS["outside"]]
    for k in range(4):
        poses.append(displaced(poses[-1], k))
    rng = np.random.default_rng(5)
    frames = []
    for p in poses:
        d = rc.raycast_ref(cases.fused_state(), cases.DIMS, cases.ORIGIN, cases.VS, Q, rc.view_pose(p), SEQ_SHAPE,
                           depth_range=cases.DEPTH_RANGE)["disparity"][0].copy()
        hit = d != -1.0
        d[hit] += rng.normal(0, 0.02, int(hit.sum())).astype(f32)
        d[rng.random(SEQ_SHAPE) < 0.03] = -1.0
        frames.append(d)
    frames.append(np.full(SEQ_SHAPE, -1.0, f32))
    return Q, np.stack(frames), np.stack(poses)


@functools.lru_cache(maxsize=None)
def sequence_expected(order=(0, 1, 2, 5, 3, 4)):
    """What DepthEstimationPipeline(track_camera=True) must do with the frames in `order`, by the twins: a list of
    (pose [4, 4] float64, lost) per frame and the volume's final state."""
    Q, frames, poses = sequence()
    state = ref.empty_state(cases.DIMS, False)
    P = ref.projection(Q)
    last, out = None, []
    for i in order:
        lost = False
        if last is None:
            last = np.array(poses[0], np.float64)
        else:
            view = rc.raycast_ref(state, cases.DIMS, cases.ORIGIN, cases.VS, Q, rc.view_pose(last), SEQ_SHAPE,
                                  depth_range=render_range(last))
            got = tr.track_ref(frames[i], Q, rc.view_pose(last)[0], tr.model_view(view["depth"][0], view["normals"][0], Q, last),
                               depth_range=SEQ_RANGE, min_pivot=1e-3, **SEQ_ARGS)
            lost = bool(got["info"][0])
            if not lost:
                last = np.vstack([got["pose"].astype(np.float64), [0.0, 0.0, 0.0, 1.0]])
        if not lost:
            ref.integrate_ref(state, cases.DIMS, cases.ORIGIN, cases.VS, 3 * cases.VS, 64.0, frames[i][None], Q, P,
                              ref.world_to_camera(last), depth_range=SEQ_RANGE)
        out.append((last.copy(), lost))
    return out, state
