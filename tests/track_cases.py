"""The triples that tests/test_track_rule_cpu.py (the library's rule compiled for the host) and tests/test_track_gpu.py
(the kernels) both hold against the NumPy twin (tests/track_ref.py).  The volume is raycast_cases.fused_state(); the model
views are its 33 x 45 renderings (the twin's here; the GPU tests render them with the library and check the bits are
these); the frames are renderings of the same volume by the raycast twin from poses a few centimetres and about a degree
away, at 37 x 70 (wider than one 64-column tile, no multiple of it or of the 4 tile rows) and 33 x 45, with disparity noise,
5 % invalid, 1 % NaN and 1 % outlier pixels.  A second set of frames, up to 32765 x 193, sees the whole model view at any
shape and reaches the deep forms of the solve kernel's sum tree (tests/test_track_tree_gpu.py; tests/test_track_cpu.py
holds the conditions that make them worth running).  Every twin result is computed once and shared."""
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


def spoil(d, rng):
    """In place: disparity noise on the hits, then 5 % invalid, 1 % NaN and 1 % outlier pixels."""
    hit = d != -1.0
    d[hit] += rng.normal(0, 0.02, int(hit.sum())).astype(f32)
    r = rng.random(d.shape)
    d[r < 0.05] = -1.0
    d[(r >= 0.05) & (r < 0.06)] = np.nan
    out = (r >= 0.06) & (r < 0.07)
    d[out] = rng.uniform(1.0, 40.0, int(out.sum())).astype(f32)


@functools.lru_cache(maxsize=None)
def frame(view, shape, k=0, confidence=False):
    """(disp [H, W] f32, Q, true pose, confidence [H, W] or None) of a noisy frame near `view`."""
    H, W = shape
    rng = np.random.default_rng(100 + 7 * k + H)
    Q = cases.q_of("kitti", shape)
    pose = displaced(model_pose(view), k)
    d = rc.raycast_ref(cases.fused_state(), cases.DIMS, cases.ORIGIN, cases.VS, Q, rc.view_pose(pose), shape,
                       depth_range=cases.DEPTH_RANGE)["disparity"][0].copy()
    spoil(d, rng)
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


# ---- frames whose sums need the deep forms of k_track_solve's tree (tests/test_track_tree_gpu.py) --------------------------
# k_track_solve sums a triple's group partials in 32 chunks of len = padded groups / 32; every frame above has at most 6
# groups (len 1).  These frames keep the model view's field of view whatever their shape -- q_of keeps the focal length,
# so a large frame would see the volume in a tenth of its pixels and most tiles would add +0.0 -- by a Q whose scale and
# centre follow the frame (anisotropic: only the model's Q has a required form).
TREE_VIEW = "outside"
LIMIT_SHAPE = (32765, 193)                                           # 8192 x 4 = TRK_MAX_TILES tiles, exactly: accepted
LIMIT_SOURCE = (4100, 193)                                           # the limit frame repeats this frame's rows
LIMIT_BAND = 256                                                     # tile rows the twin evaluates at a time there
TREE_LENS = {2, 4, 8, 16, 32, 64, 256}
# (shape, stride, len) of the one-iteration cases; a case's sums are compared, so its tree is the one under test
TREE_CASES = (((176, 130), 1, 2), ((300, 257), 1, 4), ((1027, 193), 1, 16), ((1027, 193), 2, 4), ((1027, 193), 3, 2),
              ((2100, 193), 1, 32), ((4100, 193), 1, 64), ((4100, 193), 2, 16), ((4100, 193), 3, 8), (LIMIT_SHAPE, 1, 256))
TREE_SHAPES = tuple(dict.fromkeys(s for s, _, _ in TREE_CASES if s != LIMIT_SHAPE))
TREE_TWO = ((1, 2),)                                                 # a second iteration on the first one's pose
TREE_MARGIN = 2                                                      # scaled_q's, for schedules of several iterations
TREE_MIXED = ((4100, 193), ((3, 1), (2, 1), (1, 1)))                 # groups change between launches, partial_stride stays
# every (shape, schedule) the GPU tests run; the last pair's stride is the one whose sums are compared
TREE_RUNS = (tuple((s, ((stride, 1),)) for s, stride, _ in TREE_CASES) + tuple((s, TREE_TWO) for s in TREE_SHAPES) +
             (TREE_MIXED,))
TILE_COLS, TILE_ROWS, GROUP_TILES, CHUNKS = 64, 4, 4, 32             # smx_workspace.h, k_track.h


def run_id(run):
    (H, W), schedule = run
    return f"{H}x{W}-" + "+".join(f"{k}@{s}" for s, k in schedule)


def track_grid(shape, stride):
    """smx_workspace.h's track_grid, restated: dict of ws, hs, tx, ty, tiles, groups."""
    H, W = shape
    ws, hs = -(-W // stride), -(-H // stride)
    tx, ty = -(-ws // TILE_COLS), -(-hs // TILE_ROWS)
    return dict(ws=ws, hs=hs, tx=tx, ty=ty, tiles=tx * ty, groups=-(-tx * ty // GROUP_TILES))


def tree_len(shape, stride):
    """The partials per chunk of k_track_solve for a frame at a stride."""
    groups, padded = track_grid(shape, stride)["groups"], 1
    while padded < groups:
        padded *= 2
    return padded // CHUNKS if padded > CHUNKS else 1


def scaled_q(shape, margin=0):
    """The 33 x 45 model view's Q for a frame of another shape that sees the same field of view: pixel (u, v) stands for
    the model pixel ((u + 0.5) / sx - 0.5, (v + 0.5) / sy - 0.5) with s = shape / (33, 45).  margin: the frame sees the
    model view without its outer `margin` pixels, s = shape / (33 - 2 margin, 45 - 2 margin): a frame that is tracked
    for more than one iteration then still lands on the model view, border tiles included, after a step of a degree."""
    q = cases.q_of("kitti", MODEL_SHAPE).astype(np.float64)
    sy, sx = shape[0] / (MODEL_SHAPE[0] - 2 * margin), shape[1] / (MODEL_SHAPE[1] - 2 * margin)
    q[0, 3] += q[0, 0] * (0.5 / sx - 0.5 + margin)
    q[1, 3] += q[1, 1] * (0.5 / sy - 0.5 + margin)
    q[0, 0] /= sx
    q[1, 1] /= sy
    return q.astype(f32)


def run_margin(schedule):
    """The margin of the frame a schedule is run on: none for one iteration (the first starts on the model's own pose),
    TREE_MARGIN model pixels for more."""
    return TREE_MARGIN if sum(k for _, k in schedule) > 1 else 0


@functools.lru_cache(maxsize=None)
def _scaled_render(view, shape, k, margin):
    return rc.raycast_ref(cases.fused_state(), cases.DIMS, cases.ORIGIN, cases.VS, scaled_q(shape, margin),
                          rc.view_pose(displaced(model_pose(view), k)), shape, depth_range=cases.DEPTH_RANGE)["disparity"][0]


@functools.lru_cache(maxsize=None)
def scaled_frame(shape, k=0, view=TREE_VIEW, margin=0):
    """(disp [H, W] f32, Q) of a noisy frame near `view` under scaled_q(shape, margin).  The limit frame repeats the rows
    of the LIMIT_SOURCE frame's rendering (the twin's rendering of 6.3 M pixels would take most of a minute; a frame is
    input, not expectation) and takes its noise and spoilt pixels at its own size."""
    H, W = shape
    if shape == LIMIT_SHAPE:
        src = _scaled_render(view, LIMIT_SOURCE, k, margin)
        d = src[((2 * np.arange(H) + 1) * LIMIT_SOURCE[0]) // (2 * H)].copy()
    else:
        d = _scaled_render(view, shape, k, margin).copy()
    spoil(d, np.random.default_rng(300 + 7 * k + H))
    d.setflags(write=False)
    return d, scaled_q(shape, margin)


@functools.lru_cache(maxsize=None)
def wide_confidence(shape, k=0):
    """confidence [H, W] f32 for scaled_frame(shape, k): weights spread log-uniformly over 2^-20 .. 1, with 3 % zeros and
    2 % NaNs.  The terms are float32 products, and float64 sums of a few thousand float32 values of like magnitude are
    exact in any order; weights over twenty binades make every tile's sums inexact, so that each level of the tree
    rounds, and a wrong order at any level -- inside one leaf of eight partials too -- changes bits."""
    rng = np.random.default_rng(900 + 7 * k + shape[0])
    conf = np.exp2(-rng.uniform(0.0, 20.0, shape)).astype(f32)
    c = rng.random(shape)
    conf[c < 0.03] = 0.0
    conf[(c >= 0.03) & (c < 0.05)] = np.nan
    conf.setflags(write=False)
    return conf


@functools.lru_cache(maxsize=None)
def scaled_model(view, shape, misses=False):
    """model() at another shape, under scaled_q(shape)."""
    Qm = scaled_q(shape)
    out = rc.raycast_ref(cases.fused_state(), cases.DIMS, cases.ORIGIN, cases.VS, Qm, rc.view_pose(model_pose(view)), shape,
                         depth_range=cases.DEPTH_RANGE)
    depth, normals = out["depth"][0], out["normals"][0]
    if misses:
        depth, normals = np.full_like(depth, np.nan), np.zeros_like(normals)
    return tr.model_view(depth, normals, Qm, model_pose(view))


@functools.lru_cache(maxsize=None)
def _scaled_expected(shape, schedule, k, view, model_shape, misses, confidence, extra):
    d, Q = scaled_frame(shape, k, view, run_margin(schedule))
    kw = dict(PARAMS)
    kw.update(dict(extra))
    m = model(view, misses) if model_shape == MODEL_SHAPE else scaled_model(view, model_shape, misses)
    return tr.track_ref(d, Q, start_pose(view), m, schedule=schedule, keep_tiles=True,
                        confidence=wide_confidence(shape, k) if confidence else None,
                        band_tile_rows=LIMIT_BAND if shape == LIMIT_SHAPE else None, **kw)


def scaled_expected(shape, schedule, k=0, view=TREE_VIEW, model_shape=MODEL_SHAPE, misses=False, confidence=False,
                    **extra):
    """The twin's result for scaled_frame(shape, k, view, run_margin(schedule)) against the model view of `view` (shared;
    read only), with the tile sums of its last iteration.  confidence: weighted by wide_confidence(shape, k)."""
    return _scaled_expected(shape, tuple(tuple(p) for p in schedule), k, view, model_shape, misses, confidence,
                            _freeze(extra))


def tree_expected(run):
    """scaled_expected of a run of TREE_RUNS: under wide_confidence, as tests/test_track_tree_gpu.py calls the library."""
    shape, schedule = run
    return scaled_expected(shape, schedule, confidence=True)


def sums_in_order(tiles, grid, order):
    """[31] float64: the tile sums [31, ty * tx] added in `order`: "tree", the header's; "left_to_right", one after the
    other in row-major order; "column_major", the pairs tree over the tiles taken column by column; "leaves_in_turn", the
    header's tree but for every aligned run of eight group partials, which is added one partial after the other."""
    if order == "tree":
        return tr._pairs_tree(tiles)
    if order == "left_to_right":
        return np.cumsum(tiles, axis=1)[:, -1]
    if order == "leaves_in_turn":
        part = group_partials(tiles)
        pad = np.zeros((part.shape[0], -(-part.shape[1] // 8) * 8), np.float64)
        pad[:, :part.shape[1]] = part
        return tr._pairs_tree(np.cumsum(pad.reshape(part.shape[0], -1, 8), axis=2)[:, :, -1])
    assert order == "column_major"
    K = tiles.shape[0]
    return tr._pairs_tree(np.ascontiguousarray(tiles.reshape(K, grid["ty"], grid["tx"]).transpose(0, 2, 1)).reshape(K, -1))


def group_partials(tiles):
    """[31, groups] float64: the sums of every four consecutive tiles, (t0 + t1) + (t2 + t3), as k_track_accum leaves them."""
    K, n = tiles.shape
    pad = np.zeros((K, -(-n // GROUP_TILES) * GROUP_TILES), np.float64)
    pad[:, :n] = tiles
    return tr._pairs_tree(pad.reshape(K, -1, GROUP_TILES))


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
