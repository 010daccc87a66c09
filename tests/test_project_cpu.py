"""Projection of point clouds into camera views without a GPU: the NumPy twin (tests/project_ref.py) against a plain
double loop, the round trip through reproject_ref, the KITTI ground truth the rule gives against the host path, the C
entry's refusals and size query through ctypes, and the Python layer's argument errors.  The GPU side is
tests/test_project_gpu.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import project_cases as cases
import project_ref as ref
from test_kitti_camera import _make_drive

INVALID_ARG, ERR_HIP = -1, -3


@pytest.fixture(scope="module")
def cd():
    import cuda_depth
    return cuda_depth


# ---- the twin against the loop -------------------------------------------------------------------------------------------

def _small_cloud(seed=0):
    """A few hundred points for a 9 x 14 view at f = 10: ties on equal depth, a duplicated point, points behind the
    camera, and points on and just past the image edge."""
    rng = np.random.default_rng(seed)
    H, W = 9, 14
    P = np.array([[10, 0, 6.5, 0], [0, 10, 4.0, 0], [0, 0, 0, 3.0], [0, 0, 1, 0]], dtype=np.float32)
    z = rng.choice(np.array([1.0, 1.5, 2.0, 2.5], dtype=np.float32), 300)        # few depths: many equal-depth ties
    u = rng.uniform(-3.5, W + 2.5, 300).astype(np.float32)
    v = rng.uniform(-3.5, H + 2.5, 300).astype(np.float32)
    pts = np.stack([(u - 6.5) * z / 10, (v - 4.0) * z / 10, z], 1).astype(np.float32)
    pts[50] = pts[10]                                                          # a duplicated point
    pts[60:70, 2] *= -1                                                        # behind the camera
    pts[70] = [0, 0, 0]
    pts[71] = [np.nan, 0, 1]
    pts[72] = [0, 0, np.inf]
    edge = np.array([[-6.5, -4.0, 10], [6.5, 4.0, 10], [-7.5, 0, 10], [7.5, 5.0, 10], [-8.5, -6.0, 10]], np.float32) / 10
    edge[:, 2] = 1.0                                                           # pixels (0,0), (13,8), (-1,4), (14,9), (-2,-2)
    pts[80:85] = edge
    M = np.array([[1, 0, 0, 0.01], [0, 1, 0, -0.02], [0, 0, 1, 0.0]], dtype=np.float32)
    return pts, M, P, (H, W)


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_twin_equals_the_double_loop(radius):
    pts, M, P, shape = _small_cloud()
    got = ref.project_one(pts, M, P, shape, radius=radius, depth_range=(0.5, 2.25))
    exp = ref.project_loop(pts, M, P, shape, radius=radius, depth_range=(0.5, 2.25))
    for g, e, name in zip(got, exp, ("disp", "index", "depth")):
        assert np.array_equal(g.view(np.int32), e.view(np.int32)), name
    disp, index, depth = got
    assert (index >= 0).sum() > 20
    assert np.array_equal(index < 0, np.isnan(depth)) and np.array_equal(index < 0, disp == np.float32(-1.0))
    assert not np.isin(index, np.r_[60:73]).any()                              # behind the camera, at 0, NaN, inf
    assert (depth[index >= 0] <= np.float32(2.25)).all()


def test_ties_duplicates_and_the_edge():
    pts, M, P, shape = _small_cloud()
    M = np.eye(4, dtype=np.float32)[:3]
    _, index, _ = ref.project_one(pts, M, P, shape)
    assert 50 not in index                                                     # of two equal points the first row wins
    two = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 0.5]], np.float32)
    _, idx, dep = ref.project_one(two[:2], M, P, shape)
    assert idx.max() == 0 and (idx >= 0).sum() == 1                            # equal depth: the smaller j
    _, idx, dep = ref.project_one(two, M, P, shape)
    assert idx.max() == 2 and dep[idx == 2][0] == np.float32(0.5)              # the nearer point, whatever its row
    # footprints half inside: a point one pixel outside the image lands only with radius >= 1
    out = np.array([[-7.5, 0, 10]], np.float32) / 10
    out[:, 2] = 1.0
    assert (ref.project_one(out, M, P, shape, radius=0)[1] >= 0).sum() == 0
    assert (ref.project_one(out, M, P, shape, radius=1)[1] >= 0).sum() == 3    # column 0, rows 3..5
    assert (ref.project_one(out, M, P, shape, radius=2)[1] >= 0).sum() == 10   # columns 0..1, rows 2..6
    corner = np.array([[-0.65, -0.4, 1.0]], np.float32)
    assert (ref.project_one(corner, M, P, shape, radius=2)[1] >= 0).sum() == 9


def test_offsets_are_used_clamped():
    pts, M, P, shape = _small_cloud()
    w2c = np.stack([M, M, M])
    a = ref.project_ref(pts, [5, 100, 40, 9999], w2c, P, shape)
    b = ref.project_ref(pts, [5, 100, 100, 300], w2c, P, shape)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    assert (a[1][1] == -1).all() and (a[1][0] >= 0).any()


# ---- the round trip ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(cases.ROUND_TRIPS))
def test_round_trip_inverts_reprojection(cd, name):
    Q, P, disp = cases.round_trip_case(name, cd)
    points, indices, back, index, err = cases.round_trip_twin(Q, P, disp)
    tol = 4 * err
    print(f"round trip {name}: {len(points)} points, twin relative error {err:.3g}, tolerance {tol:.3g}")
    N = len(points)
    assert N > 0.85 * disp.size
    assert np.array_equal(index.reshape(-1)[indices], np.arange(N))            # index is the inverse of indices ...
    assert (index >= 0).sum() == N                                             # ... and nothing else landed
    holes = disp[0] == np.float32(-1.0)
    assert np.array_equal(back == np.float32(-1.0), holes) and np.array_equal(index < 0, holes)
    assert 0 < err < 1e-5      # a dozen float32 roundings (6e-8 each), doubled where d + doffs cancels
    valid = ~holes
    assert (np.abs(back[valid].astype(np.float64) - disp[0][valid]) <= tol * np.abs(disp[0][valid])).all()


# ---- KITTI ---------------------------------------------------------------------------------------------------------------

def test_velodyne_projection_factors_the_image_projection(tmp_path):
    from helpers.kitti_calibration import focal_length_and_baseline, velodyne_projection, velodyne_to_image_projection
    _make_drive(str(tmp_path), frames=1, points=10)
    M, P = velodyne_projection(str(tmp_path))
    assert M.shape == (3, 4) and M.dtype == np.float32 and P.shape == (4, 4) and P.dtype == np.float32
    full = velodyne_to_image_projection(str(tmp_path))                         # [3, 4] float64
    M4 = np.vstack([M.astype(np.float64), [0, 0, 0, 1]])
    composed = P.astype(np.float64) @ M4
    assert np.allclose(composed[3], full[2], rtol=1e-6, atol=1e-6)
    assert np.allclose(composed[0], full[0] - full[2], rtol=1e-6, atol=1e-4)   # the devkit's "-1"
    assert np.allclose(composed[1], full[1] - full[2], rtol=1e-6, atol=1e-4)
    focal, baseline = focal_length_and_baseline(str(tmp_path))
    assert np.array_equal(P[2], np.array([0, 0, 0, focal * baseline], np.float32))


def test_rule_equals_host_ground_truth_on_the_collision_free_scan(tmp_path):
    _make_drive(str(tmp_path), frames=1, points=10)
    scan = cases.collision_free_scan(str(tmp_path))
    velo = os.path.join(tmp_path, "scan", "0.bin")
    cases.write_scan(velo, scan)
    host = cases.host_ground_truth(str(tmp_path), velo)
    twin = cases.twin_ground_truth(str(tmp_path), velo)
    print(f"collision-free scan: {len(scan)} returns, {np.count_nonzero(host)} pixels hit")
    assert len(scan) > 25000 and np.count_nonzero(host) > 15000
    assert host.dtype == twin.dtype == np.float64
    assert np.array_equal(host.view(np.int64), twin.view(np.int64))            # all 465 750 pixels, bit for bit


def test_rule_equals_host_ground_truth_where_one_return_lands(tmp_path):
    from helpers.kitti_calibration import load_velodyne_scan, velodyne_to_image_projection
    drive, _ = _make_drive(str(tmp_path), frames=1, points=6000, seed=2)
    velo = os.path.join(drive, "velodyne_points/data", "0000000000.bin")
    host = cases.host_ground_truth(str(tmp_path), velo)
    twin = cases.twin_ground_truth(str(tmp_path), velo)
    H, W = cases.KITTI_SHAPE
    scan = load_velodyne_scan(velo)
    scan = scan[scan[:, 0] >= 0]
    proj = (velodyne_to_image_projection(str(tmp_path)) @ scan.T).T
    col, row = np.round(proj[:, 0] / proj[:, 2]) - 1, np.round(proj[:, 1] / proj[:, 2]) - 1
    inside = (col >= 0) & (row >= 0) & (col < W) & (row < H)
    hits = np.bincount((row[inside] * W + col[inside]).astype(np.int64), minlength=H * W).reshape(H, W)
    once = hits == 1
    print(f"drive scan: {inside.sum()} returns in the image, {once.sum()} pixels hit once, {(hits > 1).sum()} more often")
    assert once.sum() > 500 and (hits > 1).sum() > 50
    assert np.array_equal(host[once].view(np.int64), twin[once].view(np.int64))
    assert np.array_equal(host[hits == 0], twin[hits == 0])                    # and nothing where nothing lands


# ---- the C entry ---------------------------------------------------------------------------------------------------------

def _valid_call():
    """Arguments smx_project_points accepts, with invented disjoint device addresses: n 2, capacity 100, 8 x 16."""
    P = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1).tolist())
    return dict(device_id=0, n=2, capacity=100, H=8, W=16, points=0x10000, offsets=0x20000, world_to_camera=0x30000,
                P=P, radius=1, z_min=0.0, z_max=math.inf, invalid_disparity=-1.0, disp=0x40000, index=0x50000,
                depth=0x60000, workspace=0x70000, workspace_bytes=1 << 20, stream=None)


def _call(native, **changes):
    a = _valid_call()
    a.update(changes)
    rc = native.LIB.smx_project_points(*a.values())
    return rc, native.last_error()


def _bad_p(k, v):
    P = np.eye(4, dtype=np.float32).reshape(-1)
    P[k] = v
    return (C.c_float * 16)(*P.tolist())


REFUSALS = [
    ("null points", dict(points=None), "must be non-NULL"),
    ("null offsets", dict(offsets=None), "must be non-NULL"),
    ("null world_to_camera", dict(world_to_camera=None), "must be non-NULL"),
    ("null P", dict(P=None), "must be non-NULL"),
    ("null disp", dict(disp=None), "must be non-NULL"),
    ("null workspace", dict(workspace=None), "must be non-NULL"),
    ("n 0", dict(n=0), "1 <= n <= 65536"),
    ("n 65537", dict(n=65537), "1 <= n <= 65536"),
    ("capacity 0", dict(capacity=0), "capacity"),
    ("capacity 2^30 + 1", dict(capacity=2 ** 30 + 1), "capacity"),
    ("H 0", dict(H=0), "H, W"),
    ("W 32769", dict(W=32769), "H, W"),
    ("pixels", dict(n=2, H=32768, W=32768), "exceeds 2^30"),
    ("radius -1", dict(radius=-1), "radius must be in 0..8"),
    ("radius 9", dict(radius=9), "radius must be in 0..8"),
    ("P inf", dict(P=_bad_p(5, np.inf)), "P[5]"),
    ("P nan", dict(P=_bad_p(15, np.nan)), "P[15]"),
    ("z_min nan", dict(z_min=math.nan), "z_min <= z_max"),
    ("z_max nan", dict(z_max=math.nan), "z_min <= z_max"),
    ("z order", dict(z_min=2.0, z_max=1.0), "z_min <= z_max"),
    ("invalid nan", dict(invalid_disparity=math.nan), "invalid"),
    ("invalid inf", dict(invalid_disparity=math.inf), "invalid"),
    ("workspace small", dict(workspace_bytes=2 * 8 * 16 * 8), "workspace_bytes"),
    ("disp on points", dict(disp=0x10000 + 1196), "overlaps an input"),
    ("index on offsets", dict(index=0x20000 + 8), "overlaps an input"),
    ("depth on poses", dict(depth=0x30000 + 92), "overlaps an input"),
    ("workspace on points", dict(workspace=0x10000, workspace_bytes=4096), "overlaps an input"),
    ("disp on index", dict(index=0x40000 + 1020), "overlap"),
    ("depth on disp", dict(depth=0x40000), "overlap"),
    ("workspace on depth", dict(workspace=0x60000 + 768), "overlap"),
    ("workspace unaligned", dict(workspace=0x70000 + 128), "256-byte aligned"),
    ("engine stream", dict(stream=C.c_void_p(-1)), "caller stream"),
]


@pytest.mark.parametrize("name,changes,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_entry_refuses(cd, name, changes, text):
    rc, msg = _call(cd._native, **changes)
    assert rc == INVALID_ARG and text in msg, (rc, msg)


def test_the_entry_accepts_the_valid_call_up_to_the_device(cd):
    import torch
    if torch.cuda.is_available():
        return           # it would launch kernels on invented addresses; tests/test_project_gpu.py makes real calls
    for changes in ({}, dict(index=None, depth=None), dict(radius=0), dict(radius=8),
                    dict(disp=0x10000 + 1200), dict(workspace_bytes=2 * 8 * 16 * 8 + 256)):
        rc, msg = _call(cd._native, **changes)
        assert rc == ERR_HIP and "cannot select HIP device" in msg, (changes, rc, msg)


def test_workspace_query(cd):
    q = cd._native.LIB.smx_project_workspace_bytes
    r256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for n, H, W in ((1, 1, 1), (2, 8, 16), (3, 33, 257), (32, 375, 1242), (65536, 128, 128), (1, 32768, 32768)):
        assert q(n, H, W) == r256(8 * n * H * W) + r256(4 * (n + 1)), (n, H, W)    # 8 bytes per pixel + the offsets
    for n, H, W in ((0, 8, 8), (-1, 8, 8), (65537, 8, 8), (1, 0, 8), (1, 8, 0), (1, 32769, 8), (1, 8, 32769),
                    (2, 32768, 32768), (65536, 128, 129)):
        assert q(n, H, W) == 0, (n, H, W)
    assert cd._native.LIB.smx_abi_version() == 4


# ---- the Python layer ----------------------------------------------------------------------------------------------------

def test_python_validation_before_the_device(cd):
    import torch
    pts, off = torch.zeros((4, 3)), torch.zeros(2, dtype=torch.int32)
    Q = cd.reprojection_matrix(700.0, 300.0, 200.0, 0.5)
    eye = np.eye(4)[None]
    f = cd.project_points_batched
    with pytest.raises(RuntimeError, match="exactly one of Q and P"):
        f(pts, off, Q, eye, (4, 8), P=np.eye(4))
    with pytest.raises(RuntimeError, match="exactly one of Q and P"):
        f(pts, off, None, eye, (4, 8))
    with pytest.raises(RuntimeError, match="Q must be a numeric 4x4"):
        f(pts, off, np.eye(3), eye, (4, 8))
    with pytest.raises(RuntimeError, match="singular"):
        f(pts, off, np.zeros((4, 4)), eye, (4, 8))
    with pytest.raises(RuntimeError, match="P must be a numeric 4x4"):
        f(pts, off, None, eye, (4, 8), P=np.eye(3))
    with pytest.raises(RuntimeError, match="P must be finite"):
        f(pts, off, None, eye, (4, 8), P=np.full((4, 4), np.nan))
    with pytest.raises(RuntimeError, match="depth_range"):
        f(pts, off, Q, eye, (4, 8), depth_range=(2.0, 1.0))
    with pytest.raises(TypeError, match="depth_range"):
        f(pts, off, Q, eye, (4, 8), depth_range=3.0)
    with pytest.raises(RuntimeError, match="invalid_disparity"):
        f(pts, off, Q, eye, (4, 8), invalid_disparity=math.nan)
    with pytest.raises(TypeError, match="radius"):
        f(pts, off, Q, eye, (4, 8), radius=1.0)
    with pytest.raises(RuntimeError, match="radius must be in 0..8"):
        f(pts, off, Q, eye, (4, 8), radius=9)
    with pytest.raises(TypeError, match="index must be a bool"):
        f(pts, off, Q, eye, (4, 8), index=1)
    with pytest.raises(TypeError, match="depth must be a bool"):
        f(pts, off, Q, eye, (4, 8), depth=None)
    with pytest.raises(RuntimeError, match="last row"):
        f(pts, off, Q, np.ones((1, 4, 4)), (4, 8))
    with pytest.raises(RuntimeError, match="exactly one of camera_to_world and world_to_camera"):
        f(pts, off, Q, eye, (4, 8), world_to_camera=np.zeros((1, 3, 4)))
    with pytest.raises(RuntimeError, match="world_to_camera must be a numeric"):
        f(pts, off, Q, None, (4, 8), world_to_camera=np.zeros((3, 4)))
    with pytest.raises(TypeError, match="shape"):
        f(pts, off, Q, eye, 8)
    with pytest.raises(ValueError, match="shape"):
        f(pts, off, Q, eye, (0, 8))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        f(pts, off, Q, eye, (4, 8))
    with pytest.raises(TypeError, match="PointCloud or an"):
        cd.project_points(np.zeros((4, 3)), Q, shape=(4, 8))
    with pytest.raises(TypeError, match="shape"):
        cd.project_points(pts, Q)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        cd.project_points(cd.PointCloud(points=pts), Q, shape=(4, 8))
    v = cd.ProjectedView(disparity=torch.zeros((4, 8)))
    assert v.index is None and v.depth is None and v.colors is None
    assert hasattr(cd.TSDFVolume, "integrate_points")
