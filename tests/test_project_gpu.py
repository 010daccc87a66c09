"""Projection of point clouds into camera views on the device (include/stereo_mi355x.h: smx_project_points), bit for bit
against the NumPy twin (tests/project_ref.py): tiny, odd and batched shapes with every radius and plane selection,
contention on a handful of pixels, run-to-run and batch independence, row order, unaligned points, clamped offsets,
batches of 700 and of 65536 tiny and empty clouds, the round trip through reproject_to_3d_batched, graph replay, TSDFVolume.integrate_points and the KITTI ground truth."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import project_cases as cases                       # noqa: E402
import project_ref as ref                           # noqa: E402
from test_kitti_camera import _make_drive           # noqa: E402

F, B = 60.0, 0.3


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_planes(got, expect, what):
    """(disp, index, depth) against the twin's, bit for bit; a plane that was not asked for is None."""
    for g, e, name in zip(got, expect, ("disp", "index", "depth")):
        if g is None:
            continue
        g = g.cpu().numpy()
        assert g.shape == e.shape and g.dtype == e.dtype, f"{what}: {name} {g.shape} {g.dtype}"
        bad = np.argwhere(g.view(np.int32) != e.view(np.int32))
        assert bad.size == 0, f"{what}: {len(bad)} values of {name} differ, first at {tuple(bad[0])}"


def q_matrix(cd, H, W):
    return cd.reprojection_matrix(F, (W - 1) / 2.0 + 0.25, (H - 1) / 2.0 - 0.5, B, fy=F * 1.01)


def poses(rng, n):
    """n camera-to-world poses near the identity: a few degrees and centimetres."""
    out = np.tile(np.eye(4), (n, 1, 1))
    for m in out:
        a, b, c = rng.uniform(-0.05, 0.05, 3)
        rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
        ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
        rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
        m[:3, :3] = rx @ ry @ rz
        m[:3, 3] = rng.uniform(-0.05, 0.05, 3)
    return out


def cloud(rng, count, H, W, Q):
    """`count` points that mostly land in an H x W view from near the identity (some around it, some behind the camera,
    a NaN and an infinity), at depths drawn from a coarse grid so that equal depths meet."""
    u = rng.uniform(-6.0, W + 5.0, count)
    v = rng.uniform(-6.0, H + 5.0, count)
    z = np.round(rng.uniform(0.4, 6.0, count), 1)
    z[rng.random(count) < 0.03] *= -1
    fx, fy, cx, cy = float(Q[2, 3]), float(Q[2, 3] / Q[1, 1]), -float(Q[0, 3]), -float(Q[1, 3] / Q[1, 1])
    pts = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1).astype(np.float32)
    if count > 40:
        pts[7] = [np.nan, 0, 1]
        pts[11] = [0, np.inf, 2]
        pts[13] = pts[3]
    return pts


def batch(rng, counts, H, W, Q):
    pts = np.concatenate([cloud(rng, c, H, W, Q) for c in counts] + [np.zeros((1, 3), np.float32)])
    return pts, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def run(cd, pts, off, Q, c2w, shape, **kw):
    out = cd.project_points_batched(dev(pts), dev(np.asarray(off, dtype=np.int32)), Q, c2w, shape, **kw)
    torch.cuda.synchronize()
    return out


SHAPES = {"one": (1, 1, 1, [1]), "odd": (1, 7, 13, [257]), "workgroup_edges": (3, 33, 257, [0, 255, 65537]),
          "batch32": (32, 24, 70, [300] * 32)}
_scenes = {}


def scene(cd, name):
    """(pts, off, Q, P, c2w, w2c) of a shape, made once."""
    if name not in _scenes:
        n, H, W, counts = SHAPES[name]
        rng = np.random.default_rng(len(name))
        Q = q_matrix(cd, H, W)
        pts, off = batch(rng, counts, H, W, Q)
        c2w = poses(rng, n)
        if name == "one":                                                      # one point that lands on the one pixel
            pts[0], c2w = [0.0, 0.005, 1.0], np.eye(4)[None]
        _scenes[name] = (pts, off, Q, cd.projection_matrix(Q), c2w, cd.world_to_camera_poses(c2w))
    return _scenes[name]


_expected = {}


def expected(cd, name, radius):
    """The twin's planes for a shape and a radius, computed once and shared by the plane selections."""
    if (name, radius) not in _expected:
        pts, off, Q, P, _, w2c = scene(cd, name)
        _expected[name, radius] = ref.project_ref(pts, off, w2c, P, SHAPES[name][1:3], radius=radius,
                                                  depth_range=(0.5, 5.5))
    return _expected[name, radius]


@pytest.mark.parametrize("planes", [(True, True), (False, False)], ids=["index_depth", "disp_only"])
@pytest.mark.parametrize("radius", [0, 1, 2, 8])
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_bitwise(cd, name, radius, planes):
    pts, off, Q, _, c2w, _ = scene(cd, name)
    got = run(cd, pts, off, Q, c2w, SHAPES[name][1:3], radius=radius, depth_range=(0.5, 5.5), index=planes[0],
              depth=planes[1])
    assert (got[1] is None) == (not planes[0]) and (got[2] is None) == (not planes[1])
    e = expected(cd, name, radius)
    assert (e[1] >= 0).any() and (radius > 0 or name == "one" or (e[1] < 0).any())
    assert_planes(got, e, f"{name} radius {radius}")


def test_contention_on_a_few_pixels(cd):
    rng = np.random.default_rng(5)
    H, W = 5, 7
    Q = q_matrix(cd, H, W)
    pts, off = batch(rng, [50000], H, W, Q)
    eye = np.eye(4)[None]
    w2c = cd.world_to_camera_poses(eye)
    for radius in (0, 2):
        got = run(cd, pts, off, Q, eye, (H, W), radius=radius, depth=True)
        assert_planes(got, ref.project_ref(pts, off, w2c, cd.projection_matrix(Q), (H, W), radius=radius),
                      f"50 000 points on 5 x 7, radius {radius}")
    # 100 000 points of one depth on one pixel: the lowest row wins
    same = np.tile(np.array([[0.0, 0.0, 2.0]], np.float32), (100000, 1))
    Q1 = cd.reprojection_matrix(F, 0.0, 0.0, B)
    disp, index, depth = run(cd, same, [0, 100000], Q1, eye, (1, 1), depth=True)
    assert int(index[0, 0, 0]) == 0 and float(depth[0, 0, 0]) == 2.0
    assert_planes((disp, index, depth), ref.project_ref(same, [0, 100000], w2c, cd.projection_matrix(Q1), (1, 1)), "one pixel")


def test_two_runs_give_the_same_bits(cd):
    pts, off, Q, _, c2w, _ = scene(cd, "workgroup_edges")
    a = run(cd, pts, off, Q, c2w, (33, 257), radius=2, depth=True)
    b = run(cd, pts, off, Q, c2w, (33, 257), radius=2, depth=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_a_cloud_alone_equals_the_cloud_in_the_batch(cd):
    pts, off, Q, _, c2w, _ = scene(cd, "batch32")
    together = run(cd, pts, off, Q, c2w, (24, 70), radius=1, depth=True)
    for f in (0, 13, 31):
        alone = run(cd, pts[off[f]:off[f + 1]], [0, off[f + 1] - off[f]], Q, c2w[f:f + 1], (24, 70), radius=1, depth=True)
        for x, y in zip(alone, together):
            assert torch.equal(x[0].view(torch.int32), y[f].view(torch.int32)), f
    pts, off, Q, _, c2w, _ = scene(cd, "workgroup_edges")
    together = run(cd, pts, off, Q, c2w, (33, 257), depth=True)
    alone = run(cd, pts[off[2]:off[3]], [0, off[3] - off[2]], Q, c2w[2:3], (33, 257), depth=True)
    for x, y in zip(alone, together):
        assert torch.equal(x[0].view(torch.int32), y[2].view(torch.int32))


def test_row_order_changes_only_the_index(cd):
    rng = np.random.default_rng(9)
    H, W, N = 20, 31, 4000
    Q = q_matrix(cd, H, W)
    pts = cloud(rng, N, H, W, Q)
    ok = np.isfinite(pts).all(axis=1)
    pts = pts[ok]
    N = len(pts)
    xy = pts[:, :2] / pts[:, 2:3]
    pts[:, 2] = rng.permutation(np.linspace(0.5, 6.0, N).astype(np.float32))   # every depth once: no ties at the identity,
    pts[:, :2] = xy * pts[:, 2:3]                                              # where c_2 is z itself
    assert len(np.unique(pts[:, 2])) == N
    eye = np.eye(4)[None]
    perm = rng.permutation(N)
    a = run(cd, pts, [0, N], Q, eye, (H, W), radius=1, depth=True)
    b = run(cd, pts[perm], [0, N], Q, eye, (H, W), radius=1, depth=True)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    ia, ib = a[1].cpu().numpy(), b[1].cpu().numpy()
    assert np.array_equal(ia < 0, ib < 0) and (ia >= 0).sum() > 300
    assert np.array_equal(perm[ib[ib >= 0]], ia[ia >= 0]) and not np.array_equal(ia, ib)


@pytest.mark.parametrize("shift", [1, 2], ids=["4_bytes", "8_bytes"])
def test_points_need_only_their_element_alignment(cd, shift):
    pts, off, Q, _, c2w, w2c = scene(cd, "odd")
    flat = torch.zeros(pts.size + 8, dtype=torch.float32, device="cuda")
    view = flat[shift:shift + pts.size].view(-1, 3)
    view.copy_(dev(pts))
    assert view.data_ptr() % 16 == 4 * shift and view.is_contiguous()
    got = cd.project_points_batched(view, dev(off), Q, c2w, (7, 13), radius=1, depth=True)
    torch.cuda.synchronize()
    assert_planes(got, ref.project_ref(pts, off, w2c, cd.projection_matrix(Q), (7, 13), radius=1),
                  f"points + {4 * shift} bytes")


def test_device_offsets_are_clamped(cd):
    pts, off, Q, P, c2w, w2c = scene(cd, "workgroup_edges")
    cap = len(pts)
    for raw in ([5, 300, 40, 2 ** 31 - 1], [-7, 65000, 300, cap + 5], [cap + 1, 3, 2, 1], [0, 0, 0, 0]):
        got = run(cd, pts, raw, Q, c2w, (33, 257), radius=1, depth=True)
        clamped = ref.clamp_offsets(raw, cap)
        assert_planes(got, ref.project_ref(pts, clamped, w2c, P, (33, 257), radius=1), f"offsets {raw}")


# ---- many clouds, most of them tiny or empty ----------------------------------------------------------------------------
# k_project_clear clamps the n + 1 offsets with 256 threads, per = (n + 256) // 256 entries each: the loop inside a thread
# and the carry from one thread's share into the next exist from n = 256 on.  k_project_splat's search between the
# workgroup's first and last cloud has more than two clouds to choose from only where clouds are shorter than 256 rows.

def alone_equals_batch(cd, pts, off, Q, w2c, shape, together, clouds, radius):
    for f in clouds:
        assert off[f + 1] > off[f], f
        alone = run(cd, pts[off[f]:off[f + 1]], [0, off[f + 1] - off[f]], Q, None, shape, radius=radius, depth=True,
                    world_to_camera=w2c[f:f + 1])
        for x, y in zip(alone, together):
            assert torch.equal(x[0].view(torch.int32), y[f].view(torch.int32)), f


@pytest.fixture(scope="module")
def tiny700(cd):
    """700 clouds of 0..6 points into 3 x 5 views: (pts, off, cloud after the empty run, Q, P, w2c)."""
    n, H, W = 700, 3, 5
    Q = q_matrix(cd, H, W)
    pts, off, after = cases.tiny_clouds(700, n, 6, H, W, Q)
    w2c = cd.world_to_camera_poses(poses(np.random.default_rng(701), n))
    assert (np.diff(off) == 0).sum() > 100 and np.diff(off).max() == 6 and len(pts) > 256 * 6
    return pts, off, after, Q, cd.projection_matrix(Q), w2c


@pytest.mark.parametrize("radius", [0, 1])
def test_700_tiny_clouds(cd, tiny700, radius):
    pts, off, after, Q, P, w2c = tiny700
    got = run(cd, pts, off, Q, None, (3, 5), radius=radius, depth=True, world_to_camera=w2c)
    e = ref.project_ref(pts, off, w2c, P, (3, 5), radius=radius)
    assert (e[1] >= 0).sum() > 300 and len({int(f) for f in np.argwhere(e[1] >= 0)[:, 0]}) > 200
    assert_planes(got, e, f"700 tiny clouds, radius {radius}")
    assert off[after] == off[after - 40], "a run of empty clouds before it"
    full = np.flatnonzero(np.diff(off) > 0)
    alone_equals_batch(cd, pts, off, Q, w2c, (3, 5), got, (int(full[0]), after, int(full[-1])), radius)


@pytest.mark.parametrize("radius", [0, 1])
def test_700_tiny_clouds_with_offsets_to_clamp(cd, tiny700, radius):
    pts, off, _, Q, P, w2c = tiny700
    cap = len(pts)
    raw = cases.unruly_offsets(off, cap)
    clamped = ref.clamp_offsets(raw, cap)
    assert (np.diff(raw.astype(np.int64)) < 0).sum() >= 6 and raw.min() < 0 and raw.max() > cap
    assert (clamped != off).sum() > 150 and (np.diff(clamped) > 0).sum() > 250 and clamped[-1] == cap
    got = run(cd, pts, raw, Q, None, (3, 5), radius=radius, depth=True, world_to_camera=w2c)
    e = ref.project_ref(pts, clamped, w2c, P, (3, 5), radius=radius)
    assert not all(np.array_equal(a, b) for a, b in zip(e, ref.project_ref(pts, off, w2c, P, (3, 5), radius=radius)))
    assert_planes(got, e, f"700 tiny clouds, clamped offsets, radius {radius}")


def test_as_many_clouds_as_the_entry_takes(cd):
    """n = 65536, the documented limit: 257 offsets per clamping thread, clouds of 0..2 points into 1 x 2 views."""
    import time
    n, H, W = 65536, 1, 2
    Q = q_matrix(cd, H, W)
    pts, off, after = cases.tiny_clouds(65536, n, 2, H, W, Q)
    w2c = cases.near_identity_views(65537, n)
    got = run(cd, pts, off, Q, None, (H, W), depth=True, world_to_camera=w2c)
    t = time.perf_counter()
    e = ref.project_ref(pts, off, w2c, cd.projection_matrix(Q), (H, W))
    print(f"the twin's time for {n} clouds: {time.perf_counter() - t:.1f} s")
    assert (e[1] >= 0).sum() > 5000 and (e[1][n // 2:] >= 0).sum() > 2500
    assert_planes(got, e, f"{n} clouds")
    full = np.flatnonzero(np.diff(off) > 0)
    alone_equals_batch(cd, pts, off, Q, w2c, (H, W), got, (int(full[0]), after, int(full[-1])), 0)


@pytest.mark.parametrize("name", list(cases.ROUND_TRIPS))
def test_round_trip_on_the_device(cd, name):
    Q, P, disp = cases.round_trip_case(name, cd)
    _, indices, back, index, err = cases.round_trip_twin(Q, P, disp)
    tol = 4 * err
    _, H, W = disp.shape
    points, _, idx, offsets, _ = cd.reproject_to_3d_batched(dev(disp), Q)
    got = cd.project_points_batched(points, offsets, Q, np.eye(4)[None], (H, W), depth=True)
    torch.cuda.synchronize()
    N = int(offsets[1])
    g_disp, g_index = got[0][0].cpu().numpy(), got[1][0].cpu().numpy()
    assert N == len(indices) and np.array_equal(idx[:N].cpu().numpy(), indices)
    assert np.array_equal(g_index.reshape(-1)[indices], np.arange(N)) and (g_index >= 0).sum() == N
    holes = disp[0] == np.float32(-1.0)
    assert np.array_equal(g_disp == np.float32(-1.0), holes)
    rel = np.abs(g_disp[~holes].astype(np.float64) - disp[0][~holes]) / np.abs(disp[0][~holes])
    print(f"round trip {name}: device relative error {rel.max():.3g}, tolerance {tol:.3g} (4 x the twin's {err:.3g})")
    assert rel.max() <= tol
    assert np.array_equal(g_disp.view(np.int32), back.view(np.int32)) and np.array_equal(g_index, index)


def test_graph_replay(cd):
    native = cd._native
    pts, off, Q, P, c2w, w2c = scene(cd, "workgroup_edges")
    n, H, W = 3, 33, 257
    tp, to, tw = dev(pts), dev(off), dev(w2c)
    disp = torch.zeros((n, H, W), dtype=torch.float32, device="cuda")
    index = torch.zeros((n, H, W), dtype=torch.int32, device="cuda")
    depth = torch.zeros((n, H, W), dtype=torch.float32, device="cuda")
    ws_bytes = native.LIB.smx_project_workspace_bytes(n, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    pc = (C.c_float * 16)(*P.reshape(-1).tolist())
    eager = run(cd, pts, off, Q, c2w, (H, W), radius=1, depth=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        rc = native.LIB.smx_project_points(0, n, len(pts), H, W, tp.data_ptr(), to.data_ptr(), tw.data_ptr(), pc, 1, 0.0,
                                           math.inf, -1.0, disp.data_ptr(), index.data_ptr(), depth.data_ptr(),
                                           ws.data_ptr(), ws_bytes, C.c_void_p(s.cuda_stream))
    assert rc == 0, native.last_error()
    for f in range(2):
        p2 = pts if f == 0 else pts[::-1].copy()
        tp.copy_(dev(p2))
        ws.fill_(f)                                                            # nothing in the workspace survives a call
        graph.replay()
        torch.cuda.synchronize()
        e = eager if f == 0 else None
        assert_planes((disp, index, depth), ref.project_ref(p2, off, w2c, P, (H, W), radius=1), f"replay {f}")
        if e is not None:
            for x, y in zip((disp, index, depth), e):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_project_points_and_integrate_points(cd):
    rng = np.random.default_rng(21)
    H, W = 24, 32
    Q = cd.reprojection_matrix(40.0, 15.5, 11.5, 0.1)
    pts = cloud(rng, 3000, H, W, Q)
    near = np.abs(pts[:, 2]) * np.float32(0.1) + np.float32(0.3)             # 0.3 .. 0.9 m: inside the volume below
    pts[:, :2] *= (near / pts[:, 2])[:, None]
    pts[:, 2] = near
    colors = rng.integers(0, 256, (len(pts), 3)).astype(np.uint8)
    pose = poses(rng, 1)[0]
    pc = cd.PointCloud(points=dev(pts), colors=dev(colors))
    view = cd.project_points(pc, Q, pose, shape=(H, W), radius=1, depth=True)
    torch.cuda.synchronize()
    e = ref.project_ref(pts, [0, len(pts)], cd.world_to_camera_poses(pose), cd.projection_matrix(Q), (H, W), radius=1)
    assert_planes((view.disparity[None], view.index[None], view.depth[None]), e, "project_points")
    gathered = np.where((e[1][0] >= 0)[..., None], colors[np.maximum(e[1][0], 0)], 0).transpose(2, 0, 1)
    assert view.colors.dtype == torch.uint8 and np.array_equal(view.colors.cpu().numpy(), gathered)
    bare = cd.project_points(dev(pts), Q, shape=(H, W), index=False)          # a tensor, the identity pose
    assert bare.colors is None and bare.index is None and bare.depth is None
    assert_planes((bare.disparity[None],), ref.project_ref(pts, [0, len(pts)], np.eye(4, dtype=np.float32)[None, :3],
                                                           cd.projection_matrix(Q), (H, W))[:1], "tensor cloud")
    empty = cd.project_points(cd.PointCloud(points=dev(pts[:0]), colors=dev(colors[:0])), Q, shape=(H, W))
    assert bool((empty.disparity == -1).all()) and bool((empty.index == -1).all()) and int(empty.colors.sum()) == 0

    def volume():
        return cd.TSDFVolume((8, 8, 8), 0.15, (-0.6, -0.6, 0.2), color=True)
    a, b = volume(), volume()
    a.integrate_points(pc, Q, pose, (H, W), radius=1, depth_range=(0.2, 1.5))
    v = cd.project_points(pc, Q, pose, shape=(H, W), radius=1, depth_range=(0.2, 1.5))
    b.integrate(v.disparity, Q, pose, image=v.colors, depth_range=(0.2, 1.5))
    torch.cuda.synchronize()
    assert float(a.weight.sum()) > 20
    assert torch.equal(a.tsdf.view(torch.int32), b.tsdf.view(torch.int32))
    assert torch.equal(a.weight.view(torch.int32), b.weight.view(torch.int32)) and torch.equal(a.color, b.color)


def test_python_errors_on_the_device(cd):
    pts, off = torch.zeros((4, 3), device="cuda"), torch.tensor([0, 4], dtype=torch.int32, device="cuda")
    Q, eye = q_matrix(cd, 4, 8), np.eye(4)[None]
    with pytest.raises(RuntimeError, match="points must be float32"):
        cd.project_points_batched(pts.double(), off, Q, eye, (4, 8))
    with pytest.raises(RuntimeError, match="offsets must be int32"):
        cd.project_points_batched(pts, off.long(), Q, eye, (4, 8))
    with pytest.raises(RuntimeError, match="need 1 pose"):
        cd.project_points_batched(pts, off, Q, np.tile(np.eye(4), (2, 1, 1)), (4, 8))
    with pytest.raises(RuntimeError, match="colors must be uint8"):
        cd.project_points(cd.PointCloud(points=pts, colors=torch.zeros((3, 3), dtype=torch.uint8, device="cuda")), Q,
                          shape=(4, 8))


# ---- KITTI ground truth ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kitti_drive(tmp_path_factory):
    """A one-frame drive whose scan is the collision-free one: (calibration directory, drive, scan file)."""
    root = str(tmp_path_factory.mktemp("kitti"))
    drive, _ = _make_drive(root, frames=1, points=10)
    velo = os.path.join(drive, "velodyne_points/data", "0000000000.bin")
    cases.write_scan(velo, cases.collision_free_scan(root))
    return root, drive, velo


def test_kitti_ground_truth_on_the_device(cd, kitti_drive):
    from helpers.kitti_calibration import velodyne_disparity_map_device
    from pipeline.camera import KittiSingleViewCamera
    root, drive, velo = kitti_drive
    host = cases.host_ground_truth(root, velo)
    got = velodyne_disparity_map_device(root, velo, cases.KITTI_SHAPE, "cuda")
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == cases.KITTI_SHAPE
    assert np.count_nonzero(host) > 15000
    differ = int((got.cpu().numpy().view(np.int64) != host.view(np.int64)).sum())
    print(f"device ground truth: {int((got > 0).sum())} pixels hit, {differ} differ from the host path")
    assert differ == 0
    _, _, gt = next(iter(KittiSingleViewCamera(drive, gt_on_device=True).stream_image_pairs_with_gt_disparity()))
    _, _, gt_host = next(iter(KittiSingleViewCamera(drive).stream_image_pairs_with_gt_disparity()))
    assert gt.is_cuda and gt.dtype == torch.float64 and tuple(gt.shape) == (384, 1280) and not gt_host.is_cuda
    assert torch.equal(gt.cpu().view(torch.int64), gt_host.view(torch.int64))
    assert np.array_equal(gt[5:380, 19:1261].cpu().numpy(), host)


def test_kitti_evaluation_is_the_same_with_the_ground_truth_on_the_device(cd, kitti_drive):
    from pipeline import DepthEstimationPipeline
    from pipeline.camera import KittiSingleViewCamera
    from pipeline.depth_estimation_pipeline_metrics import D1Metric, MAEMetric, ThresholdMetric
    from pipeline.depth_estimation_pipeline_runner import (extract_config_from_camera,
                                                           run_depth_estimation_pipeline_evaluation)
    _, drive, _ = kitti_drive
    results = []
    for on_device in (False, True):
        cam = KittiSingleViewCamera(drive, return_right_view=True, only_one=True, gt_on_device=on_device)
        pipe = DepthEstimationPipeline(extract_config_from_camera(cam))
        metrics = [D1Metric(), ThresholdMetric(1), ThresholdMetric(2), ThresholdMetric(3), ThresholdMetric(5), MAEMetric()]
        results.append(run_depth_estimation_pipeline_evaluation(cam, pipe, metrics, verbose=False))
    assert len(results[0]) == 6 and all(math.isfinite(v) for v in results[0].values())
    assert results[0] == results[1]
