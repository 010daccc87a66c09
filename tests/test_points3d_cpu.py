"""Metric 3D points and voxel downsampling without a GPU: the NumPy reference (tests/points3d_ref.py) against float64
reprojection, hand-computed pixels and a dictionary brute force; geometry round trips; PLY files; the calibration
builders of Q; the C ABI's declarations, exports and argument checks; Python validation and the pipeline's keyword
defaults."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import points3d_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stereo_mi355x.h")
F, B = 721.5, 0.54
NEW_SYMBOLS = ("smx_reproject_points", "smx_reproject_workspace_bytes", "smx_voxel_downsample",
               "smx_voxel_workspace_bytes")


@pytest.fixture(scope="module")
def cd():
    import cuda_depth
    return cuda_depth


def test_reprojection_matrix_layout(cd):
    q = cd.reprojection_matrix(700.0, 300.0, 200.0, 0.5, fy=710.0, cx_right=320.0)
    assert q.dtype == np.float32 and q.shape == (4, 4)
    e = np.array([[1, 0, 0, -300], [0, 700 / 710, 0, -200 * 700 / 710], [0, 0, 0, 700], [0, 0, 2, 40]], np.float64)
    assert np.array_equal(q, e.astype(np.float32))
    with pytest.raises(RuntimeError, match="baseline"):
        cd.reprojection_matrix(700.0, 300.0, 200.0, 0.0)
    with pytest.raises(RuntimeError, match="fx and fy"):
        cd.reprojection_matrix(-1.0, 300.0, 200.0, 0.5)
    with pytest.raises(TypeError):
        cd.reprojection_matrix("700", 300.0, 200.0, 0.5)


def test_reference_against_float64_and_hand_pixels(cd):
    rng = np.random.default_rng(1)
    n, H, W = 2, 20, 30
    d = rng.uniform(1.0, 90.0, (n, H, W)).astype(np.float32)
    Q = cd.reprojection_matrix(F, 14.5, 9.5, B, cx_right=14.5 + 2.25)        # doffs = 2.25
    pts, _, idx, off, xyz = ref.reproject_ref(d, Q)
    assert off.tolist() == [0, H * W, 2 * H * W]
    v, u = np.divmod(idx[:H * W], W)
    d0 = d[0].reshape(-1).astype(np.float64)
    Z = F * B / (d0 + 2.25)
    X = (u - 14.5) * Z / F
    Y = (v - 9.5) * Z / F
    e = np.stack([X, Y, Z], 1)
    assert np.allclose(pts[:H * W], e, rtol=4 * np.finfo(np.float32).eps, atol=1e-6)
    # hand-computed pixel: row 3, column 7 with d = 10 and an exact Q
    Q2 = np.array([[1, 0, 0, -7], [0, 1, 0, -2], [0, 0, 0, 100], [0, 0, 0.5, 0]], np.float32)
    dd = np.full((1, 4, 8), -1.0, np.float32)
    dd[0, 3, 7] = 10.0
    dd[0, 0, 0] = 4.0
    p, _, i, o, xyz = ref.reproject_ref(dd, Q2)
    assert i.tolist() == [0, 31] and o.tolist() == [0, 2]
    assert p.tolist() == [[-3.5, -1.0, 50.0], [0.0, 0.2, 20.0]] or np.allclose(p, [[-3.5, -1.0, 50.0], [0.0, 0.2, 20.0]])
    assert np.isnan(xyz[0, 1, 1]).all() and xyz[0, 3, 7].tolist() == [0.0, np.float32(1 / 5.0).item() * 1.0, 20.0] \
        or np.allclose(xyz[0, 3, 7], [0.0, 0.2, 20.0])


def test_reference_exclusions():
    Q = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 10], [0, 0, 1, -2]], np.float32)   # W' = d - 2
    d = np.array([[[np.nan, np.inf, -np.inf, -1.0, 2.0, 1.0, 3.0, 12.0, 7.0, 4.5]]], np.float32)
    # W' > 0 needs d > 2; Z = 10 / (d - 2): d = 3 -> 10, d = 12 -> 1, d = 7 -> 2, d = 4.5 -> 4
    pts, _, idx, off, _ = ref.reproject_ref(d, Q, depth_range=(1.0, 4.0))
    assert idx.tolist() == [7, 8, 9]                              # 10 > 4 excluded; edges 1 and 4 kept
    assert pts[:, 2].tolist() == [1.0, 2.0, 4.0]
    conf = np.array([[[1, 1, 1, 1, 1, 1, 1, np.nan, 0.5, 0.49]]], np.float32)
    _, _, idx, _, _ = ref.reproject_ref(d, Q, confidence=conf, min_confidence=0.5, depth_range=(0.0, np.inf))
    assert idx.tolist() == [6, 8]
    _, _, idx, _, _ = ref.reproject_ref(d, Q, invalid_disparity=3.0)
    assert 6 not in idx.tolist()


def test_colour_conversion():
    v = np.array([np.nan, -np.inf, -3.0, 0.49, 0.5, 1.5, 254.49, 254.5, 300.0, np.inf], np.float32)
    assert ref.colour_u8(v).tolist() == [0, 0, 0, 0, 1, 2, 254, 255, 255, 255]


def test_fronto_parallel_plane_round_trip(cd):
    H, W, d0 = 40, 64, np.float32(17.25)
    fx, fy, cx, cy = 700.0, 705.0, 31.3, 19.8
    Q = cd.reprojection_matrix(fx, cx, cy, B, fy=fy)
    pts, _, idx, _, _ = ref.reproject_ref(np.full((1, H, W), d0, np.float32), Q)
    assert np.allclose(pts[:, 2], fx * B / float(d0), rtol=1e-6)
    P = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]], np.float64)
    h = np.c_[pts.astype(np.float64), np.ones(len(pts))] @ P.T
    uv = h[:, :2] / h[:, 2:]
    v, u = np.divmod(idx, W)
    assert np.abs(uv[:, 0] - u).max() < 1e-3 and np.abs(uv[:, 1] - v).max() < 1e-3


def brute_voxel(points, colors, offsets, vs, min_points):
    """Per map: a dict of voxel -> points in input order; sums in the two-level order with np.float32 scalars."""
    out_p, out_c, out_n, out_off, dropped = [], [], [], [0], []
    lim = 2 ** 20
    for m in range(len(offsets) - 1):
        vox, drop = {}, 0
        for j in range(offsets[m], offsets[m + 1]):
            with np.errstate(all="ignore"):
                f = [np.floor(np.float32(points[j, a]) / np.float32(vs)) for a in range(3)]
            if not all(-lim <= x < lim for x in f):
                drop += 1
                continue
            vox.setdefault(tuple(int(x) for x in f), []).append(j)
        for key in sorted(vox):
            js = vox[key]
            if len(js) < min_points:
                drop += len(js)
                continue
            chunks = [js[k:k + 64] for k in range(0, len(js), 64)]
            S = None
            for ch in chunks:
                s = points[ch[0]].astype(np.float32).copy()
                for j in ch[1:]:
                    s = (s + points[j]).astype(np.float32)
                S = s if S is None else (S + s).astype(np.float32)
            out_p.append(S / np.float32(len(js)))
            if colors is not None:
                tot = colors[js].astype(np.int64).sum(0)
                out_c.append((tot + len(js) // 2) // len(js))
            out_n.append(len(js))
        out_off.append(len(out_n))
        dropped.append(drop)
    return (np.array(out_p, np.float32).reshape(-1, 3), None if colors is None else np.array(out_c, np.uint8).reshape(-1, 3),
            np.array(out_n, np.int32), out_off, dropped)


@pytest.mark.parametrize("vs,mp", [(0.5, 1), (0.5, 2), (3.0, 1), (100.0, 1), (0.01, 1)])
def test_voxel_reference_equals_brute_force(vs, mp):
    rng = np.random.default_rng(int(vs * 100) + mp)
    pts = rng.normal(0.0, 2.0, (700, 3)).astype(np.float32)      # negative coordinates
    pts[:150] = np.float32(0.1)                                   # one voxel of 150 points: three chunks
    pts[200] = np.float32((2 ** 20 - 1) * 0.5)
    pts[201] = np.float32(2 ** 19)
    pts[202] = np.float32(-(2 ** 20) * 0.5)
    pts[203, 0] = np.nan
    cols = rng.integers(0, 256, (700, 3)).astype(np.uint8)
    off = [0, 1, 1, 300, 700]                                     # one point, empty, two maps
    got = ref.voxel_ref(pts, cols, off, vs, mp)
    exp = brute_voxel(pts, cols, off, vs, mp)
    assert got[3].tolist() == exp[3] and got[4].tolist() == exp[4]
    assert np.array_equal(got[0].view(np.uint32), exp[0].view(np.uint32))
    assert np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])
    assert int(got[2].sum()) + int(got[4].sum()) == 700
    if vs == 0.5:
        assert got[4][2] >= 1                                     # pts[201]: index 2^20 is dropped


def test_voxel_single_point_and_single_voxel():
    p = np.array([[-0.0, 1.25, -7.5]], np.float32)
    got = ref.voxel_ref(p, None, [0, 1], 0.1)
    assert np.array_equal(got[0].view(np.uint32), p.view(np.uint32))   # one point returns itself, -0 included
    pts = np.random.default_rng(0).uniform(0.0, 0.99, (300, 3)).astype(np.float32)
    got = ref.voxel_ref(pts, None, [0, 300], 1.0)
    assert got[2].tolist() == [300] and got[3].tolist() == [0, 1]


def test_clamp_offsets():
    """The device's reading of the caller's offsets: non-decreasing, in [0, capacity]; valid offsets are kept as they
    are."""
    assert ref.clamp_offsets([0, 3, 3, 10], 10).tolist() == [0, 3, 3, 10]
    assert ref.clamp_offsets([-5, 4, 2, 7, 6, 30], 20).tolist() == [0, 4, 4, 7, 7, 20]
    assert ref.clamp_offsets([25, 30, 1], 20).tolist() == [20, 20, 20]             # all past the capacity: n empty maps
    assert ref.clamp_offsets([5, 2 ** 31 - 1], 9).tolist() == [5, 9]
    rng = np.random.default_rng(1)
    for _ in range(50):
        off = rng.integers(-100, 1200, rng.integers(2, 12))
        c = ref.clamp_offsets(off, 1000)
        assert c[0] == min(max(off[0], 0), 1000) and np.all(np.diff(c) >= 0) and 0 <= c.min() and c.max() <= 1000
        # brute force: the smallest non-decreasing sequence in [0, cap] at or above the input, cut at the capacity
        exp = np.minimum(np.maximum.accumulate(np.maximum(off, 0)), 1000)
        assert np.array_equal(c, exp)


def test_ply_round_trip(tmp_path):
    from helpers.ply import read_ply, write_ply
    rng = np.random.default_rng(2)
    pts = rng.normal(size=(17, 3)).astype(np.float32)
    cols = rng.integers(0, 256, (17, 3)).astype(np.uint8)
    path = str(tmp_path / "c.ply")
    write_ply(path, pts, cols)
    data = open(path, "rb").read()
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 17\nproperty float x\nproperty float y\n"
              b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert data.startswith(header) and len(data) == len(header) + 17 * 15
    p2, c2 = read_ply(path)
    assert np.array_equal(p2, pts) and np.array_equal(c2, cols)
    write_ply(path, pts)
    data = open(path, "rb").read()
    assert b"uchar" not in data[:200] and len(data) == data.index(b"end_header\n") + 11 + 17 * 12
    p3, c3 = read_ply(path)
    assert np.array_equal(p3, pts) and c3 is None


def test_kitti_q_from_calibration_file(tmp_path, cd):
    from helpers import kitti_calibration as kc
    p2 = [721.5377, 0, 609.5593, 44.85728, 0, 721.5377, 172.854, 0.2163791, 0, 0, 1, 0.002745884]
    p3 = [721.5377, 0, 609.5593, -339.5242, 0, 721.5377, 172.854, 2.199936, 0, 0, 1, 0.002729905]
    with open(tmp_path / "calib_cam_to_cam.txt", "w") as f:
        f.write("calib_time: 09-Jan-2012 13:57:47\n")
        f.write("P_rect_02: " + " ".join(f"{v:e}" for v in p2) + "\n")
        f.write("P_rect_03: " + " ".join(f"{v:e}" for v in p3) + "\n")
    q = kc.reprojection_matrix(str(tmp_path))
    b = -339.5242 / -721.5377 - 44.85728 / -721.5377
    assert np.array_equal(q, cd.reprojection_matrix(721.5377, 609.5593, 172.854, b, fy=721.5377, cx_right=609.5593))
    assert abs(b - 0.5327) < 1e-3
    fl, bl = kc.focal_length_and_baseline(str(tmp_path))
    assert abs(bl - b) < 1e-12


def test_middlebury_q_from_calibration_fields(cd):
    from pipeline.camera.middlebury_stereo_camera import MiddleBuryStereoCameraCalibration
    cal = MiddleBuryStereoCameraCalibration(cam0=np.array([[3997.684, 0, 1176.728], [0, 3997.684, 1011.728], [0, 0, 1]]),
                                            cam1=np.array([[3997.684, 0, 1307.839], [0, 3997.684, 1011.728], [0, 0, 1]]),
                                            doffs=131.111, baseline=193.001, width=2964, height=1988, ndisp=280,
                                            vmin=31, vmax=257)
    q = cal.reprojection_matrix()
    assert np.array_equal(q, cd.reprojection_matrix(3997.684, 1176.728, 1011.728, 193.001, fy=3997.684,
                                                    cx_right=1307.839))
    d = np.array([[[100.0]]], np.float32)
    pts, *_ = ref.reproject_ref(d, q)
    assert abs(pts[0, 2] - 3997.684 * 193.001 / (100.0 + 131.111)) < 1e-2 * 1e-3 * 3338


def test_header_exports_and_native_table():
    import cuda_depth._native as native
    text = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", text), name
        assert name in native.EXPORTS, name
        assert getattr(native.LIB, name) is not None
    out = os.popen(f"nm -D --defined-only {native.LIB_PATH}").read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT " + name + r"\b", out), name


def test_c_abi_rejects_bad_arguments_without_a_device():
    import cuda_depth._native as native
    lib, bad = native.LIB, native.SMX_OK - 1                       # SMX_ERR_INVALID_ARG = -1
    q = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1).tolist())
    fake = C.c_void_p(0x1000)
    ws = C.c_void_p(0x100000000)
    wsb = lib.smx_reproject_workspace_bytes(1, 4, 8)
    assert wsb > 0 and lib.smx_reproject_workspace_bytes(0, 4, 8) == 0 and lib.smx_reproject_workspace_bytes(1, 40000, 8) == 0

    def rp(**kw):
        a = dict(dev=0, n=1, H=4, W=8, disp=fake, Q=q, conf=None, minc=0.0, z0=0.0, z1=math.inf, inv=-1.0, img=None,
                 ch=0, dt=0, pts=C.c_void_p(0x2000000), col=None, idx=None, xyz=None, off=C.c_void_p(0x3000000), ws=ws,
                 wsb=wsb, stream=None)
        a.update(kw)
        return lib.smx_reproject_points(*a.values())

    assert rp(disp=None) == bad
    assert rp(Q=None) == bad
    assert rp(n=0) == bad
    assert rp(W=40000) == bad
    assert rp(z0=2.0, z1=1.0) == bad
    assert rp(z0=math.nan) == bad
    assert rp(minc=math.nan) == bad
    assert rp(inv=math.nan) == bad
    assert rp(col=C.c_void_p(0x4000000)) == bad                   # colours without an image
    assert rp(img=C.c_void_p(0x5000000), ch=2) == bad
    assert rp(img=C.c_void_p(0x5000000), ch=3, dt=7) == bad
    assert rp(wsb=wsb - 1) == bad
    assert rp(pts=fake) == bad                                    # points overlap disp
    assert rp(stream=native.STREAM_ENGINE) == bad
    assert rp(ws=C.c_void_p(0x100000000 + 8)) == bad and "workspace must be 256-byte aligned" in native.last_error()
    q2 = (C.c_float * 16)(*([math.inf] + [0.0] * 15))
    assert rp(Q=q2) == bad
    assert "Q[0]" in native.last_error()

    vwb = lib.smx_voxel_workspace_bytes(2, 100)
    assert vwb > 0 and lib.smx_voxel_workspace_bytes(0, 100) == 0 and lib.smx_voxel_workspace_bytes(1, 0) == 0

    def vd(**kw):
        a = dict(dev=0, n=2, cap=100, pts=fake, col=None, off=C.c_void_p(0x6000000), vs=0.1, mp=1,
                 op=C.c_void_p(0x2000000), oc=None, cnt=C.c_void_p(0x3000000), oo=C.c_void_p(0x4000000),
                 dr=C.c_void_p(0x5000000), ws=ws, wsb=vwb, stream=None)
        a.update(kw)
        return lib.smx_voxel_downsample(*a.values())

    assert vd(pts=None) == bad
    assert vd(col=fake) == bad                                    # colours without out_colors
    assert vd(n=0) == bad
    assert vd(cap=0) == bad
    assert vd(vs=0.0) == bad
    assert vd(vs=math.inf) == bad
    assert vd(mp=0) == bad
    assert vd(wsb=vwb - 1) == bad
    assert vd(op=fake) == bad                                     # output overlaps points
    assert vd(stream=native.STREAM_ENGINE) == bad
    assert vd(ws=C.c_void_p(0x100000000 + 128)) == bad and "workspace must be 256-byte aligned" in native.last_error()


def test_python_validation_before_the_device(cd):
    import torch
    t = torch.zeros((4, 8))
    with pytest.raises(RuntimeError, match="Q must be a numeric 4x4"):
        cd.reproject_to_3d_batched(t[None], np.eye(3))
    with pytest.raises(RuntimeError, match="Q must be finite"):
        cd.reproject_to_3d_batched(t[None], np.full((4, 4), np.inf))
    with pytest.raises(RuntimeError, match="depth_range"):
        cd.reproject_to_3d_batched(t[None], np.eye(4), depth_range=(2.0, 1.0))
    with pytest.raises(TypeError, match="depth_range"):
        cd.reproject_to_3d_batched(t[None], np.eye(4), depth_range=3.0)
    with pytest.raises(RuntimeError, match="invalid_disparity"):
        cd.reproject_to_3d_batched(t[None], np.eye(4), invalid_disparity=math.nan)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        cd.reproject_to_3d_batched(t[None], np.eye(4))
    with pytest.raises(RuntimeError, match="disp must be"):
        cd.reproject_to_3d(t[None, None], np.eye(4))
    with pytest.raises(RuntimeError, match="voxel_size"):
        cd.voxel_downsample(cd.PointCloud(points=torch.zeros((1, 3))), 0.0)
    with pytest.raises(RuntimeError, match="min_points"):
        cd.voxel_downsample(cd.PointCloud(points=torch.zeros((1, 3))), 0.1, min_points=0)
    with pytest.raises(TypeError, match="min_points"):
        cd.voxel_downsample(cd.PointCloud(points=torch.zeros((1, 3))), 0.1, min_points=1.5)
    with pytest.raises(TypeError, match="PointCloud"):
        cd.voxel_downsample([], 0.1)
    c = cd.PointCloud(points=torch.zeros((2, 3)))
    assert c.colors is None and c.indices is None and c.counts is None and c.xyz_map is None


def test_pipeline_keyword_defaults():
    from pipeline import DepthEstimationPipeline
    from pipeline.depth_estimation_pipeline import DepthEstimationResult
    sig = inspect.signature(DepthEstimationPipeline.__init__).parameters
    assert sig["reprojection_matrix"].default is None
    assert sig["point_cloud_depth_range"].default == (0.0, math.inf)
    assert sig["point_cloud_voxel_size"].default == 0.0
    assert sig["point_cloud_min_points"].default == 1
    assert sig["point_cloud_min_confidence"].default == 0.0
    import torch
    r = DepthEstimationResult(left_image=torch.zeros(1), right_image=torch.zeros(1), disparity_map=torch.zeros(1))
    assert r.point_cloud is None
    with pytest.raises(RuntimeError, match="Q must be"):
        DepthEstimationPipeline(reprojection_matrix=np.eye(3))
    with pytest.raises(RuntimeError, match="voxel_size"):
        DepthEstimationPipeline(reprojection_matrix=np.eye(4), point_cloud_voxel_size=-1.0)
