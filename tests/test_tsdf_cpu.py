"""TSDF fusion without a GPU: the NumPy reference (tests/tsdf_ref.py) against a scalar per-voxel loop, the projection's
geometry, surface quality on exact and noisy analytic scenes, the update rules (one call of n against n calls,
untouched voxels, the weight cap, confidence weights, colour); PLY files with normals; the C ABI's declarations, exports
and argument checks; Python and pipeline validation before the device is touched."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import points3d_ref
import tsdf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stereo_mi355x.h")
NEW_SYMBOLS = ("smx_tsdf_integrate", "smx_tsdf_integrate_workspace_bytes", "smx_tsdf_extract_points",
               "smx_tsdf_extract_workspace_bytes")
f32 = np.float32


@pytest.fixture(scope="module")
def cd():
    import cuda_depth
    return cuda_depth


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def scalar_integrate(state, dims, origin, s, tau, wmax, disp, Q, P, w2c, image=None, conf=None, min_conf=0.0,
                     zr=(0.0, np.inf), invalid=-1.0):
    """The header's rule voxel by voxel and frame by frame with np.float32 scalars."""
    nx, ny, nz = dims
    n, H, W = disp.shape
    q, P = np.asarray(Q, np.float32), np.asarray(P, np.float32)
    col = None if image is None else ref.pixel_colours(image, n, H, W)
    with np.errstate(all="ignore"):
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    g = [f32(origin[0]) + (f32(i) + f32(0.5)) * f32(s), f32(origin[1]) + (f32(j) + f32(0.5)) * f32(s),
                         f32(origin[2]) + (f32(k) + f32(0.5)) * f32(s)]
                    for f in range(n):
                        M = w2c[f]
                        c = [((M[r, 0] * g[0] + M[r, 1] * g[1]) + M[r, 2] * g[2]) + M[r, 3] for r in range(3)]
                        if not c[2] > 0:
                            continue
                        p = {r: ((P[r, 0] * c[0] + P[r, 1] * c[1]) + P[r, 2] * c[2]) + P[r, 3] for r in (0, 1, 3)}
                        if not p[3] > 0:
                            continue
                        fu, fv = np.floor(p[0] / p[3] + f32(0.5)), np.floor(p[1] / p[3] + f32(0.5))
                        if not (0 <= fu <= W - 1 and 0 <= fv <= H - 1):
                            continue
                        u, v = int(fu), int(fv)
                        d = disp[f, v, u]
                        if not (np.isfinite(d) and d != f32(invalid)):
                            continue
                        fu32, fv32 = f32(u), f32(v)
                        ww = ((q[3, 0] * fu32 + q[3, 1] * fv32) + q[3, 2] * d) + q[3, 3]
                        if not ww > 0:
                            continue
                        zm = (((q[2, 0] * fu32 + q[2, 1] * fv32) + q[2, 2] * d) + q[2, 3]) / ww
                        if not (np.isfinite(zm) and f32(zr[0]) <= zm <= f32(zr[1])):
                            continue
                        w = f32(1.0)
                        if conf is not None:
                            w = conf[f, v, u]
                            if not (w >= f32(min_conf) and w > 0):
                                continue
                        sdf = zm - c[2]
                        if not sdf >= -f32(tau):
                            continue
                        t = min(sdf / f32(tau), f32(1.0))
                        T0, W0 = state["tsdf"][k, j, i], state["weight"][k, j, i]
                        den = W0 + w
                        state["tsdf"][k, j, i] = ((T0 * W0) + (t * w)) / den
                        state["weight"][k, j, i] = min(den, f32(wmax))
                        if col is not None:
                            C0 = state["color"][k, j, i, :3].astype(np.float32)
                            I = col[f, v, u].astype(np.float32)
                            state["color"][k, j, i, :3] = ref.colour_u8(((C0 * W0) + (I * w)) / den)
                            state["color"][k, j, i, 3] = 0


def small_case(rng, n=3, H=11, W=13):
    Q = np.array([[1, 0, 0, -6.25], [0, 1, 0, -5.5], [0, 0, 0, 20.0], [0, 0, 4.0, 1.5]], np.float32)   # f 20, B 0.25
    d = rng.uniform(2.0, 12.0, (n, H, W)).astype(np.float32)
    d[rng.random((n, H, W)) < 0.1] = -1.0
    d[0, 0, 0] = np.nan
    c2w = np.stack([ref.look_at(rng.uniform(-0.2, 0.2, 3) + [0, 0, -0.5], (0.0, 0.0, 1.5)) for _ in range(n)])
    return Q, d, c2w


@pytest.mark.parametrize("dims,colour,with_conf", [((7, 5, 9), True, False), ((5, 9, 3), False, True),
                                                  ((1, 3, 11), True, True)])
def test_reference_equals_scalar_loop(dims, colour, with_conf):
    rng = np.random.default_rng(sum(dims))
    Q, d, c2w = small_case(rng)
    n, H, W = d.shape
    origin, s = (-0.35, -0.3, 0.6), 0.1
    img = rng.uniform(-5, 260, (n, 3, H, W)).astype(np.float32) if colour else None
    conf = rng.random((n, H, W)).astype(np.float32) if with_conf else None
    a, b = ref.empty_state(dims, colour), ref.empty_state(dims, colour)
    P, w2c = ref.projection(Q), ref.world_to_camera(c2w)
    for _ in range(2):
        ref.integrate_ref(a, dims, origin, s, 0.25, 2.5, d, Q, P, w2c, image=img, confidence=conf, min_confidence=0.2,
                          depth_range=(0.5, 3.0))
        scalar_integrate(b, dims, origin, s, 0.25, 2.5, d, Q, P, w2c, img, conf, 0.2, (0.5, 3.0))
    assert (a["weight"] > 0).sum() > 5
    assert np.array_equal(bits(a["tsdf"]), bits(b["tsdf"])) and np.array_equal(bits(a["weight"]), bits(b["weight"]))
    if colour:
        assert np.array_equal(a["color"], b["color"])


def test_projection_inverts_reprojection(cd):
    for Q in (cd.reprojection_matrix(721.5, 609.5, 172.8, 0.54),
              cd.reprojection_matrix(3997.7, 1176.7, 1011.7, 193.0, cx_right=1307.8)):
        P = cd.projection_matrix(Q)
        assert P.dtype == np.float32
        assert np.allclose(P.astype(np.float64) @ Q.astype(np.float64), np.eye(4), atol=1e-4)
    with pytest.raises(RuntimeError, match="singular"):
        cd.projection_matrix(np.diag([1.0, 1.0, 0.0, 1.0]))


def test_voxel_on_a_reprojected_point_projects_to_its_pixel(cd):
    H, W = 20, 30
    Q = cd.reprojection_matrix(50.0, 14.5, 9.5, 0.3, cx_right=16.0)
    d = np.full((1, H, W), 7.25, np.float32)
    pts, _, idx, _, _ = points3d_ref.reproject_ref(d, Q)
    P = ref.projection(Q)
    for k in (0, 37, 301, 599):
        v, u = divmod(int(idx[k]), W)
        # a 1x1x1 volume whose only voxel centre is that point, seen by the identity pose
        origin = tuple(float(c) - 0.05 for c in pts[k])
        st = ref.empty_state((1, 1, 1), False)
        seen = ref.integrate_ref(st, (1, 1, 1), origin, 0.1, 0.3, 10.0, d, Q, P, ref.world_to_camera(np.eye(4)))
        assert seen[0]
        g = np.array([f32(origin[a]) + f32(0.5) * f32(0.1) for a in range(3)], np.float32)
        h = P.astype(np.float64) @ np.r_[g.astype(np.float64), 1.0]
        assert (round(h[0] / h[3]), round(h[1] / h[3])) == (u, v)
        assert abs(st["tsdf"][0, 0, 0]) < 0.05


SCENE_DIMS, SCENE_VS, SCENE_ORIGIN = (48, 23, 60), 0.1, (-2.4, -0.4, 4.0)
CAM = dict(H=96, W=128, fx=100.0, cx=63.5, cy=47.5, baseline=0.5)


def fuse_scene(cd, poses, noise=0.0, outliers=0.0, seed=0):
    scene = ref.demo_scene()
    Q = cd.reprojection_matrix(CAM["fx"], CAM["cx"], CAM["cy"], CAM["baseline"])
    rng = np.random.default_rng(seed)
    maps = []
    for pose in poses:
        d = scene.render(pose, CAM["H"], CAM["W"], CAM["fx"], CAM["cx"], CAM["cy"], CAM["baseline"])
        ok = d > 0
        d[ok] += rng.normal(0.0, noise, int(ok.sum())).astype(np.float32) if noise else 0
        out = ok & (rng.random(d.shape) < outliers)
        d[out] = rng.uniform(1.0, 20.0, int(out.sum())).astype(np.float32)
        maps.append(d)
    d = np.stack(maps)
    st = ref.empty_state(SCENE_DIMS, False)
    ref.integrate_ref(st, SCENE_DIMS, SCENE_ORIGIN, SCENE_VS, 3 * SCENE_VS, 64.0, d, Q, ref.projection(Q),
                      ref.world_to_camera(poses))
    return scene, st, d, Q


def test_exact_scene_surface_and_normals(cd):
    poses = ref.orbit_poses(6)
    scene, st, _, _ = fuse_scene(cd, poses)
    pts, nrm, _ = ref.extract_ref(st, SCENE_DIMS, SCENE_ORIGIN, SCENE_VS, 1.0)
    assert len(pts) > 2000
    dist = scene.distance(pts)
    assert np.mean(dist < 0.5 * SCENE_VS) >= 0.95
    want, interior = scene.face_normals(pts, 2 * SCENE_VS)
    assert interior.sum() > 1000
    cosang = np.sum(nrm[interior].astype(np.float64) * want[interior], axis=1)
    # The distance is projective (along the camera's z axis), which tilts the gradient on surfaces seen at a grazing
    # angle, the ground above all: measured on this scene, 89 % of the face-interior normals lie within 10 degrees and
    # 96 % within 20.
    assert np.mean(cosang > math.cos(math.radians(10))) >= 0.85
    assert np.mean(cosang > math.cos(math.radians(20))) >= 0.95


def test_noisy_scene_fusion_beats_single_frames(cd):
    poses = ref.orbit_poses(8)
    scene, st, d, Q = fuse_scene(cd, poses, noise=0.5, outliers=0.05, seed=3)
    pts, _, _ = ref.extract_ref(st, SCENE_DIMS, SCENE_ORIGIN, SCENE_VS, 2.0)
    fused = np.sqrt(np.mean(scene.distance(pts) ** 2))
    single = []
    for f, pose in enumerate(poses):
        p, *_ = points3d_ref.reproject_ref(d[f:f + 1], Q)
        pw = p.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]
        single.append(np.sqrt(np.mean(scene.distance(pw) ** 2)))
    assert fused < 0.5 * np.mean(single), (fused, single)


def test_one_call_equals_n_calls_and_untouched_voxels():
    rng = np.random.default_rng(4)
    Q, d, c2w = small_case(rng, n=4)
    dims, origin = (9, 7, 11), (-0.45, -0.35, 0.55)
    img = rng.integers(0, 256, (4, d.shape[1], d.shape[2])).astype(np.uint8)
    a = ref.empty_state(dims)
    a["tsdf"][:] = f32(0.25)
    a["color"][:] = 9
    b = {k: v.copy() for k, v in a.items()}
    P, w2c = ref.projection(Q), ref.world_to_camera(c2w)
    seen = ref.integrate_ref(a, dims, origin, 0.1, 0.25, 3.0, d, Q, P, w2c, image=img)
    for f in range(4):
        ref.integrate_ref(b, dims, origin, 0.1, 0.25, 3.0, d[f:f + 1], Q, P, w2c[f:f + 1], image=img[f:f + 1])
    for key in ("tsdf", "weight", "color"):
        assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key
    un = ~seen.reshape(dims[::-1])
    assert un.any() and seen.any()
    assert np.all(a["tsdf"][un] == f32(0.25)) and np.all(a["weight"][un] == 0) and np.all(a["color"][un] == 9)
    assert np.all(a["color"][~un][:, 3] == 0)


def test_weight_cap_confidence_and_colour_rules():
    # one voxel in front of a fronto-parallel wall: every frame measures it through the same pixel
    Q = np.array([[1, 0, 0, -2.0], [0, 1, 0, -2.0], [0, 0, 0, 10.0], [0, 0, 1.0, 0.0]], np.float32)   # Z = 10 / d
    d = np.full((5, 5, 5), 5.0, np.float32)                                                          # Z = 2
    dims, origin = (1, 1, 1), (-0.05, -0.05, 1.85)                                                   # centre z = 1.9
    P, w2c = ref.projection(Q), ref.world_to_camera(np.stack([np.eye(4)] * 5))
    st = ref.empty_state(dims, False)
    ref.integrate_ref(st, dims, origin, 0.1, 0.25, 2.5, d, Q, P, w2c)
    t = f32(f32(2.0) - f32(1.9000001)) / f32(0.25)
    assert st["weight"][0, 0, 0] == f32(2.5)                                                          # capped
    assert abs(st["tsdf"][0, 0, 0] - t) < 1e-6
    # confidence: c < min_confidence or c <= 0 is skipped, c is the weight
    conf = np.full((5, 5, 5), 0.5, np.float32)
    conf[1], conf[2], conf[3] = 0.1, 0.0, np.nan
    st = ref.empty_state(dims, False)
    ref.integrate_ref(st, dims, origin, 0.1, 0.25, 64.0, d, Q, P, w2c, confidence=conf, min_confidence=0.0)
    assert st["weight"][0, 0, 0] == f32(0.5) + f32(0.1) + f32(0.5) + f32(0.5) - 0 or \
        st["weight"][0, 0, 0] == ((f32(0.5) + f32(0.1)) + f32(0.5))
    st = ref.empty_state(dims, False)
    ref.integrate_ref(st, dims, origin, 0.1, 0.25, 64.0, d, Q, P, w2c, confidence=conf, min_confidence=0.2)
    assert st["weight"][0, 0, 0] == f32(1.0)
    # colour: gray copied to R, G, B; f32 rounded half up and clamped; running weighted mean, stored rounded
    for img, first in ((np.full((5, 5, 5), 200, np.uint8), [200, 200, 200]),
                       (np.full((5, 3, 5, 5), 254.5, np.float32), [255, 255, 255]),
                       (np.full((5, 3, 5, 5), -3.0, np.float32), [0, 0, 0])):
        st = ref.empty_state(dims, True)
        ref.integrate_ref(st, dims, origin, 0.1, 0.25, 64.0, d[:1], Q, P, w2c[:1], image=img[:1])
        assert st["color"][0, 0, 0].tolist() == first + [0]
    img = np.zeros((2, 3, 5, 5), np.uint8)
    img[0] = 100
    img[1] = 101
    st = ref.empty_state(dims, True)
    ref.integrate_ref(st, dims, origin, 0.1, 0.25, 64.0, d[:2], Q, P, w2c[:2], image=img)
    assert st["color"][0, 0, 0].tolist() == [101, 101, 101, 0]                                       # 100.5 -> 101


def test_extraction_rules():
    # a field that crosses zero along x in the middle, with a truncated jump and an unweighted voxel
    st = ref.empty_state((4, 2, 1), True)
    st["tsdf"][0, 0] = [0.6, 0.2, -0.6, -1.0]
    st["tsdf"][0, 1] = [1.0, -0.5, 0.4, 0.3]
    st["weight"][:] = 1.0
    st["weight"][0, 1, 3] = 0.5
    st["color"][0, 0, 1, :3] = [10, 20, 30]
    st["color"][0, 0, 2, :3] = [40, 50, 60]
    pts, nrm, col = ref.extract_ref(st, (4, 2, 1), (0.0, 0.0, 0.0), 1.0)
    # (0,0): x 0.2 -> -0.6 crossing; (1,0) y: 0.2 -> -0.5 none (same... no: 0.2 >= 0, -0.5 < 0) crossing;
    # (2,0) y: -0.6 -> 0.4 crossing; (1,1) x: -0.5 -> 0.4 crossing; (0,1)/(1,0): |1.0| rejects; (3,*) w or |T|
    assert len(pts) == 4
    assert np.allclose(pts[0], [1.5 + 0.25, 0.5, 0.5])
    assert col[0].tolist() == [10, 20, 30]                                                           # t = 0.25
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-6)


def test_ply_round_trip_with_normals(tmp_path):
    from helpers.ply import read_ply, write_ply
    rng = np.random.default_rng(2)
    pts = rng.normal(size=(11, 3)).astype(np.float32)
    nrm = rng.normal(size=(11, 3)).astype(np.float32)
    cols = rng.integers(0, 256, (11, 3)).astype(np.uint8)
    path = str(tmp_path / "n.ply")
    write_ply(path, pts, cols, normals=nrm)
    data = open(path, "rb").read()
    assert b"property float nx\nproperty float ny\nproperty float nz\nproperty uchar red" in data
    assert len(data) == data.index(b"end_header\n") + 11 + 11 * 27
    p2, c2, n2 = read_ply(path, with_normals=True)
    assert np.array_equal(p2, pts) and np.array_equal(c2, cols) and np.array_equal(n2, nrm)
    p3, c3 = read_ply(path)
    assert np.array_equal(p3, pts) and np.array_equal(c3, cols)
    write_ply(path, pts, normals=nrm)
    p4, c4, n4 = read_ply(path, with_normals=True)
    assert c4 is None and np.array_equal(n4, nrm)
    write_ply(path, pts)
    assert read_ply(path, with_normals=True)[2] is None
    with pytest.raises(ValueError, match="normals"):
        write_ply(path, pts, normals=nrm[:3])


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
    assert "smx_tsdf_integrate" in text.split("Conventions")[0]


def test_c_abi_rejects_bad_arguments_without_a_device():
    import cuda_depth._native as native
    lib, bad = native.LIB, native.SMX_OK - 1                       # SMX_ERR_INVALID_ARG = -1
    eye = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1).tolist())
    org = (C.c_float * 3)(0.0, 0.0, 0.0)
    fake = C.c_void_p(0x1000)
    ws = C.c_void_p(0x100000000)
    wsb = lib.smx_tsdf_integrate_workspace_bytes(2, 4, 8)
    assert wsb >= 2 * 4 * 8 * 12 and lib.smx_tsdf_integrate_workspace_bytes(0, 4, 8) == 0
    assert lib.smx_tsdf_integrate_workspace_bytes(1, 40000, 8) == 0

    def ti(**kw):
        a = dict(dev=0, nx=8, ny=8, nz=8, origin=org, s=0.1, tau=0.3, wmax=64.0, tsdf=C.c_void_p(0x2000000),
                 weight=C.c_void_p(0x3000000), color=None, n=2, H=4, W=8, disp=fake, Q=eye, P=eye,
                 pose=C.c_void_p(0x4000000), conf=None, minc=0.0, z0=0.0, z1=math.inf, inv=-1.0, img=None, ch=0, dt=0,
                 ws=ws, wsb=wsb, stream=None)
        a.update(kw)
        return lib.smx_tsdf_integrate(*a.values())

    inf, nan = math.inf, math.nan
    q_inf = (C.c_float * 16)(*([inf] + [0.0] * 15))
    for kw in (dict(origin=None), dict(tsdf=None), dict(weight=None), dict(disp=None), dict(Q=None), dict(P=None),
               dict(pose=None), dict(ws=None), dict(nx=0), dict(ny=4097), dict(nz=-1), dict(nx=4096, ny=4096, nz=65),
               dict(n=0), dict(H=0), dict(W=40000), dict(n=8192, H=512, W=512), dict(s=0.0), dict(s=inf),
               dict(s=nan), dict(tau=0.1), dict(tau=0.05), dict(tau=inf), dict(wmax=0.0), dict(wmax=inf),
               dict(Q=q_inf), dict(P=q_inf), dict(origin=(C.c_float * 3)(0.0, nan, 0.0)), dict(z0=nan),
               dict(z0=2.0, z1=1.0), dict(minc=nan), dict(inv=nan), dict(color=C.c_void_p(0x5000000)),
               dict(img=C.c_void_p(0x6000000), ch=2), dict(img=C.c_void_p(0x6000000), ch=3, dt=7), dict(wsb=wsb - 1),
               dict(tsdf=fake), dict(weight=C.c_void_p(0x2000000 + 64)), dict(ws=C.c_void_p(0x3000000 + 16)),
               dict(stream=native.STREAM_ENGINE)):
        assert ti(**kw) == bad, kw
    assert ti(P=q_inf) == bad and "P[0]" in native.last_error()
    assert ti(ws=C.c_void_p(0x100000000 + 8)) == bad and "workspace must be 256-byte aligned" in native.last_error()

    ewb = lib.smx_tsdf_extract_workspace_bytes(8, 8, 8)
    assert ewb >= 2 * 64 * 4 and lib.smx_tsdf_extract_workspace_bytes(0, 8, 8) == 0

    def te(**kw):
        a = dict(dev=0, nx=8, ny=8, nz=8, origin=org, s=0.1, tsdf=C.c_void_p(0x2000000), weight=C.c_void_p(0x3000000),
                 color=None, minw=1.0, cap=100, pts=C.c_void_p(0x4000000), nrm=None, col=None,
                 count=C.c_void_p(0x5000000), ws=ws, wsb=ewb, stream=None)
        a.update(kw)
        return lib.smx_tsdf_extract_points(*a.values())

    for kw in (dict(origin=None), dict(tsdf=None), dict(weight=None), dict(pts=None), dict(count=None), dict(ws=None),
               dict(nx=0), dict(nz=5000), dict(s=-1.0), dict(origin=(C.c_float * 3)(inf, 0.0, 0.0)), dict(minw=0.0),
               dict(minw=nan), dict(minw=inf), dict(cap=0), dict(cap=2 ** 30 + 1), dict(col=C.c_void_p(0x6000000)),
               dict(wsb=ewb - 1), dict(pts=C.c_void_p(0x2000000 + 8)), dict(count=C.c_void_p(0x4000000 + 4)),
               dict(stream=native.STREAM_ENGINE)):
        assert te(**kw) == bad, kw
    assert te(ws=C.c_void_p(0x100000000 + 128)) == bad and "workspace must be 256-byte aligned" in native.last_error()


def test_python_validation_before_the_device(cd):
    import torch
    with pytest.raises(RuntimeError, match="nx must be in"):
        cd.TSDFVolume((0, 4, 4), 0.1, (0, 0, 0))
    with pytest.raises(RuntimeError, match="2\\^30 voxels"):
        cd.TSDFVolume((4096, 4096, 128), 0.1, (0, 0, 0))
    with pytest.raises(TypeError, match="dims"):
        cd.TSDFVolume(4, 0.1, (0, 0, 0))
    with pytest.raises(RuntimeError, match="voxel_size"):
        cd.TSDFVolume((4, 4, 4), 0.0, (0, 0, 0))
    with pytest.raises(RuntimeError, match="origin"):
        cd.TSDFVolume((4, 4, 4), 0.1, (0, math.nan, 0))
    with pytest.raises(RuntimeError, match="truncation"):
        cd.TSDFVolume((4, 4, 4), 0.1, (0, 0, 0), truncation=0.1)
    with pytest.raises(RuntimeError, match="max_weight"):
        cd.TSDFVolume((4, 4, 4), 0.1, (0, 0, 0), max_weight=0.0)
    with pytest.raises(RuntimeError, match="GPU device"):
        cd.TSDFVolume((4, 4, 4), 0.1, (0, 0, 0), device="cpu")
    # integrate's checks run before any tensor is touched: a volume object without state is enough
    vol = object.__new__(cd.TSDFVolume)
    t = torch.zeros((4, 8))
    Q = cd.reprojection_matrix(10.0, 4.0, 2.0, 0.1)
    with pytest.raises(RuntimeError, match="Q is singular"):
        vol.integrate(t, np.diag([1.0, 1.0, 0.0, 1.0]), np.eye(4))
    with pytest.raises(RuntimeError, match="Q must be a numeric 4x4"):
        vol.integrate(t, np.eye(3), np.eye(4))
    with pytest.raises(RuntimeError, match="depth_range"):
        vol.integrate(t, Q, np.eye(4), depth_range=(2.0, 1.0))
    with pytest.raises(RuntimeError, match="camera_to_world must be finite"):
        vol.integrate(t, Q, np.full((4, 4), np.nan))
    bad_row = np.eye(4)
    bad_row[3, 0] = 0.5
    with pytest.raises(RuntimeError, match="last row"):
        vol.integrate(t, Q, bad_row)
    with pytest.raises(RuntimeError, match="singular"):
        vol.integrate(t, Q, np.diag([1.0, 0.0, 1.0, 1.0]))
    with pytest.raises(RuntimeError, match="\\[4, 4\\] or \\[n, 4, 4\\]"):
        vol.integrate(t, Q, np.eye(3))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        vol.integrate(t, Q, torch.eye(4, dtype=torch.float64))
    w2c = cd.world_to_camera_poses(ref.look_at((1.0, 2.0, 3.0), (0.0, 0.0, 10.0)))
    assert w2c.shape == (1, 3, 4) and w2c.dtype == np.float32


def test_pipeline_keyword_errors(cd):
    import inspect
    import torch
    from pipeline import DepthEstimationPipeline
    sig = inspect.signature(DepthEstimationPipeline.__init__).parameters
    assert sig["tsdf_volume"].default is None
    assert inspect.signature(DepthEstimationPipeline.process).parameters["camera_pose"].default is None
    vol = object.__new__(cd.TSDFVolume)
    with pytest.raises(ValueError, match="reprojection_matrix"):
        DepthEstimationPipeline(tsdf_volume=vol)
    with pytest.raises(TypeError, match="TSDFVolume"):
        DepthEstimationPipeline(reprojection_matrix=np.eye(4), tsdf_volume=object())
    pipe = object.__new__(DepthEstimationPipeline)                  # process() checks before touching the device
    pipe._tsdf_volume = None
    with pytest.raises(ValueError, match="camera_pose needs"):
        pipe.process(torch.zeros((3, 4, 4)), torch.zeros((3, 4, 4)), camera_pose=np.eye(4))
    pipe._tsdf_volume = vol                                         # as a pipeline built with a volume
    with pytest.raises(ValueError, match="camera_pose is required"):
        pipe.process(torch.zeros((3, 4, 4)), torch.zeros((3, 4, 4)))
