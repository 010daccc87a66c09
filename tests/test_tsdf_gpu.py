"""TSDF fusion on the device (include/stereo_mi355x.h: smx_tsdf_integrate, smx_tsdf_extract_points), bit for bit
against the NumPy reference (tests/tsdf_ref.py): batches of 1, 3 and 8 maps on odd volumes, every colour source,
confidence weights, KITTI- and Middlebury-style Q, poses inside, outside and behind the volume; one call of n against n
calls, untouched sentinels, ordered extraction with and without enough capacity, graph replay and the pipeline's
volume for the cuda backend."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stereo_synthetic as syn                      # noqa: E402
import tsdf_ref as ref                              # noqa: E402

DIMS = (37, 29, 41)
VS = 0.05
ORIGIN = (-0.9, -0.6, 0.4)
TAU = 3 * VS


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def bits(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bitwise(got, expect, what):
    g, e = bits(got), bits(expect)
    assert g.shape == e.shape, f"{what}: shape {g.shape} != {e.shape}"
    bad = np.argwhere(g != e)
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first at {tuple(bad[0])}"


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def q_kitti(cd, H, W):
    return cd.reprojection_matrix(60.0, (W - 1) / 2.0 + 0.25, (H - 1) / 2.0 - 0.5, 0.2)


def q_middlebury(cd, H, W):
    return cd.reprojection_matrix(60.0, (W - 1) / 2.0, (H - 1) / 2.0, 0.2, fy=61.0, cx_right=(W - 1) / 2.0 + 4.5)


def poses(kind, n, rng):
    """Camera-to-world poses around the volume [-0.9, 0.95] x [-0.6, 0.85] x [0.4, 2.45]."""
    out = []
    for f in range(n):
        jit = rng.uniform(-0.15, 0.15, 3)
        if kind == "outside":
            eye = np.array([0.0, 0.0, -0.5]) + jit
        elif kind == "inside":
            eye = np.array([0.0, 0.1, 1.0]) + jit
        else:                                                       # behind: looking away from the volume
            eye = np.array([0.0, 0.0, -0.3]) + jit
            out.append(ref.look_at(eye, eye + np.array([0.1, 0.0, -1.0])))
            continue
        out.append(ref.look_at(eye, np.array([0.0, 0.1, 1.6]) + rng.uniform(-0.2, 0.2, 3)))
    return np.stack(out)


def maps(rng, n, H, W, zmean=1.5):
    """Disparities of a bumpy surface near depth zmean for Q's f*B = 12, with invalid, NaN and outlier pixels."""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.empty((n, H, W), np.float32)
    for f in range(n):
        z = zmean + 0.3 * np.sin(u / 9.0 + f) * np.cos(v / 7.0) + rng.normal(0, 0.01, (H, W))
        d[f] = (12.0 / z).astype(np.float32)
    r = rng.random((n, H, W))
    d[r < 0.05] = -1.0
    d[(r >= 0.05) & (r < 0.06)] = np.nan
    d[(r >= 0.06) & (r < 0.07)] = rng.uniform(1.0, 40.0, int(((r >= 0.06) & (r < 0.07)).sum()))
    return d


def image(rng, n, H, W, kind):
    if kind is None:
        return None
    ch, dt = kind
    shape = (n, H, W) if ch == 1 else (n, 3, H, W)
    if dt == "u8":
        return rng.integers(0, 256, shape).astype(np.uint8)
    v = rng.uniform(-20.0, 275.0, shape).astype(np.float32)
    v.reshape(-1)[::17] = np.nan
    return v


def run_both(cd, vol, state, d, Q, c2w, img=None, conf=None, **kw):
    vol.integrate(dev(d), Q, c2w, image=dev(img), confidence=dev(conf), **kw)
    ref.integrate_ref(state, vol.dims, vol.origin, vol.voxel_size, vol.truncation, vol.max_weight, d, Q,
                      ref.projection(Q), ref.world_to_camera(c2w), image=img, confidence=conf, **kw)
    torch.cuda.synchronize()


def assert_volume(vol, state, what):
    assert_bitwise(vol.tsdf, state["tsdf"], f"{what}: tsdf")
    assert_bitwise(vol.weight, state["weight"], f"{what}: weight")
    if state["color"] is not None:
        assert np.array_equal(vol.color.cpu().numpy(), state["color"]), f"{what}: color"


COLOURS = [None, (1, "u8"), (3, "f32")]


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("colour", COLOURS)
@pytest.mark.parametrize("qkind", ["kitti", "middlebury"])
def test_integration_matches_reference(cd, n, colour, qkind):
    rng = np.random.default_rng(n * 100 + (0 if colour is None else colour[0]) * 7 + len(qkind))
    H, W = 33, 45
    Q = q_kitti(cd, H, W) if qkind == "kitti" else q_middlebury(cd, H, W)
    vol = cd.TSDFVolume(DIMS, VS, ORIGIN, color=colour is not None, max_weight=5.0)
    state = ref.empty_state(DIMS, colour is not None)
    for kind in ("outside", "inside", "behind"):
        d = maps(rng, n, H, W)
        run_both(cd, vol, state, d, Q, poses(kind, n, rng), image(rng, n, H, W, colour), depth_range=(0.3, 4.0))
        assert_volume(vol, state, f"{kind} n={n}")
    assert (state["weight"] > 0).mean() > 0.02, "the test volume is barely measured"


@pytest.mark.parametrize("min_conf", [0.0, 0.3])
def test_integration_with_confidence(cd, min_conf):
    rng = np.random.default_rng(5)
    n, H, W = 3, 31, 47
    Q = q_kitti(cd, H, W)
    vol = cd.TSDFVolume(DIMS, VS, ORIGIN, color=True)
    state = ref.empty_state(DIMS)
    for _ in range(2):
        d = maps(rng, n, H, W)
        conf = rng.random((n, H, W)).astype(np.float32)
        conf.reshape(-1)[::13] = np.nan
        conf.reshape(-1)[::11] = 0.0
        img = image(rng, n, H, W, (3, "u8"))
        run_both(cd, vol, state, d, Q, poses("outside", n, rng), img, conf, min_confidence=min_conf,
                 invalid_disparity=-1.0)
        assert_volume(vol, state, f"confidence {min_conf}")


def test_one_call_equals_n_calls_and_sentinels(cd):
    rng = np.random.default_rng(8)
    n, H, W = 6, 29, 41
    Q = q_middlebury(cd, H, W)
    d = maps(rng, n, H, W)
    img = image(rng, n, H, W, (1, "u8"))
    c2w = poses("outside", n, rng)
    nx, ny, nz = DIMS
    t0 = np.full((nz, ny, nx), -0.75, np.float32)
    t0.view(np.uint32)[:, :, ::2] = 0x3f7ff123                      # sentinel bit patterns
    t0.view(np.uint32)[:, 1::3, 1::2] = 0xbe5eb00f
    c0 = np.tile(np.array([1, 2, 3, 77], np.uint8), (nz, ny, nx, 1))
    state = {"tsdf": t0, "weight": np.full((nz, ny, nx), 0.5, np.float32), "color": c0}
    before = {k: v.copy() for k, v in state.items()}
    a = cd.TSDFVolume(DIMS, VS, ORIGIN, max_weight=3.0)
    b = cd.TSDFVolume(DIMS, VS, ORIGIN, max_weight=3.0)
    for v in (a, b):
        v.tsdf.copy_(dev(t0))
        v.weight.copy_(dev(state["weight"]))
        v.color.copy_(dev(c0))
    a.integrate(dev(d), Q, c2w, image=dev(img))
    for f in range(n):
        b.integrate(dev(d[f]), Q, c2w[f], image=dev(img[f]))
    seen = ref.integrate_ref(state, DIMS, ORIGIN, VS, a.truncation, 3.0, d, Q, ref.projection(Q),
                             ref.world_to_camera(c2w), image=img)
    torch.cuda.synchronize()
    assert_volume(a, state, "one call")
    assert_volume(b, state, "n calls")
    un = ~seen.reshape(DIMS[::-1])
    assert un.any() and seen.any()
    assert np.array_equal(bits(a.tsdf)[un], bits(before["tsdf"])[un]), "unmeasured tsdf changed"
    assert np.array_equal(bits(a.weight)[un], bits(before["weight"])[un]), "unmeasured weight changed"
    assert np.array_equal(a.color.cpu().numpy()[un], before["color"][un]), "unmeasured colour changed"


def filled_volume(cd, rng, colour=True):
    H, W = 40, 56
    Q = q_kitti(cd, H, W)
    vol = cd.TSDFVolume(DIMS, VS, ORIGIN, color=colour)
    state = ref.empty_state(DIMS, colour)
    for _ in range(2):
        run_both(cd, vol, state, maps(rng, 4, H, W), Q, poses("outside", 4, rng),
                 image(rng, 4, H, W, (3, "u8")) if colour else None)
    return vol, state


@pytest.mark.parametrize("min_weight", [1.0, 2.5])
def test_extraction_matches_reference(cd, min_weight):
    rng = np.random.default_rng(11)
    vol, state = filled_volume(cd, rng)
    assert_volume(vol, state, "fill")
    ep, en, ec = ref.extract_ref(state, DIMS, ORIGIN, VS, min_weight)
    assert len(ep) > 100
    cloud = vol.extract_point_cloud(min_weight=min_weight)
    assert_bitwise(cloud.points, ep, "points")
    assert_bitwise(cloud.normals, en, "normals")
    assert np.array_equal(cloud.colors.cpu().numpy(), ec)
    # a capacity below the total: the count is the total, the prefix is written, nothing past it
    import cuda_depth._native as native
    cap = len(ep) // 3
    pts = torch.full((cap + 5, 3), 7.0, device="cuda")
    nrm = torch.full((cap + 5, 3), 7.0, device="cuda")
    col = torch.full((cap + 5, 3), 7, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    nx, ny, nz = DIMS
    ws_bytes = native.LIB.smx_tsdf_extract_workspace_bytes(nx, ny, nz)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    rc = native.LIB.smx_tsdf_extract_points(0, nx, ny, nz, (C.c_float * 3)(*ORIGIN), VS, vol.tsdf.data_ptr(),
                                            vol.weight.data_ptr(), vol.color.data_ptr(), min_weight, cap,
                                            pts.data_ptr(), nrm.data_ptr(), col.data_ptr(), count.data_ptr(),
                                            ws.data_ptr(), ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, native.last_error()
    torch.cuda.synchronize()
    assert int(count.item()) == len(ep)
    assert_bitwise(pts[:cap], ep[:cap], "prefix points")
    assert_bitwise(nrm[:cap], en[:cap], "prefix normals")
    assert np.array_equal(col[:cap].cpu().numpy(), ec[:cap])
    assert bool((pts[cap:] == 7.0).all() and (nrm[cap:] == 7.0).all() and (col[cap:] == 7).all()), "written past cap"
    plain = vol.extract_point_cloud(min_weight=min_weight, normals=False)
    assert plain.normals is None
    assert_bitwise(plain.points, ep, "points without normals")


def test_extraction_retry_and_no_colour(cd):
    rng = np.random.default_rng(12)
    vol, state = filled_volume(cd, rng, colour=False)
    ep, en, _ = ref.extract_ref(state, DIMS, ORIGIN, VS, 1.0)
    vol._capacity = 7                                               # too small: one retry with the exact count
    cloud = vol.extract_point_cloud()
    assert cloud.colors is None and vol._capacity == len(ep)
    assert_bitwise(cloud.points, ep, "points")
    assert_bitwise(cloud.normals, en, "normals")
    vol.reset()
    assert int(vol.weight.count_nonzero()) == 0
    assert vol.extract_point_cloud().points.shape == (0, 3)


def test_graph_replay(cd):
    import cuda_depth._native as native
    rng = np.random.default_rng(33)
    n, H, W = 3, 30, 44
    Q = q_kitti(cd, H, W)
    P = ref.projection(Q)
    d = maps(rng, n, H, W)
    img = image(rng, n, H, W, (3, "u8"))
    c2w = poses("outside", n, rng)
    vol = cd.TSDFVolume(DIMS, VS, ORIGIN)
    td, ti, tp = dev(d), dev(img), dev(ref.world_to_camera(c2w))
    ws_bytes = native.LIB.smx_tsdf_integrate_workspace_bytes(n, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    qc = (C.c_float * 16)(*Q.reshape(-1).tolist())
    pc = (C.c_float * 16)(*P.reshape(-1).tolist())
    oc = (C.c_float * 3)(*ORIGIN)
    nx, ny, nz = DIMS
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        rc = native.LIB.smx_tsdf_integrate(0, nx, ny, nz, oc, VS, vol.truncation, vol.max_weight, vol.tsdf.data_ptr(),
                                           vol.weight.data_ptr(), vol.color.data_ptr(), n, H, W, td.data_ptr(), qc, pc,
                                           tp.data_ptr(), None, 0.0, 0.0, math.inf, -1.0, ti.data_ptr(), 3,
                                           native.DTYPE_U8, ws.data_ptr(), ws_bytes, C.c_void_p(s.cuda_stream))
        assert rc == 0, native.last_error()
        pts, nrm, col, count = vol.extract_point_cloud_batched(20000)
    torch.cuda.synchronize()
    vol.reset()
    torch.cuda.synchronize()
    state = ref.empty_state(DIMS)
    for f in range(2):
        d2 = d if f == 0 else maps(rng, n, H, W, zmean=1.3)
        td.copy_(dev(d2))
        graph.replay()
        torch.cuda.synchronize()
        ref.integrate_ref(state, DIMS, ORIGIN, VS, vol.truncation, vol.max_weight, d2, Q, P,
                          ref.world_to_camera(c2w), image=img)
        assert_volume(vol, state, f"replay {f}")
        ep, en, ec = ref.extract_ref(state, DIMS, ORIGIN, VS, 1.0)
        assert int(count.item()) == len(ep)
        assert_bitwise(pts[:len(ep)], ep, f"replay {f}: points")
        assert_bitwise(nrm[:len(ep)], en, f"replay {f}: normals")
        assert np.array_equal(col[:len(ep)].cpu().numpy(), ec)


def test_python_errors(cd):
    vol = cd.TSDFVolume(DIMS, VS, ORIGIN)
    t = torch.zeros((2, 4, 8), device="cuda")
    Q = cd.reprojection_matrix(10.0, 4.0, 2.0, 0.1)
    with pytest.raises(RuntimeError, match="colour volume needs image"):
        vol.integrate(t, Q, np.stack([np.eye(4)] * 2))
    with pytest.raises(RuntimeError, match="need 2 pose"):
        vol.integrate(t, Q, np.eye(4), image=torch.zeros((2, 4, 8), dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="image must be"):
        vol.integrate(t, Q, np.stack([np.eye(4)] * 2), image=torch.zeros((2, 2, 4, 8), device="cuda"))
    with pytest.raises(RuntimeError, match="capacity"):
        vol.extract_point_cloud_batched(0)


@pytest.mark.parametrize("confidence", [False, True])
def test_pipeline_volume(cd, confidence):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, D = 48, 96, 16
    Q = cd.reprojection_matrix(50.0, W / 2.0, H / 2.0, 0.1)
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=0, max_disparity=D - 1,
                                        stereo_matching_backend="cuda", left_right_check=True)
    dims, vs, origin = (40, 24, 48), 0.05, (-1.0, -0.6, 0.2)
    vol = cd.TSDFVolume(dims, vs, origin)
    pipe = DepthEstimationPipeline(cfg, reprojection_matrix=Q, tsdf_volume=vol, confidence=confidence,
                                   point_cloud_depth_range=(0.0, 4.0), point_cloud_min_confidence=0.1)
    state = ref.empty_state(dims)
    rng = np.random.default_rng(4)
    for f in range(3):
        left, right, _ = syn.make_pair(H, W, D, 2, f)
        L, R = syn.gray_to_rgb(left).astype(np.uint8), syn.gray_to_rgb(right).astype(np.uint8)
        pose = ref.look_at(rng.uniform(-0.1, 0.1, 3), np.array([0.0, 0.0, 1.5]))
        res = pipe.process(torch.from_numpy(L), torch.from_numpy(R), camera_pose=pose)
        torch.cuda.synchronize()
        d = res.disparity_map.cpu().numpy()[None]
        conf = None if res.confidence_map is None else res.confidence_map.cpu().numpy()[None]
        assert (conf is not None) == confidence
        ref.integrate_ref(state, dims, origin, vs, vol.truncation, vol.max_weight, d, Q, ref.projection(Q),
                          ref.world_to_camera(pose), image=res.left_image.cpu().numpy()[None], confidence=conf,
                          min_confidence=0.1 if confidence else 0.0, depth_range=(0.0, 4.0),
                          invalid_disparity=cfg.invalid_disparity)
        assert_volume(vol, state, f"frame {f}")
    assert (state["weight"] > 0).any()
    with pytest.raises(ValueError, match="camera_pose"):
        pipe.process(torch.from_numpy(L), torch.from_numpy(R))
