"""Ray casting of TSDF volumes on the device (include/stereo_mi355x.h: smx_tsdf_raycast), bit for bit against the dense
NumPy twin (tests/raycast_ref.py) for all five outputs, on the cases of tests/raycast_cases.py: the 37 x 29 x 41 volume
(no multiple of the brick), 33 x 45 views (no multiple of the pixel tile), one and three views per call, the sweep of
step, min_weight and Q, poses outside, inside, behind and exactly along an axis, a volume measured in one corner only
(most bricks empty: the jumps must change nothing), optional outputs, a volume without colour, more views than the grid
holds, graph capture of integrate followed by raycast, and the pipeline's render_model."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import raycast_cases as cases                       # noqa: E402
import raycast_ref as rc                            # noqa: E402
import stereo_synthetic as syn                      # noqa: E402
import tsdf_ref as ref                              # noqa: E402

f32 = np.float32
THREE = ("outside", "inside", "behind")


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def upload(cd, state):
    vol = cd.TSDFVolume(cases.DIMS, cases.VS, cases.ORIGIN, color=state["color"] is not None)
    vol.tsdf.copy_(dev(state["tsdf"]))
    vol.weight.copy_(dev(state["weight"]))
    if vol.color is not None:
        vol.color.copy_(dev(state["color"]))
    return vol


def as_dict(view):
    torch.cuda.synchronize()
    return {k: None if getattr(view, k) is None else getattr(view, k).cpu().numpy()
            for k in ("disparity", "depth", "normals", "colors", "weight")}


def step_of(step_voxels) -> float:
    return float(f32(cases.VS) * f32(step_voxels))


@pytest.mark.parametrize("qkind", cases.QKINDS)
@pytest.mark.parametrize("step_voxels", cases.STEPS)
@pytest.mark.parametrize("min_weight", cases.MIN_WEIGHTS)
def test_three_views_match_the_twin(cd, qkind, step_voxels, min_weight):
    vol = upload(cd, cases.fused_state())
    got = as_dict(vol.render(cases.q_of(qkind), cases.poses_of(THREE), cases.SHAPE, min_weight=min_weight,
                             step=step_of(step_voxels), depth_range=cases.DEPTH_RANGE))
    want = cases.expected(THREE, qkind, step_voxels, min_weight)
    assert got["disparity"].shape == (3,) + cases.SHAPE and got["normals"].shape == (3, 3) + cases.SHAPE
    cases.assert_same(got, want, f"{qkind} step {step_voxels} min_weight {min_weight}")
    hits = np.isfinite(want["depth"]).reshape(3, -1).mean(axis=1)
    assert hits[2] == 0 and (min_weight > 1.0 or (hits[0] > 0.5 and hits[1] > 0.3)), hits


@pytest.mark.parametrize("qkind", ["centred", "middlebury"])
def test_one_view_along_an_axis_from_a_voxel_centre(cd, qkind):
    vol = upload(cd, cases.fused_state())
    got = as_dict(vol.render(cases.q_of(qkind), cases.aligned_pose(), cases.SHAPE, depth_range=cases.DEPTH_RANGE))
    want = cases.expected(("aligned",), qkind, 1.0, 1.0)                         # step defaults to voxel_size
    assert got["disparity"].shape == cases.SHAPE and got["colors"].shape == (3,) + cases.SHAPE
    cases.assert_same({k: v[None] for k, v in got.items()}, want, f"aligned {qkind}")
    assert np.isfinite(want["depth"][0, 16, 22])                                 # the ray with dw = (0, 0, 1) hits


@pytest.mark.parametrize("step_voxels", [0.5, 2.5])
def test_empty_bricks_change_nothing(cd, step_voxels):
    state = cases.fused_state(True, True)                                        # measured in one corner only
    assert 0 < cases.occupied_bricks(state, 1.0) < 0.3
    views = ("outside", "inside", "oblique")
    got = as_dict(upload(cd, state).render(cases.q_of("kitti"), cases.poses_of(views), cases.SHAPE,
                                           step=step_of(step_voxels), depth_range=cases.DEPTH_RANGE))
    want = cases.expected(views, "kitti", step_voxels, 1.0, True, True)
    cases.assert_same(got, want, f"corner volume, step {step_voxels}")
    assert np.isfinite(want["depth"]).any()


@pytest.mark.parametrize("step_voxels", cases.STEPS)
def test_measured_free_space_changes_nothing(cd, step_voxels):
    views = ("outside", "inside", "behind", "oblique")                          # a ball in measured free space: free,
    got = as_dict(upload(cd, cases.analytic_state()).render(cases.q_of("kitti"), cases.poses_of(views), cases.SHAPE,
                                                            step=step_of(step_voxels), depth_range=cases.DEPTH_RANGE))
    want = cases.expected_analytic(views, step_voxels)                           # mixed and empty bricks
    cases.assert_same(got, want, f"ball in free space, step {step_voxels}")
    assert np.isfinite(want["depth"][0]).mean() > 0.05


def test_default_range_no_colour_and_an_empty_volume(cd):
    state = cases.fused_state(False)
    vol = upload(cd, state)
    Q, pose = cases.q_of("kitti"), cases.poses_of(("oblique",))
    *_, (z_min, z_max) = vol._check_render_args(Q, pose, cases.SHAPE, 1.0, None, None, True, True, -1.0)
    assert z_min == 0.0 and 2.0 < z_max < 4.0                                    # eye to the farthest corner
    got = as_dict(vol.render(Q, pose, cases.SHAPE))
    want = cases.expected(("oblique",), "kitti", 1.0, 1.0, False, False, (z_min, z_max))
    assert got["colors"] is None and want["colors"] is None
    cases.assert_same(got, want, "defaults, no colour")
    assert np.isfinite(want["depth"]).mean() > 0.1
    vol.reset()
    got = as_dict(vol.render(Q, pose, cases.SHAPE, invalid_disparity=-7.0))
    assert (got["disparity"] == -7.0).all() and np.isnan(got["depth"]).all()
    assert (got["normals"] == 0).all() and (got["weight"] == 0).all()


def raycast_call(native, vol, n, shape, Q, poses, step, depth_range, disp, depth, normals, colors, weight, ws, stream,
                 min_weight=1.0):
    nx, ny, nz = vol.dims
    H, W = shape
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rcode = native.LIB.smx_tsdf_raycast(0, nx, ny, nz, (C.c_float * 3)(*vol.origin), vol.voxel_size, vol.tsdf.data_ptr(),
                                        vol.weight.data_ptr(), ptr(vol.color), min_weight, n, H, W,
                                        (C.c_float * 16)(*Q.reshape(-1).tolist()), poses.data_ptr(), step, depth_range[0],
                                        depth_range[1], -1.0, ptr(disp), ptr(depth), ptr(normals), ptr(colors),
                                        ptr(weight), ws.data_ptr(), ws.numel(), C.c_void_p(stream))
    assert rcode == 0, native.last_error()


def test_optional_outputs_and_sentinels(cd):
    import cuda_depth._native as native
    vol = upload(cd, cases.fused_state())
    H, W = cases.SHAPE
    n, P = 3, 3 * H * W
    want = cases.expected(THREE, "kitti", 1.0, 1.0)
    Q = cases.q_of("kitti")
    poses = dev(rc.view_pose(cases.poses_of(THREE)))
    ws = torch.empty(native.LIB.smx_tsdf_raycast_workspace_bytes(*cases.DIMS), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    PAD = 64
    # every optional output NULL: disp is written, the sentinels around it and in the buffers not handed over stay
    buf = torch.full((PAD + P + PAD,), 7.25, device="cuda")
    others = [torch.full((3 * P,), 7.25, device="cuda"), torch.full((3 * P,), 7, dtype=torch.uint8, device="cuda")]
    raycast_call(native, vol, n, cases.SHAPE, Q, poses, step_of(1.0), cases.DEPTH_RANGE, buf[PAD:PAD + P], None, None, None,
                 None, ws, stream)
    torch.cuda.synchronize()
    cases.assert_same({"disparity": buf[PAD:PAD + P].cpu().numpy().reshape(n, H, W)}, want, "disp alone")
    assert bool((buf[:PAD] == 7.25).all() and (buf[PAD + P:] == 7.25).all()), "written outside disp"
    assert bool((others[0] == 7.25).all() and (others[1] == 7).all())
    # each optional output alone, in padded buffers
    for key, mult, dtype in (("depth", 1, torch.float32), ("normals", 3, torch.float32), ("colors", 3, torch.uint8),
                             ("weight", 1, torch.float32)):
        disp = torch.empty(P, device="cuda")
        out = torch.full((PAD + mult * P + PAD,), 9, dtype=dtype, device="cuda")
        arg = {k: None for k in ("depth", "normals", "colors", "weight")}
        arg[key] = out[PAD:PAD + mult * P]
        raycast_call(native, vol, n, cases.SHAPE, Q, poses, step_of(1.0), cases.DEPTH_RANGE, disp, arg["depth"],
                     arg["normals"], arg["colors"], arg["weight"], ws, stream)
        torch.cuda.synchronize()
        shape = (n, 3, H, W) if mult == 3 else (n, H, W)
        cases.assert_same({"disparity": disp.cpu().numpy().reshape(n, H, W), key: arg[key].cpu().numpy().reshape(shape)}, want,
                          f"disp and {key}")
        assert bool((out[:PAD] == 9).all() and (out[PAD + mult * P:] == 9).all()), f"written outside {key}"
    plain = as_dict(vol.render(Q, cases.poses_of(THREE), cases.SHAPE, depth_range=cases.DEPTH_RANGE, normals=False,
                               colors=False))
    assert plain["normals"] is None and plain["colors"] is None
    cases.assert_same(plain, want, "render without normals and colours")


def test_more_views_than_the_grid_holds(cd):
    vol = upload(cd, cases.fused_state())
    shape, names = (2, 3), ("outside", "inside", "oblique")
    n = 65535 + 3                                                                # the march's grid holds 65535 views
    Q = cases.q_of("centred", shape)
    three = rc.raycast_ref(cases.fused_state(), cases.DIMS, cases.ORIGIN, cases.VS, Q, rc.view_pose(cases.poses_of(names)),
                           shape, depth_range=cases.DEPTH_RANGE)
    assert np.isfinite(three["depth"]).any()
    poses = np.tile(cases.poses_of(names), (n // 3, 1, 1))
    got = as_dict(vol.render(Q, poses, shape, depth_range=cases.DEPTH_RANGE))
    want = {k: np.tile(v, (n // 3,) + (1,) * (v.ndim - 1)) for k, v in three.items()}
    cases.assert_same(got, want, f"{n} views")


def test_graph_capture_of_integrate_then_raycast(cd):
    import cuda_depth._native as native
    rng = np.random.default_rng(33)
    n, H, W = 3, 30, 44
    Qi = cases.reprojection(60.0, (W - 1) / 2.0 + 0.25, (H - 1) / 2.0 - 0.5, 0.2)
    P = ref.projection(Qi)
    c2w = cases.fusion_poses(n, rng)
    d = cases.fusion_maps(rng, n, H, W)
    img = rng.integers(0, 256, (n, 3, H, W)).astype(np.uint8)
    vol = cd.TSDFVolume(cases.DIMS, cases.VS, cases.ORIGIN)
    td, ti, tp = dev(d), dev(img), dev(ref.world_to_camera(c2w))
    iws = torch.empty(native.LIB.smx_tsdf_integrate_workspace_bytes(n, H, W), dtype=torch.uint8, device="cuda")
    rws = torch.empty(native.LIB.smx_tsdf_raycast_workspace_bytes(*cases.DIMS), dtype=torch.uint8, device="cuda")
    views, Qr = ("outside", "oblique"), cases.q_of("middlebury")
    VH, VW = cases.SHAPE
    vp = dev(rc.view_pose(cases.poses_of(views)))
    out = {"disparity": torch.empty((2, VH, VW), device="cuda"), "depth": torch.empty((2, VH, VW), device="cuda"),
           "normals": torch.empty((2, 3, VH, VW), device="cuda"),
           "colors": torch.empty((2, 3, VH, VW), dtype=torch.uint8, device="cuda"),
           "weight": torch.empty((2, VH, VW), device="cuda")}
    nx, ny, nz = cases.DIMS
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        rcode = native.LIB.smx_tsdf_integrate(0, nx, ny, nz, (C.c_float * 3)(*cases.ORIGIN), cases.VS, vol.truncation,
                                              vol.max_weight, vol.tsdf.data_ptr(), vol.weight.data_ptr(),
                                              vol.color.data_ptr(), n, H, W, td.data_ptr(),
                                              (C.c_float * 16)(*Qi.reshape(-1).tolist()),
                                              (C.c_float * 16)(*P.reshape(-1).tolist()), tp.data_ptr(), None, 0.0, 0.0,
                                              math.inf, -1.0, ti.data_ptr(), 3, native.DTYPE_U8, iws.data_ptr(),
                                              iws.numel(), C.c_void_p(s.cuda_stream))
        assert rcode == 0, native.last_error()
        raycast_call(native, vol, 2, cases.SHAPE, Qr, vp, step_of(1.0), cases.DEPTH_RANGE, out["disparity"], out["depth"],
                     out["normals"], out["colors"], out["weight"], rws, s.cuda_stream)
    torch.cuda.synchronize()
    vol.reset()
    torch.cuda.synchronize()
    state = ref.empty_state(cases.DIMS)
    for f in range(2):
        d2 = d if f == 0 else cases.fusion_maps(rng, n, H, W, zmean=1.3)
        td.copy_(dev(d2))
        graph.replay()
        torch.cuda.synchronize()
        ref.integrate_ref(state, cases.DIMS, cases.ORIGIN, cases.VS, vol.truncation, vol.max_weight, d2, Qi, P,
                          ref.world_to_camera(c2w), image=img)
        want = rc.raycast_ref(state, cases.DIMS, cases.ORIGIN, cases.VS, Qr, rc.view_pose(cases.poses_of(views)),
                              cases.SHAPE, depth_range=cases.DEPTH_RANGE)
        cases.assert_same({k: v.cpu().numpy() for k, v in out.items()}, want, f"replay {f}")
        assert np.isfinite(want["depth"]).mean() > 0.2


def test_pipeline_model_disparity_map(cd):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, D = 48, 96, 16
    Q = cd.reprojection_matrix(50.0, W / 2.0, H / 2.0, 0.1)
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=0, max_disparity=D - 1,
                                        stereo_matching_backend="cuda", left_right_check=True)
    dims, vs, origin = (40, 24, 48), 0.05, (-1.0, -0.6, 0.2)
    vol = cd.TSDFVolume(dims, vs, origin)
    pipe = DepthEstimationPipeline(cfg, reprojection_matrix=Q, tsdf_volume=vol, point_cloud_depth_range=(0.0, 4.0),
                                   render_model=True)
    state = ref.empty_state(dims)
    rng = np.random.default_rng(4)
    hits = 0
    for f in range(3):
        left, right, _ = syn.make_pair(H, W, D, 2, f)
        L, R = syn.gray_to_rgb(left).astype(np.uint8), syn.gray_to_rgb(right).astype(np.uint8)
        pose = ref.look_at(rng.uniform(-0.1, 0.1, 3), np.array([0.0, 0.0, 1.5]))
        res = pipe.process(torch.from_numpy(L), torch.from_numpy(R), camera_pose=pose)
        torch.cuda.synchronize()
        assert res.model_disparity_map.shape == (H, W) and res.model_disparity_map.dtype == torch.float32
        ref.integrate_ref(state, dims, origin, vs, vol.truncation, vol.max_weight, res.disparity_map.cpu().numpy()[None], Q,
                          ref.projection(Q), ref.world_to_camera(pose), image=res.left_image.cpu().numpy()[None],
                          depth_range=(0.0, 4.0), invalid_disparity=cfg.invalid_disparity)
        *_, depth_range = vol._check_render_args(Q, pose, (H, W), 1.0, None, None, False, False, cfg.invalid_disparity)
        want = rc.raycast_ref(state, dims, origin, vs, Q, rc.view_pose(pose), (H, W), depth_range=depth_range,
                              invalid_disparity=cfg.invalid_disparity)
        cases.assert_same({"disparity": res.model_disparity_map.cpu().numpy()[None]}, want, f"frame {f}")
        hits += int((want["disparity"] != cfg.invalid_disparity).sum())
    assert hits > 0
    plain = DepthEstimationPipeline(cfg, reprojection_matrix=Q, tsdf_volume=cd.TSDFVolume(dims, vs, origin))
    assert plain.process(torch.from_numpy(L), torch.from_numpy(R), camera_pose=pose).model_disparity_map is None
