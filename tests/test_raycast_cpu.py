"""Ray casting of TSDF volumes without a GPU: the rule of smx_tsdf_raycast (include/stereo_mi355x.h) as its NumPy twin
(tests/raycast_ref.py) states it -- the quality of a rendered novel view of the fused analytic scene against the scene
itself and against the extracted points, and the rays that must not hit -- then the C ABI's declaration, export, size
query and argument checks, and the Python-level errors of TSDFVolume.render and of the pipeline's render_model."""
import ctypes as C
import dataclasses
import inspect
import math
import os
import re

import numpy as np
import pytest

import raycast_ref as rc
import tsdf_ref as ref

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stereo_mi355x.h")
NEW_SYMBOLS = ("smx_tsdf_raycast", "smx_tsdf_raycast_workspace_bytes")


@pytest.fixture(scope="module")
def cd():
    import cuda_depth
    return cuda_depth


def q_matrix(fx, cx, cy, B):
    return np.array([[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, fx], [0, 0, 1 / B, 0]], np.float64).astype(f32)


# ---- quality on the analytic scene ------------------------------------------------------------------------------------

def test_novel_view_of_the_fused_scene():
    """(a) at least 0.95 of the pixels whose true surface point lies inside the volume are hits (0.976 here);
    (b) the hit points are no farther (RMS) from the true surface than extract_ref's points of the same volume
    (0.0041 m against 0.0089 m here)."""
    dims, vs, origin = (56, 40, 60), 0.05, (-1.4, -1.0, 0.6)
    scene = ref.Scene(ground_y=0.8, boxes=[((-0.7, 0.1, 1.6), (0.1, 0.8, 2.3)), ((0.3, -0.3, 2.2), (0.9, 0.8, 2.8))])
    H, W, fx, B = 40, 56, 60.0, 0.2
    cx, cy = (W - 1) / 2 + 0.25, (H - 1) / 2 - 0.5
    Q = q_matrix(fx, cx, cy, B)
    state = ref.empty_state(dims, False)
    for a in np.linspace(0, 2 * np.pi, 8, endpoint=False):
        c2w = ref.look_at(np.array([0.5 * np.cos(a), -0.2 + 0.1 * np.sin(a), 0.2 * np.sin(a)]), (0.0, 0.5, 2.2))
        d = scene.render(c2w, H, W, fx, cx, cy, B)[None]
        ref.integrate_ref(state, dims, origin, vs, 3 * vs, 64.0, d, Q, ref.projection(Q), ref.world_to_camera(c2w),
                          depth_range=(0.2, 6.0))
    novel = ref.look_at(np.array([0.15, -0.25, 0.1]), (0.05, 0.45, 2.2))            # a pose that was not fused
    out = rc.raycast_ref(state, dims, origin, vs, Q, rc.view_pose(novel), (H, W), depth_range=(0.2, 6.0))
    depth = out["depth"][0]
    hit = np.isfinite(depth)
    assert np.array_equal(hit, out["disparity"][0] != -1.0)
    truth = scene.render(novel, H, W, fx, cx, cy, B)
    tz = np.where(truth > 0, fx * B / np.maximum(truth, 1e-9), np.inf)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")

    def world(lam):
        pc = np.stack([(u - cx) / fx * lam, (v - cy) / fx * lam, lam], -1)
        return pc @ novel[:3, :3].T + novel[:3, 3]

    lo = np.array(origin)
    hi = lo + np.array(dims) * vs
    tw = world(np.where(np.isfinite(tz), tz, 0.0))
    reach = np.isfinite(tz) & ((tw > lo) & (tw < hi)).all(-1)
    assert reach.mean() > 0.5
    coverage = (hit & reach).sum() / reach.sum()
    rms_cast = np.sqrt((scene.distance(world(depth)[hit]) ** 2).mean())
    pts, _, _ = ref.extract_ref(state, dims, origin, vs, 1.0)
    rms_points = np.sqrt((scene.distance(pts) ** 2).mean())
    print(f"coverage {coverage:.4f}, rms of hit points {rms_cast:.4f} m, of extracted points {rms_points:.4f} m")
    assert coverage >= 0.95
    assert rms_cast <= rms_points
    # disparity and depth say the same, normals are unit vectors facing the camera, weights are the fused ones
    dd = out["disparity"][0][hit]
    assert np.allclose(dd, fx * B / depth[hit], rtol=1e-5)
    nrm = out["normals"][0][:, hit]
    length = np.linalg.norm(nrm, axis=0)
    assert ((np.abs(length - 1) < 1e-5) | (length == 0)).all() and (length > 0).mean() > 0.99
    rays = world(np.ones_like(depth))[hit] - novel[:3, 3]
    assert ((nrm.T * rays).sum(1)[length > 0] < 0).mean() > 0.99
    assert (out["weight"][0][hit] >= 1.0).all() and (out["weight"][0][~hit] == 0).all()
    assert (out["normals"][0][:, ~hit] == 0).all() and out["colors"] is None


# ---- rays that must not hit ---------------------------------------------------------------------------------------------

S, DIMS, ORIGIN = 0.125, (12, 12, 24), (-0.75, -0.75, 0.0)
SHAPE = (9, 9)
Q_SMALL = q_matrix(40.0, 4.0, 4.0, 0.1)
IDENTITY = np.eye(4)
ALIGNED = (0.0625, 2.9)              # identity pose: p_z = lam, so lam_m = (m + 0.5) * S are voxel centres exactly


def layered(tsdf_of_z, weight=1.0):
    """A volume whose tsdf depends on z only: tsdf_of_z(voxel centre z) [nz]."""
    nx, ny, nz = DIMS
    zc = (np.arange(nz, dtype=f32) + f32(0.5)) * f32(S)
    state = ref.empty_state(DIMS, True)
    state["tsdf"][:] = np.asarray(tsdf_of_z(zc), f32)[:, None, None]
    state["weight"][:] = weight
    state["color"][..., 0] = (np.arange(nz, dtype=np.uint8) * 10)[:, None, None]
    return state


def cast(state, Q=Q_SMALL, depth_range=ALIGNED, **kw):
    return rc.raycast_ref(state, DIMS, ORIGIN, S, Q, rc.view_pose(IDENTITY), SHAPE, depth_range=depth_range, **kw)


def assert_no_hit(out):
    assert (out["disparity"] == -1.0).all() and np.isnan(out["depth"]).all()
    assert (out["normals"] == 0).all() and (out["weight"] == 0).all() and (out["colors"] == 0).all()


def ramp(zc):
    return np.clip((f32(1.5) - zc) / f32(0.375), -1, 1)


def test_a_wall_is_hit_where_it_stands():
    out = cast(layered(ramp))
    assert np.allclose(out["depth"], 1.5, atol=1e-5) and np.allclose(out["disparity"], 40.0 * 0.1 / 1.5, rtol=1e-5)
    assert np.allclose(out["normals"][0, 2], -1.0) and np.allclose(out["normals"][0, :2], 0.0)
    assert (out["weight"] == 1.0).all()
    assert set(np.unique(out["colors"][0, 0])) <= {110, 120} and (out["colors"][0, 1:] == 0).all()
    assert rc.sample_count(*ALIGNED, S) == 23


def test_a_ray_that_starts_behind_the_surface_does_not_hit():
    assert_no_hit(cast(layered(ramp), depth_range=(0.0625 + 13 * S, 2.9)))          # the first sample has T = -0.5


def test_a_jump_from_truncated_free_space_does_not_hit():
    assert_no_hit(cast(layered(lambda zc: np.where(zc < 1.5, 1.0, -0.5))))
    out = cast(layered(lambda zc: np.where(zc < 1.5, 0.99, -0.5)))                  # the control: just inside the band
    assert np.isfinite(out["depth"]).all()


def test_unmeasured_voxels_are_walked_through_and_end_nothing():
    assert_no_hit(cast(layered(ramp, weight=0.0)))
    assert_no_hit(cast(layered(ramp, weight=0.5)))                                  # below min_weight = 1
    assert np.isfinite(cast(layered(ramp, weight=0.5), min_weight=0.5)["depth"]).all()
    state = layered(ramp)
    state["weight"][11] = 0.0            # the layer in front of the crossing: sample m-1 is invalid, the ray ends unhit
    assert_no_hit(cast(state))
    state = layered(ramp)
    state["weight"][4:6] = 0.0           # a gap in free space is walked through
    assert np.allclose(cast(state)["depth"], 1.5, atol=1e-5)


def test_pixels_without_a_ray():
    q = Q_SMALL.copy()
    q[2, 3] = -40.0                                                                  # Z' <= 0 everywhere
    assert_no_hit(cast(layered(ramp), Q=q))
    q[2, 3] = 0.0
    assert_no_hit(cast(layered(ramp), Q=q))


# ---- the C ABI --------------------------------------------------------------------------------------------------------------

def test_c_abi_is_declared_and_exported():
    import cuda_depth._native as native
    text = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", text), name
        assert name in native.EXPORTS, name
        assert getattr(native.LIB, name) is not None
        assert name in text.split("Conventions")[0], f"{name} is missing from the header's list of entry points"
    out = os.popen(f"nm -D --defined-only {native.LIB_PATH}").read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT " + name + r"\b", out), name
    assert native.LIB.smx_abi_version() == 4
    assert len(native.EXPORTS["smx_tsdf_raycast"][1]) == 27


def test_workspace_query():
    import cuda_depth._native as native
    q = native.LIB.smx_tsdf_raycast_workspace_bytes
    for bad in ((0, 8, 8), (8, -1, 8), (8, 8, 4097), (4097, 1, 1), (4096, 4096, 65), (1025, 1024, 1024)):
        assert q(*bad) == 0, bad
    for dims in ((1, 1, 1), (8, 8, 8), (9, 8, 8), (37, 29, 41), (512, 256, 512), (4096, 4096, 64), (1024, 1024, 1024),
                 (1, 4096, 4096)):
        bricks = math.prod((d + 7) // 8 for d in dims)
        assert q(*dims) == 2 * ((bricks + 255) // 256 * 256), dims  # two bytes per brick, each array aligned
    assert q(512, 256, 512) == 2 * 131072


def test_c_abi_rejects_bad_arguments_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: an accepted call would launch kernels on invented addresses")
    import cuda_depth._native as native
    lib, bad = native.LIB, native.SMX_OK - 1                          # SMX_ERR_INVALID_ARG = -1
    wsb = lib.smx_tsdf_raycast_workspace_bytes(16, 12, 10)
    inf, nan = math.inf, math.nan
    keep = []

    def floats(values):
        arr = (C.c_float * len(values))(*values)
        keep.append(arr)
        return arr

    Q = q_matrix(40.0, 4.0, 4.0, 0.1).reshape(-1).tolist()

    def q_with(k, v):
        return floats(Q[:k] + [v] + Q[k + 1:])

    def p(addr):
        return C.c_void_p(addr)

    # the volume 16 x 12 x 10: 7680 bytes per f32 array; 2 views of 6 x 8: 384 bytes per f32 plane; workspace 512 bytes
    def call(**kw):
        a = dict(dev=0, nx=16, ny=12, nz=10, origin=floats([0.0, 0.0, 0.0]), vs=0.1, tsdf=p(0x2000000),
                 weight=p(0x3000000), color=p(0x4000000), minw=1.0, n=2, H=6, W=8, Q=floats(Q), pose=p(0x5000000),
                 step=0.1, zmin=0.0, zmax=4.0, invalid=-1.0, disp=p(0x6000000), depth=p(0x7000000),
                 normals=p(0x8000000), colors=p(0x9000000), wout=p(0xa000000), ws=p(0x100000000), wsb=wsb, stream=None)
        a.update(kw)
        return lib.smx_tsdf_raycast(*a.values())

    assert call() == -3 and "cannot select HIP device" in native.last_error()       # valid: stops at the device
    assert call(color=None, depth=None, normals=None, colors=None, wout=None) == -3  # every optional operand NULL
    assert call(zmin=1.0, zmax=1.0) == -3 and call(zmin=0.0, zmax=6553.5, step=0.1) == -3
    broken = dict(
        null=[dict(origin=None), dict(tsdf=None), dict(weight=None), dict(Q=None), dict(pose=None), dict(disp=None),
              dict(ws=None)],
        volume=[dict(nx=0), dict(ny=4097), dict(nz=-1), dict(nx=4096, ny=4096, nz=65), dict(vs=0.0), dict(vs=nan),
                dict(vs=inf), dict(origin=floats([0.0, nan, 0.0])), dict(origin=floats([inf, 0.0, 0.0]))],
        maps=[dict(n=0), dict(H=0), dict(W=32769), dict(H=32769), dict(n=2 ** 20, H=32, W=33)],
        min_weight=[dict(minw=0.0), dict(minw=-1.0), dict(minw=nan), dict(minw=inf)],
        step=[dict(step=0.0), dict(step=-0.1), dict(step=nan), dict(step=inf)],
        z=[dict(zmin=-0.5), dict(zmin=nan), dict(zmax=nan), dict(zmax=inf), dict(zmin=2.0, zmax=1.0), dict(zmin=-inf)],
        samples=[dict(zmax=6554.0, step=0.1), dict(zmax=1.0, step=1e-6)],
        Q=[dict(Q=q_with(5, nan)), dict(Q=q_with(15, inf)), dict(Q=q_with(2, 0.5)), dict(Q=q_with(6, 1.0)),
           dict(Q=q_with(10, -1.0)), dict(Q=q_with(12, 1e-3)), dict(Q=q_with(13, 1.0)), dict(Q=q_with(14, 0.0))],
        invalid_disparity=[dict(invalid=nan), dict(invalid=inf)],
        colors=[dict(color=None)],
        workspace_bytes=[dict(wsb=wsb - 1), dict(wsb=0)],
        overlaps=[dict(disp=p(0x2000000 + 7676)), dict(depth=p(0x3000000)), dict(normals=p(0x4000000 + 7000)),
                  dict(colors=p(0x5000000 + 92)), dict(wout=p(0x2000000 - 380)), dict(ws=p(0x3000000 + 256)),
                  dict(depth=p(0x6000000 + 380)), dict(normals=p(0x7000000 - 1148)), dict(colors=p(0x8000000 + 4)),
                  dict(wout=p(0x9000000 + 287)), dict(ws=p(0xa000000 + 256)), dict(ws=p(0x6000000 + 256))],
        alignment=[dict(ws=p(0x100000000 + 8))],
        stream=[dict(stream=native.STREAM_ENGINE)])
    for rule, cases in broken.items():
        for kw in cases:
            assert call(**kw) == bad, (rule, kw)
            assert "smx_tsdf_raycast" in native.last_error(), (rule, kw, native.last_error())
    # operands just clear of each other are accepted
    assert call(disp=p(0x2000000 + 7680), wout=p(0x2000000 - 384), depth=p(0x6000000 + 384)) == -3
    for kw, word in ((dict(tsdf=None), "non-NULL"), (dict(nx=0), "nx, ny, nz"), (dict(vs=nan), "voxel_size"),
                     (dict(n=0), "n >= 1"), (dict(n=2 ** 20, H=32, W=33), "2^30"), (dict(minw=nan), "min_weight"),
                     (dict(step=0.0), "step"), (dict(zmin=-0.5), "z_min"), (dict(zmax=6554.0), "samples per ray"),
                     (dict(Q=q_with(5, nan)), "Q[5]"), (dict(Q=q_with(10, -1.0)), "must not depend on d"),
                     (dict(invalid=nan), "invalid_disparity"), (dict(color=None), "colour volume"),
                     (dict(wsb=wsb - 1), "smx_tsdf_raycast_workspace_bytes"),
                     (dict(depth=p(0x3000000)), "overlaps an input"), (dict(depth=p(0x6000000 + 380)), "two outputs"),
                     (dict(ws=p(0x100000000 + 8)), "256-byte aligned"), (dict(stream=native.STREAM_ENGINE), "stream")):
        assert call(**kw) == bad and word in native.last_error(), (kw, native.last_error())
    # the order of the rules: the earlier one answers a doubly wrong call
    assert call(tsdf=None, nx=0) == bad and "non-NULL" in native.last_error()
    assert call(minw=nan, step=0.0) == bad and "min_weight" in native.last_error()
    assert call(wsb=0, stream=native.STREAM_ENGINE) == bad and "workspace_bytes" in native.last_error()


# ---- Python ---------------------------------------------------------------------------------------------------------------

def test_python_validation_before_the_device(cd):
    vol = object.__new__(cd.TSDFVolume)                               # the checks run before any state is touched
    vol.dims, vol.voxel_size, vol.origin = (16, 12, 10), 0.1, (0.0, 0.0, 0.0)
    Q = cd.reprojection_matrix(40.0, 4.0, 4.0, 0.1)
    eye = np.eye(4)
    for exc, match, args, kw in (
            (RuntimeError, "Q must be", (np.eye(3), eye, (6, 8)), {}),
            (RuntimeError, "must not depend on the disparity", (np.eye(4), eye, (6, 8)), {}),
            (RuntimeError, "camera_to_world must be", (Q, np.eye(3), (6, 8)), {}),
            (RuntimeError, "finite", (Q, np.full((4, 4), np.nan), (6, 8)), {}),
            (RuntimeError, "last row", (Q, np.ones((2, 4, 4)), (6, 8)), {}),
            (TypeError, "shape", (Q, eye, 6), {}),
            (ValueError, "shape", (Q, eye, (0, 8)), {}),
            (RuntimeError, "2\\^30", (Q, np.stack([eye] * 2), (32768, 32768)), {}),
            (RuntimeError, "min_weight", (Q, eye, (6, 8)), dict(min_weight=0.0)),
            (TypeError, "min_weight", (Q, eye, (6, 8)), dict(min_weight="1")),
            (RuntimeError, "step", (Q, eye, (6, 8)), dict(step=0.0)),
            (RuntimeError, "step", (Q, eye, (6, 8)), dict(step=math.nan)),
            (TypeError, "depth_range", (Q, eye, (6, 8)), dict(depth_range=3.0)),
            (RuntimeError, "depth_range", (Q, eye, (6, 8)), dict(depth_range=(-1.0, 2.0))),
            (RuntimeError, "depth_range", (Q, eye, (6, 8)), dict(depth_range=(2.0, 1.0))),
            (RuntimeError, "depth_range", (Q, eye, (6, 8)), dict(depth_range=(0.0, math.inf))),
            (RuntimeError, "samples per ray", (Q, eye, (6, 8)), dict(depth_range=(0.0, 10.0), step=1e-4)),
            (TypeError, "normals", (Q, eye, (6, 8)), dict(normals=1)),
            (TypeError, "colors", (Q, eye, (6, 8)), dict(colors=None)),
            (RuntimeError, "invalid_disparity", (Q, eye, (6, 8)), dict(invalid_disparity=math.nan))):
        with pytest.raises(exc, match=match):
            vol.render(*args, **kw)
    # the defaults: step = voxel_size, depth_range = 0 .. eye to the farthest corner (float64)
    q, poses, batched, shape, step, (z_min, z_max) = vol._check_render_args(Q, eye, (6, 8), 1.0, None, None, True, True,
                                                                            -1.0)
    assert (batched, shape, step, z_min) == (False, (6, 8), 0.1, 0.0)
    assert z_max == pytest.approx(math.sqrt(1.6 ** 2 + 1.2 ** 2 + 1.0 ** 2), rel=1e-12)
    assert poses.dtype == np.float32 and poses.shape == (1, 3, 4)
    far = eye.copy()
    far[:3, 3] = (-3.0, 0.0, 0.5)
    *_, (_, z_max2) = vol._check_render_args(Q, np.stack([eye, far]), (6, 8), 1.0, 0.05, None, False, False, -1.0)
    assert z_max2 == pytest.approx(math.sqrt(4.6 ** 2 + 1.2 ** 2 + 0.5 ** 2), rel=1e-12)
    # poses are rounded, not inverted
    pose = ref.look_at((0.3, -0.2, 0.1), (0.0, 0.5, 2.0))
    assert np.array_equal(cd.camera_to_world_poses(pose)[0], pose[:3].astype(np.float32))
    sig = inspect.signature(cd.TSDFVolume.render).parameters
    assert list(sig)[1:4] == ["Q", "camera_to_world", "shape"]
    defaults = dict(min_weight=1.0, step=None, depth_range=None, normals=True, colors=True, invalid_disparity=-1.0)
    for name, v in defaults.items():
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == v, name
    assert [f.name for f in dataclasses.fields(cd.RenderedView)] == ["disparity", "depth", "normals", "colors", "weight"]


def test_pipeline_render_model_argument_rules(cd):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig, DepthEstimationResult
    cfg = DepthEstimationPipelineConfig(image_shape=(48, 96), min_disparity=0, max_disparity=15)
    with pytest.raises(ValueError, match="render_model needs tsdf_volume"):
        DepthEstimationPipeline(cfg, render_model=True)
    with pytest.raises(ValueError, match="render_model needs tsdf_volume"):
        DepthEstimationPipeline(cfg, render_model=True, reprojection_matrix=cd.reprojection_matrix(50.0, 48.0, 24.0, 0.1))
    with pytest.raises(TypeError, match="render_model must be a bool"):
        DepthEstimationPipeline(cfg, render_model=1)
    assert inspect.signature(DepthEstimationPipeline.__init__).parameters["render_model"].default is False
    field = {f.name: f for f in dataclasses.fields(DepthEstimationResult)}["model_disparity_map"]
    assert field.default is None and field.kw_only
    assert [f.name for f in dataclasses.fields(DepthEstimationResult) if not f.kw_only][:4] == [
        "left_image", "right_image", "disparity_map", "confidence_map"]
