"""Rectification, the parts that need no GPU: the C-ABI symbol and its argument checks (every SMX_ERR_INVALID_ARG path
returns before the device is touched), the CPU reference of the remap rule (tests/rectify_ref.py) against a plain
per-pixel version and against the exact bilinear value, the map builder and its quantisation, the KITTI helper and the
argument checks of the Python wrappers, the backend and the pipeline."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rectify_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from cuda_depth import _native
    return _native


def random_qmap(rng, Ho, Wo, Hi, Wi, extremes=True):
    q = np.stack([rng.integers(-96, (Wi + 2) * 32, (Ho, Wo)), rng.integers(-96, (Hi + 2) * 32, (Ho, Wo))], -1)
    if extremes:
        pick = rng.random((Ho, Wo, 2)) < 0.1
        q[pick] = rng.choice([I32_MIN, I32_MAX, I32_MIN + 1, I32_MAX - 31, -1, 0, 31, 32], int(pick.sum()))
    return q.astype(np.int32)


def random_images(rng, n, C, H, W, dtype):
    if dtype == np.uint8:
        return rng.integers(0, 256, (n, C, H, W)).astype(np.uint8)
    img = rng.uniform(-300, 300, (n, C, H, W)).astype(np.float32)
    pick = rng.random(img.shape) < 0.05
    img[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], np.float32), int(pick.sum()))
    return img


# ----------------------------------------------------------------------------- the reference against the rule
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("border", [ref.CONSTANT, ref.REPLICATE])
@pytest.mark.parametrize("C_", [1, 3, 4])
def test_reference_matches_the_per_pixel_rule(dtype, border, C_):
    rng = np.random.default_rng(C_ * 10 + border + (dtype == np.uint8) * 100)
    Hi, Wi, Ho, Wo, n = 7, 9, 6, 11, 2
    img = random_images(rng, n, C_, Hi, Wi, dtype)
    q = random_qmap(rng, Ho, Wo, Hi, Wi)
    bv = 77 if dtype == np.uint8 else -12.5
    got = ref.remap(img, q, border, bv)
    assert got.dtype == dtype and got.shape == (n, C_, Ho, Wo)
    for i in range(n):
        for c in range(C_):
            for v in range(Ho):
                for u in range(Wo):
                    e = ref.remap_pixel(img, q, i, c, v, u, border, bv)
                    g = got[i, c, v, u]
                    if dtype == np.uint8:
                        assert int(g) == e, (i, c, v, u)
                    else:
                        assert np.float32(g).view(np.uint32) == np.float32(e).view(np.uint32), (i, c, v, u, g, e)


@pytest.mark.parametrize("border", [ref.CONSTANT, ref.REPLICATE])
def test_uint8_is_the_exact_bilinear_value_rounded_half_up(border):
    rng = np.random.default_rng(3)
    Hi, Wi = 12, 15
    img = random_images(rng, 1, 3, Hi, Wi, np.uint8)
    q = random_qmap(rng, 20, 17, Hi, Wi, extremes=False)
    got = ref.remap(img, q, border, 200)
    x, y = q[..., 0] / 32.0, q[..., 1] / 32.0                   # exact in float64
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    ax, ay = x - x0, y - y0
    exact = np.zeros((3,) + x.shape)
    for dy, dx, wt in ((0, 0, (1 - ax) * (1 - ay)), (0, 1, ax * (1 - ay)), (1, 0, (1 - ax) * ay), (1, 1, ax * ay)):
        yy, xx = y0 + dy, x0 + dx
        inside = (yy >= 0) & (yy < Hi) & (xx >= 0) & (xx < Wi)
        if border == ref.REPLICATE:
            inside[:] = True
        p = img[0][:, np.clip(yy, 0, Hi - 1), np.clip(xx, 0, Wi - 1)].astype(float)
        exact += wt * np.where(inside, p, 200.0)
    np.testing.assert_array_equal(got[0], np.floor(exact + 0.5).astype(np.uint8))


def test_zero_weight_taps_do_not_leak_and_give_plus_zero():
    img = np.array([[[[1.0, np.nan], [np.inf, -np.inf]]]], np.float32)
    q = np.array([[[0, 0], [16, 0], [0, 16]]], np.int32)       # on (0, 0); half way to the NaN; half way to the inf
    got = ref.remap(img, q)
    assert got[0, 0, 0, 0] == 1.0
    assert np.isnan(got[0, 0, 0, 1]) and np.isinf(got[0, 0, 0, 2])
    assert got.view(np.uint32)[0, 0, 0, 1] == 0x7FC00000                # the canonical NaN
    nan = ref.remap(np.array([[[[np.inf, -np.inf]]]], np.float32), np.array([[[16, 0]]], np.int32))
    assert nan.view(np.uint32)[0, 0, 0, 0] == 0x7FC00000               # inf - inf: also canonical
    z = ref.remap(np.full((1, 1, 2, 2), -0.0, np.float32), np.zeros((1, 1, 2), np.int32))
    assert z.view(np.uint32)[0, 0, 0, 0] == 0                  # +0.0: the zero-weight taps add +0.0


# ----------------------------------------------------------------------------- map builder and quantisation
K0 = np.array([[700.0, 0.0, 300.5], [0.0, 690.0, 120.25], [0.0, 0.0, 1.0]])


def test_identity_calibration_gives_the_identity_map_and_image(native):
    import cuda_depth
    Hi, Wi = 40, 64
    mx, my = cuda_depth.rectification_map(K0, np.zeros(5), np.eye(3), np.hstack([K0, np.zeros((3, 1))]), (Hi, Wi),
                                          (Hi, Wi))
    q = cuda_depth.quantize_map(mx, my, (Hi, Wi))
    v, u = np.mgrid[0:Hi, 0:Wi]
    np.testing.assert_array_equal(q[..., 0], 32 * u)
    np.testing.assert_array_equal(q[..., 1], 32 * v)
    rng = np.random.default_rng(0)
    img8 = rng.integers(0, 256, (2, 3, Hi, Wi)).astype(np.uint8)
    np.testing.assert_array_equal(ref.remap(img8, q), img8)
    imgf = rng.uniform(0, 255, (1, 1, Hi, Wi)).astype(np.float32)
    assert np.array_equal(ref.remap(imgf, q).view(np.uint32), imgf.view(np.uint32))
    assert ref.valid_mask(q, (Hi, Wi)).all()


def test_principal_point_shift_shifts_the_map(native):
    import cuda_depth
    P = K0.copy()
    P[0, 2] -= 5.0                                              # rectified principal point 5 px left, 3 px up
    P[1, 2] -= 3.0
    mx, my = cuda_depth.rectification_map(K0, None, np.eye(3), P, (50, 60), (30, 40))
    v, u = np.mgrid[0:30, 0:40]
    np.testing.assert_allclose(mx, u + 5.0, atol=1e-9)
    np.testing.assert_allclose(my, v + 3.0, atol=1e-9)
    q = cuda_depth.quantize_map(mx, my, (50, 60))
    np.testing.assert_array_equal(q[..., 0], 32 * (u + 5))
    np.testing.assert_array_equal(q[..., 1], 32 * (v + 3))


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))


def test_distorted_calibration_matches_a_forward_model(native):
    import cuda_depth
    D = np.array([-0.28, 0.08, 1e-3, -5e-4, -0.01])
    R = _rot(0.01, -0.02, 0.005)
    P = np.array([[650.0, 0.0, 310.0], [0.0, 650.0, 118.0], [0.0, 0.0, 1.0]])
    mx, my = cuda_depth.rectification_map(K0, D, R, P, (240, 600), (200, 580))
    rx, ry = ref.rectification_map(K0, D, R, P, (200, 580))
    np.testing.assert_allclose(mx, rx, rtol=0, atol=1e-9)
    np.testing.assert_allclose(my, ry, rtol=0, atol=1e-9)
    k1, k2, p1, p2, k3 = D
    for v, u in ((0, 0), (17, 311), (199, 579), (100, 3)):     # independent per-pixel model
        X = np.linalg.solve(P @ R, [u, v, 1.0])
        x, y = X[0] / X[2], X[1] / X[2]
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        assert abs(mx[v, u] - (K0[0, 0] * xd + K0[0, 2])) < 1e-7
        assert abs(my[v, u] - (K0[1, 1] * yd + K0[1, 2])) < 1e-7


def test_points_behind_the_camera_are_outside(native):
    import cuda_depth
    R = _rot(0.0, np.pi, 0.0)                                   # looking backwards: X2 < 0 everywhere
    mx, my = cuda_depth.rectification_map(K0, None, R, K0, (10, 10), (4, 5))
    assert np.isnan(mx).all() and np.isnan(my).all()
    q = cuda_depth.quantize_map(mx, my, (10, 10))
    assert (q == -64).all()


def test_quantize_map_rounds_clamps_and_handles_non_finite(native):
    import cuda_depth
    Hi, Wi = 10, 20
    mx = np.array([[0.0, 1.015625, -0.015625, 1e30, -1e30, np.nan, np.inf, -np.inf, 20.99, 5.5 / 32]])
    my = np.array([[0.0, 2.0, 1e12, -3.0, 11.5, 1.0, 0.0, 1.0, np.nan, -1.9]])
    q = cuda_depth.quantize_map(mx, my, (Hi, Wi))
    assert q.dtype == np.int32 and q.shape == (1, 10, 2)
    np.testing.assert_array_equal(q[0, :, 0], [0, 33, 0, 21 * 32, -64, -64, -64, -64, 21 * 32, 6])
    np.testing.assert_array_equal(q[0, :, 1], [0, 64, 11 * 32, -64, 11 * 32, 32, 0, 32, -64, -61])
    np.testing.assert_array_equal(q, ref.quantize_map(mx, my, (Hi, Wi)))
    with pytest.raises(ValueError):
        cuda_depth.quantize_map(mx, my[:, :3], (Hi, Wi))
    with pytest.raises(ValueError):
        cuda_depth.quantize_map(mx, my, (0, Wi))


# ----------------------------------------------------------------------------- KITTI helper
def _write_kitti(dirname, D, R_rect, P_shift):
    def fmt(a):
        return " ".join(f"{v:.9e}" for v in np.asarray(a, float).reshape(-1))
    lines = ["calib_time: 09-Jan-2012 13:57:47", "corner_dist: 9.950000e-02"]
    for c in range(4):
        K = K0.copy()
        P = np.hstack([K0, np.zeros((3, 1))])
        P[0, 2] -= P_shift
        P[0, 3] = -K0[0, 0] * 0.54 * (c == 3)
        lines += [f"S_0{c}: 1.392000e+03 5.120000e+02", f"K_0{c}: {fmt(K)}", f"D_0{c}: {fmt(D)}",
                  f"R_0{c}: {fmt(np.eye(3))}", f"T_0{c}: {fmt(np.zeros(3))}", f"S_rect_0{c}: 1.242000e+03 3.750000e+02",
                  f"R_rect_0{c}: {fmt(R_rect)}", f"P_rect_0{c}: {fmt(P)}"]
    with open(os.path.join(dirname, "calib_cam_to_cam.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def test_kitti_helper_identity_like_rig(native, tmp_path):
    from helpers import kitti_calibration as kc
    _write_kitti(str(tmp_path), np.zeros(5), np.eye(3), 0.0)
    rect = kc.stereo_rectification(str(tmp_path), device="cpu")
    assert rect.in_shape == (512, 1392) and rect.out_shape == (375, 1242)
    lm = rect.left_map.numpy()
    v, u = np.mgrid[0:375, 0:1242]
    np.testing.assert_array_equal(lm[..., 0], 32 * u)
    np.testing.assert_array_equal(lm[..., 1], 32 * v)
    np.testing.assert_array_equal(rect.right_map.numpy(), lm)
    assert rect.left_valid.numpy().all()


def test_kitti_helper_distorted_rig(native, tmp_path):
    import cuda_depth
    from helpers import kitti_calibration as kc
    D = np.array([-0.37, 0.2, 1e-3, 4e-4, -0.07])
    R = _rot(0.004, -0.01, 0.002)
    _write_kitti(str(tmp_path), D, R, 2.0)
    rect = kc.stereo_rectification(str(tmp_path), cams=(2, 3), border_mode="replicate", device="cpu")
    P = np.hstack([K0, np.zeros((3, 1))])
    P[0, 2] -= 2.0
    expect = cuda_depth.quantize_map(*ref.rectification_map(K0, D, R, P, (375, 1242)), (512, 1392))
    got = rect.left_map.numpy()
    assert np.abs(got.astype(np.int64) - expect).max() <= 1          # the two float64 builders may differ in an ulp
    assert rect.border_mode == "replicate"
    np.testing.assert_array_equal(rect.left_valid.numpy(), ref.valid_mask(got, (512, 1392)))


# ----------------------------------------------------------------------------- C ABI
def test_the_symbol_is_declared_listed_and_exported(native):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stereo_mi355x.h")).read(), flags=re.S)
    lib = C.CDLL(native.LIB_PATH)
    assert re.search(r"\bint\s+smx_remap_pairs\s*\(", header)
    for name, value in (("SMX_BORDER_CONSTANT", 0), ("SMX_BORDER_REPLICATE", 1), ("SMX_DTYPE_U8", 0),
                        ("SMX_DTYPE_F32", 1)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", header), name
    assert "smx_remap_pairs" in native.EXPORTS and hasattr(lib, "smx_remap_pairs")
    assert native.LIB.smx_abi_version() == 4


# fake device pointers: never dereferenced, every check returns first
LI, RI, LM, RM, LO, RO = 0x1000000, 0x2000000, 0x3000000, 0x4000000, 0x5000000, 0x6000000


def _call(native, **change):
    a = dict(dev=0, n=2, C=3, dt=0, Hi=8, Wi=8, Ho=8, Wo=8, li=LI, ri=RI, lm=LM, rm=RM, lo=LO, ro=RO, b=0, bv=0.0,
             s=None)
    a.update(change)
    return native.LIB.smx_remap_pairs(a["dev"], a["n"], a["C"], a["dt"], a["Hi"], a["Wi"], a["Ho"], a["Wo"], a["li"],
                                      a["ri"], a["lm"], a["rm"], a["lo"], a["ro"], a["b"], a["bv"], a["s"])


def test_remap_rejects_bad_arguments_without_a_device(native):
    cases = [
        (dict(li=None), "left_in, left_map and left_out must be non-NULL"),
        (dict(lm=None), "left_in, left_map and left_out must be non-NULL"),
        (dict(lo=None), "left_in, left_map and left_out must be non-NULL"),
        (dict(ri=None), "all NULL or all non-NULL"),
        (dict(rm=None), "all NULL or all non-NULL"),
        (dict(ro=None), "all NULL or all non-NULL"),
        (dict(ri=None, rm=None), "all NULL or all non-NULL"),
        (dict(n=0), "need n >= 1"),
        (dict(n=-3), "need n >= 1"),
        (dict(Hi=0), "sizes must be in 1..32768"),
        (dict(Wi=32769), "sizes must be in 1..32768"),
        (dict(Ho=-1), "sizes must be in 1..32768"),
        (dict(Wo=0), "sizes must be in 1..32768"),
        (dict(C=0), "channels must be in 1..4"),
        (dict(C=5), "channels must be in 1..4"),
        (dict(dt=2), "unknown dtype"),
        (dict(dt=-1), "unknown dtype"),
        (dict(b=2), "unknown border mode"),
        (dict(b=-1), "unknown border mode"),
        (dict(bv=float("nan")), "border_value must be finite"),
        (dict(dt=1, bv=float("inf")), "border_value must be finite"),
        (dict(bv=0.5), "integer in 0..255"),
        (dict(bv=-1.0), "integer in 0..255"),
        (dict(bv=256.0), "integer in 0..255"),
        (dict(lo=LI + 100), "overlaps an input or a map"),
        (dict(lo=RI - 10), "overlaps an input or a map"),
        (dict(ro=LM + 8), "overlaps an input or a map"),
        (dict(ro=RM), "overlaps an input or a map"),
        (dict(ro=LO + 64), "left_out and right_out overlap"),
        (dict(s=C.c_void_p(-1)), "needs a caller stream"),
        (dict(n=2 ** 31 - 1, C=4, dt=1, Hi=32768, Wi=32768), "do not fit the address space"),
    ]
    for change, msg in cases:
        rc = _call(native, **change)
        assert rc == -1, (change, rc)
        assert msg in native.last_error(), (change, native.last_error())
    # the right view may be left out altogether; n * C * H * W bytes are computed in 64 bits
    assert _call(native, ri=None, rm=None, ro=None, lo=None) == -1
    assert _call(native, dt=1, bv=-7.25, lo=LI + 8 * 8 * 2 * 3 * 4 - 1) == -1
    assert "overlaps" in native.last_error()


# ----------------------------------------------------------------------------- Python wrappers, backend, pipeline
def _rect(**kw):
    import cuda_depth
    q = np.zeros((6, 8, 2), np.int32)
    return cuda_depth.StereoRectification(q, q, (5, 7), (6, 8), device="cpu", **kw)


def test_stereo_rectification_checks_its_arguments(native):
    import cuda_depth
    q = np.zeros((6, 8, 2), np.int32)
    r = _rect()
    assert r.in_shape == (5, 7) and r.out_shape == (6, 8) and r.border_mode == "constant" and r.border_value == 0.0
    assert r.left_valid.dtype.is_floating_point is False and tuple(r.left_valid.shape) == (6, 8)
    with pytest.raises(ValueError):
        _rect(border_mode="wrap")
    with pytest.raises(ValueError):
        _rect(border_value=float("nan"))
    with pytest.raises(TypeError):
        _rect(border_value="0")
    with pytest.raises(ValueError):
        cuda_depth.StereoRectification(q.astype(np.int64), q, (5, 7), (6, 8), device="cpu")
    with pytest.raises(ValueError):
        cuda_depth.StereoRectification(q, q[:5], (5, 7), (6, 8), device="cpu")
    with pytest.raises(ValueError):
        cuda_depth.StereoRectification(q, q, (5, 0), (6, 8), device="cpu")
    with pytest.raises(ValueError):
        cuda_depth.rectification_map(K0, np.zeros(3), np.eye(3), K0, (5, 7), (6, 8))


def test_rectify_rejects_host_tensors(native):
    import torch
    r = _rect()
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        r.rectify(torch.zeros((3, 5, 7), dtype=torch.uint8), torch.zeros((3, 5, 7), dtype=torch.uint8))
    with pytest.raises(TypeError):
        r.rectify(np.zeros((3, 5, 7), np.uint8))


def test_backend_and_pipeline_take_rectification(native):
    import inspect
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    from pipeline.depth import CudaStereoMatchingBackend
    for cls in (CudaStereoMatchingBackend, DepthEstimationPipeline):
        p = inspect.signature(cls.__init__).parameters["rectification"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    cfg = DepthEstimationPipelineConfig(image_shape=(7, 8), min_disparity=0, max_disparity=3)
    with pytest.raises(ValueError, match="out_shape"):                # (6, 8) against (7, 8), before any device use
        DepthEstimationPipeline(cfg, rectification=_rect())
    import cuda_depth
    with pytest.raises(ValueError, match="out_shape"):
        CudaStereoMatchingBackend(cuda_depth.StereoMatchingConfiguration(height=6, width=9), rectification=_rect())
    with pytest.raises(TypeError):
        CudaStereoMatchingBackend(cuda_depth.StereoMatchingConfiguration(height=6, width=8), rectification=object())
