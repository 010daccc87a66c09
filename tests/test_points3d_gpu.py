"""Metric 3D points and voxel downsampling on the device (include/stereo_mi355x.h: smx_reproject_points,
smx_voxel_downsample), bit for bit against the NumPy reference (tests/points3d_ref.py): batches, odd and tiny shapes,
every colour source, confidence, the organised map, batch independence, run-to-run determinism, graph replay and the
pipeline's point_cloud for both backends, with and without rectification."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import points3d_ref as ref                          # noqa: E402
import rectify_ref                                  # noqa: E402
import stereo_synthetic as syn                      # noqa: E402

F, CX, CY, B = 721.5, 609.5, 172.8, 0.54


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


def q_matrix(cd, H, W, doffs=0.0):
    return cd.reprojection_matrix(F, (W - 1) / 2.0 + 0.25, (H - 1) / 2.0 - 0.5, B, fy=F * 1.01, cx_right=None if not doffs
                                  else (W - 1) / 2.0 + 0.25 + doffs)


def maps(rng, n, H, W):
    """Disparities in (0, 100) with invalid, NaN, inf, zero and negative pixels."""
    d = rng.uniform(0.5, 100.0, (n, H, W)).astype(np.float32)
    r = rng.random((n, H, W))
    d[r < 0.10] = -1.0
    d[(r >= 0.10) & (r < 0.12)] = np.nan
    d[(r >= 0.12) & (r < 0.13)] = np.inf
    d[(r >= 0.13) & (r < 0.14)] = 0.0
    d[(r >= 0.14) & (r < 0.15)] = -3.0
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
    v.reshape(-1)[5::23] = np.float32(127.5)
    return v


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_batched(cd, d, Q, img=None, conf=None, **kw):
    p, c, i, o, xyz = cd.reproject_to_3d_batched(dev(d), Q, image=dev(img), confidence=dev(conf), organized=True, **kw)
    torch.cuda.synchronize()
    o = o.cpu().numpy()
    tot = int(o[-1])
    return (p[:tot].cpu().numpy(), None if c is None else c[:tot].cpu().numpy(), i[:tot].cpu().numpy(), o,
            xyz.cpu().numpy())


COLOURS = [None, (1, "u8"), (3, "u8"), (1, "f32"), (3, "f32")]


@pytest.mark.parametrize("n,H,W", [(1, 1, 1), (1, 7, 13), (3, 33, 257), (3, 5, 300), (32, 24, 70), (1, 64, 1)])
@pytest.mark.parametrize("colour", COLOURS)
def test_reprojection_matches_reference(cd, n, H, W, colour):
    rng = np.random.default_rng(n * 1000 + H * 7 + W + (0 if colour is None else colour[0] * 11))
    d = maps(rng, n, H, W)
    img = image(rng, n, H, W, colour)
    Q = q_matrix(cd, H, W, doffs=3.5)
    got = run_batched(cd, d, Q, img, depth_range=(0.5, 400.0))
    exp = ref.reproject_ref(d, Q, img, depth_range=(0.5, 400.0))
    assert np.array_equal(got[3], exp[3]), "offsets"
    assert_bitwise(got[0], exp[0], "points")
    assert np.array_equal(got[2], exp[2]), "indices"
    if colour is None:
        assert got[1] is None
    else:
        assert np.array_equal(got[1], exp[1]), "colors"
    assert_bitwise(got[4], exp[4], "xyz_map")


@pytest.mark.parametrize("min_conf", [0.0, 0.4])
def test_reprojection_with_confidence(cd, min_conf):
    rng = np.random.default_rng(3)
    n, H, W = 3, 31, 77
    d = maps(rng, n, H, W)
    conf = rng.random((n, H, W)).astype(np.float32)
    conf.reshape(-1)[::13] = np.nan
    Q = q_matrix(cd, H, W)
    got = run_batched(cd, d, Q, None, conf, min_confidence=min_conf, invalid_disparity=-3.0)
    exp = ref.reproject_ref(d, Q, None, conf, min_conf, invalid_disparity=-3.0)
    assert np.array_equal(got[3], exp[3])
    assert_bitwise(got[0], exp[0], "points")
    assert np.array_equal(got[2], exp[2])
    assert_bitwise(got[4], exp[4], "xyz_map")


def test_order_offsets_and_batch_independence(cd):
    rng = np.random.default_rng(9)
    n, H, W = 5, 40, 90
    d = maps(rng, n, H, W)
    d[2] = -1.0                                                   # an empty map inside the batch
    img = image(rng, n, H, W, (3, "u8"))
    Q = q_matrix(cd, H, W)
    clouds = cd.reproject_to_3d(dev(d), Q, image=dev(img))
    assert len(clouds) == n and clouds[2].points.shape == (0, 3)
    for i in range(n):
        idx = clouds[i].indices.cpu().numpy()
        assert np.all(np.diff(idx) > 0), "row-major order"
        alone = cd.reproject_to_3d(dev(d[i]), Q, image=dev(img[i]))
        assert_bitwise(alone.points, clouds[i].points, f"map {i} alone")
        assert np.array_equal(alone.colors.cpu().numpy(), clouds[i].colors.cpu().numpy())
        assert np.array_equal(alone.indices.cpu().numpy(), idx)


def scene_cloud(cd, rng, n, H, W):
    d = rng.uniform(2.0, 80.0, (n, H, W)).astype(np.float32)
    d[rng.random((n, H, W)) < 0.1] = -1.0
    img = image(rng, n, H, W, (3, "u8"))
    Q = cd.reprojection_matrix(F, W / 2.0, H / 2.0, B)
    return d, img, Q


def voxel_check(cd, pts, cols, off, vs, mp):
    p, c, k, o, dr = cd.voxel_downsample_batched(dev(pts), dev(np.asarray(off, dtype=np.int32)), vs,
                                                   colors=dev(cols), min_points=mp)
    torch.cuda.synchronize()
    o = o.cpu().numpy()
    tot = int(o[-1])
    e = ref.voxel_ref(pts, cols, off, vs, mp)
    assert np.array_equal(o, e[3]), "offsets"
    assert np.array_equal(dr.cpu().numpy(), e[4]), "dropped"
    assert_bitwise(p[:tot], e[0], "centroids")
    assert np.array_equal(k[:tot].cpu().numpy(), e[2]), "counts"
    if cols is not None:
        assert np.array_equal(c[:tot].cpu().numpy(), e[1]), "colours"
    return p[:tot].cpu().numpy(), o


@pytest.mark.parametrize("vs,mp", [(0.05, 1), (0.2, 1), (0.5, 3), (5.0, 1), (1e-6, 1)])
def test_voxel_matches_reference(cd, vs, mp):
    rng = np.random.default_rng(int(vs * 1000) + mp)
    n, H, W = 3, 48, 120
    d, img, Q = scene_cloud(cd, rng, n, H, W)
    pts, cols, _, off, _ = ref.reproject_ref(d, Q, img)
    voxel_check(cd, pts, cols, off, vs, mp)


def test_voxel_edge_cases(cd):
    rng = np.random.default_rng(5)
    pts = rng.normal(0.0, 3.0, (5000, 3)).astype(np.float32)      # negative coordinates
    pts[:300] = np.float32(0.25)                                   # one big voxel (several chunks of 64)
    pts[400] = np.float32((2 ** 20 - 1) * 0.5)                     # index 2^20 - 1 at voxel 0.5: kept
    pts[401] = np.float32(2 ** 19)                                 # index 2^20 at 0.5: dropped
    pts[402] = np.float32(-(2 ** 20) * 0.5)                        # index -2^20: kept
    pts[403, 1] = np.nan
    pts[404, 2] = -np.inf
    cols = rng.integers(0, 256, (5000, 3)).astype(np.uint8)
    for vs, mp in ((0.5, 1), (0.5, 2), (1000.0, 1), (0.01, 1)):
        off = [0, 1, 1, 2000, 5000]                                # a one-point map, an empty map
        voxel_check(cd, pts, cols, off, vs, mp)
        voxel_check(cd, pts, None, off, vs, mp)


@pytest.mark.parametrize("mp", [1, 2])
def test_voxel_700_tiny_maps(cd, mp):
    """700 maps of 0..6 points, many of them empty (tests/project_cases.py: tiny_clouds, folded into one octant): one
    partial tile and one slice of the histograms per map, and the dropped counts of many maps inside one wave.  At 3 m
    the voxels are about half as many as the points."""
    import project_cases
    Q = cd.reprojection_matrix(60.0, 2.25, 0.5, 0.3, fy=60.6)
    pts, off, _ = project_cases.tiny_clouds(700, 700, 6, 3, 5, Q)
    pts = np.abs(pts)
    cols = np.random.default_rng(700).integers(0, 256, (len(pts), 3)).astype(np.uint8)
    e = ref.voxel_ref(pts, cols, off, 3.0, mp)
    assert 0.4 < ref.voxel_ref(pts, None, off, 3.0, 1)[3][-1] / off[-1] < 0.6
    assert (np.diff(off) == 0).sum() > 100 and (mp == 1 or (e[4] > 0).sum() > 200)
    voxel_check(cd, pts, cols, off, 3.0, mp)
    voxel_check(cd, pts, None, off, 3.0, mp)


def test_voxel_independent_of_batch_and_runs(cd):
    rng = np.random.default_rng(21)
    n, H, W = 4, 40, 100
    d, img, Q = scene_cloud(cd, rng, n, H, W)
    pts, cols, _, off, _ = ref.reproject_ref(d, Q, img)
    a1 = cd.voxel_downsample_batched(dev(pts), dev(off.astype(np.int32)), 0.1, colors=dev(cols))
    a2 = cd.voxel_downsample_batched(dev(pts), dev(off.astype(np.int32)), 0.1, colors=dev(cols))
    tot = int(a1[3][-1])                                          # rows past the total are not written
    assert torch.equal(a1[3], a2[3]) and torch.equal(a1[4], a2[4])
    assert_bitwise(a1[0][:tot], a2[0][:tot], "two runs")
    assert torch.equal(a1[1][:tot], a2[1][:tot]) and torch.equal(a1[2][:tot], a2[2][:tot])
    clouds = [cd.PointCloud(points=dev(pts[off[i]:off[i + 1]]), colors=dev(cols[off[i]:off[i + 1]]))
              for i in range(n)]
    together = cd.voxel_downsample(clouds, 0.1)
    for i in range(n):
        alone = cd.voxel_downsample(clouds[i], 0.1)
        assert_bitwise(alone.points, together[i].points, f"map {i}")
        assert torch.equal(alone.colors, together[i].colors) and torch.equal(alone.counts, together[i].counts)


def test_graph_replay(cd):
    rng = np.random.default_rng(33)
    n, H, W = 2, 30, 64
    d, img, Q = scene_cloud(cd, rng, n, H, W)
    td, ti = dev(d), dev(img)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        p, c, i, o, _ = cd.reproject_to_3d_batched(td, Q, image=ti)
        vp, vc, vk, vo, vd = cd.voxel_downsample_batched(p, o, 0.2, colors=c)
    for f in range(2):
        d2 = d if f == 0 else d * np.float32(1.5)
        td.copy_(dev(d2))
        graph.replay()
        torch.cuda.synchronize()
        pts, cols, _, off, _ = ref.reproject_ref(d2, Q, img)
        assert np.array_equal(o.cpu().numpy(), off)
        assert_bitwise(p[:off[-1]], pts, f"replay {f}: points")
        e = ref.voxel_ref(pts, cols, off, 0.2, 1)
        tot = int(vo[-1])
        assert np.array_equal(vo.cpu().numpy(), e[3])
        assert_bitwise(vp[:tot], e[0], f"replay {f}: centroids")
        assert np.array_equal(vc[:tot].cpu().numpy(), e[1])


def test_python_errors(cd):
    t = torch.zeros((2, 4, 8), device="cuda")
    Q = np.eye(4, dtype=np.float32)
    with pytest.raises(RuntimeError, match="image must be"):
        cd.reproject_to_3d(t, Q, image=torch.zeros((2, 2, 4, 8), device="cuda"))
    with pytest.raises(RuntimeError, match="confidence must be float32"):
        cd.reproject_to_3d(t, Q, confidence=t[:1])
    with pytest.raises(RuntimeError, match="offsets must be int32"):
        cd.voxel_downsample_batched(torch.zeros((4, 3), device="cuda"), torch.zeros(3, device="cuda"), 0.1)


@pytest.mark.parametrize("backend", ["cuda", "sgm"])
@pytest.mark.parametrize("rectified", [False, True])
def test_pipeline_point_cloud(cd, backend, rectified):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W, D = 48, 96, 16
    left, right, _ = syn.make_pair(H, W, D, 2, 3)
    L, R = syn.gray_to_rgb(left).astype(np.uint8), syn.gray_to_rgb(right).astype(np.uint8)
    Q = cd.reprojection_matrix(50.0, W / 2.0, H / 2.0, 0.1)
    rect = None
    if rectified:
        v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        qm = rectify_ref.quantize_map(u * 0.98 + 1.0, v * 0.98 + 0.5, (H, W))
        rect = cd.StereoRectification(qm, qm, (H, W), (H, W))
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=0, max_disparity=D - 1,
                                        stereo_matching_backend=backend, left_right_check=True)
    for vs in (0.0, 0.05):
        pipe = DepthEstimationPipeline(cfg, reprojection_matrix=Q, point_cloud_voxel_size=vs, confidence=True,
                                       point_cloud_min_confidence=0.1, point_cloud_depth_range=(0.0, 4.0),
                                       rectification=rect)
        res = pipe.process(torch.from_numpy(L), torch.from_numpy(R))
        assert res.point_cloud is not None and res.confidence_map is not None
        exp = cd.reproject_to_3d(res.disparity_map, Q, image=res.left_image, confidence=res.confidence_map,
                                 min_confidence=0.1, depth_range=(0.0, 4.0), invalid_disparity=cfg.invalid_disparity)
        if vs > 0:
            exp = cd.voxel_downsample(exp, vs)
        got = res.point_cloud
        assert got.points.shape[0] > 0
        assert_bitwise(got.points, exp.points, f"{backend} vs {vs}")
        assert torch.equal(got.colors, exp.colors)
        if vs > 0:
            assert torch.equal(got.counts, exp.counts)
        else:
            assert torch.equal(got.indices, exp.indices)
        plain = DepthEstimationPipeline(cfg, rectification=rect).process(torch.from_numpy(L), torch.from_numpy(R))
        assert plain.point_cloud is None
        assert_bitwise(plain.disparity_map, res.disparity_map, "the map does not change")
