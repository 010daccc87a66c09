"""The point-cloud, TSDF, speckle and metrics kernels at production batch sizes, bit for bit against their NumPy references
(tests/points3d_ref.py, tests/tsdf_ref.py, tests/postprocess_ref.py, and the numpy_metrics rule of tests/test_metrics.py
for the metrics, whose absolute-error sum is a float64 sum compared to 2e-6 relative).  Each case runs a kernel past the
size at which it takes another code path; the sizes are in tests/scale_cases.py, and tests/test_scale_geometry_cpu.py
checks against the kernel sources that every case still crosses its threshold.

    case                                    path it reaches
    test_reprojection_c2_batch              k_reproj_scan: 32 C2 maps, 12,000 rows, 12 rows per thread
    test_reprojection_scan_edges            k_reproj_scan at n*H = 1024, 1025, 2049 (1, 2, 3 rows per thread)
    test_voxel_c2_batch                     the padded, uninitialised tail of reproject_to_3d_batched's output as input;
                                            launch_scan: flag scan of 3,639 blocks (k_scan_top with 4 sums per thread),
                                            histogram scan of 230 blocks; k_vox_bbox's grid-stride loop (57 trips);
                                            the radix sort with ~80 tiles per map, and at 1 mm voxels all 8 passes
    test_voxel_scan_edge_clamped_offsets    launch_scan at cap = 2^22 (Lf = cap + 1: 1,025 blocks, 2 sums per thread);
                                            offsets the device must clamp (first > 0, empty, decreasing, past cap)
    test_voxel_one_huge_voxel               k_vox_reduce and k_vox_heads over one voxel of > 16 k chunks of 64 points
    test_tsdf_c2_maps_nx512                 k_tsdf_integrate with 8 x-blocks and a partial group of 4 rows (8 C2 maps
                                            in one call, then 1); k_tsdf_scatter's two 256-wide chunks per row, also
                                            with a capacity cut inside a second chunk
    test_tsdf_extract_states                k_tsdf_scatter over three chunks per row (the last partial); the extraction
                                            row scan at 1,057 blocks (2 sums per thread) and at exactly 1,024
    test_speckles_and_fill_c2_batch         k_spk_flatten and k_spk_finalize past 8192 workgroups (two grid-stride
                                            trips): 6 C2 maps, speckle sizes 100 and 12, then the fill
    test_metrics_4k_batch                   k_metrics past 1024 workgroups per map, n = 4 maps on blockIdx.y
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import points3d_ref as pref                         # noqa: E402
import postprocess_ref as sref                      # noqa: E402
import scale_cases as sc                            # noqa: E402
import tsdf_ref as tref                             # noqa: E402
from test_metrics import numpy_metrics              # noqa: E402

F, CX, CY, B = 721.5, 609.5, 172.8, 0.54            # KITTI-like C2 intrinsics
MIN_CONF = 0.2


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


def assert_equal(got, expect, what):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    e = np.asarray(expect)
    assert g.shape == e.shape, f"{what}: shape {g.shape} != {e.shape}"
    bad = np.argwhere(g != e)
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first at {tuple(bad[0])}"


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def q_c2(cd):
    return cd.reprojection_matrix(F, CX, CY, B)


# ---- 1. reprojection ---------------------------------------------------------------------------------------------------

def c2_maps(rng, n, H, W):
    """Disparities uniform in 0.3..96 px (depths 4 m .. 1.3 km) with 10 % invalid and 1 % NaN pixels, a u8 RGB frame and
    a confidence map with NaNs."""
    d = rng.uniform(0.3, 96.0, (n, H, W)).astype(np.float32)
    r = rng.random((n, H, W), dtype=np.float32)
    d[r < 0.10] = -1.0
    d[(r >= 0.10) & (r < 0.11)] = np.nan
    img = rng.integers(0, 256, (n, 3, H, W), dtype=np.uint8)
    conf = rng.random((n, H, W), dtype=np.float32)
    conf.reshape(-1)[::97] = np.nan
    return d, img, conf


@pytest.fixture(scope="module")
def c2_batch(cd):
    """The 32 C2 maps of case 1 and their reference reprojection (points, colours, indices, offsets, xyz_map)."""
    n, H, W = sc.REPROJ_BATCH
    d, img, conf = c2_maps(np.random.default_rng(2024), n, H, W)
    Q = q_c2(cd)
    return d, img, conf, Q, pref.reproject_ref(d, Q, img, conf, MIN_CONF)


def test_reprojection_c2_batch(cd, c2_batch):
    d, img, conf, Q, exp = c2_batch
    n, H, W = d.shape
    p, c, i, o, xyz = cd.reproject_to_3d_batched(dev(d), Q, image=dev(img), confidence=dev(conf),
                                                 min_confidence=MIN_CONF, organized=True)
    torch.cuda.synchronize()
    assert_equal(o, exp[3], "offsets")
    assert np.diff(exp[3]).min() >= sc.REPROJ_MIN_KEPT * H * W, "a map keeps too few points for many radix tiles"
    tot = int(exp[3][-1])
    assert_bitwise(p[:tot], exp[0], "points")
    assert_equal(c[:tot], exp[1], "colours")
    assert_equal(i[:tot], exp[2], "indices")
    assert_bitwise(xyz, exp[4], "xyz_map")


@pytest.mark.parametrize("n,H,W", sc.REPROJ_EDGES)
def test_reprojection_scan_edges(cd, n, H, W):
    rng = np.random.default_rng(n * H + W)
    d, _, conf = c2_maps(rng, n, H, W)
    d[0, : H // 3] = -1.0                                         # empty rows: the row scan adds zeros
    img = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    Q = cd.reprojection_matrix(F, W / 2.0, H / 2.0, B)
    p, c, i, o, xyz = cd.reproject_to_3d_batched(dev(d), Q, image=dev(img), confidence=dev(conf),
                                                 min_confidence=MIN_CONF, organized=True)
    torch.cuda.synchronize()
    exp = pref.reproject_ref(d, Q, img, conf, MIN_CONF)
    tot = int(exp[3][-1])
    assert_equal(o, exp[3], "offsets")
    assert_bitwise(p[:tot], exp[0], "points")
    assert_equal(c[:tot], exp[1], "colours")
    assert_equal(i[:tot], exp[2], "indices")
    assert_bitwise(xyz, exp[4], "xyz_map")


# ---- 2 - 4. voxel downsampling -----------------------------------------------------------------------------------------

def key_bits(points, offsets, voxel_size):
    """The width of the device's radix key for this batch: the bits of the kept voxel indices' range per axis + 1."""
    idx, ok = pref._voxel_index(np.asarray(points[offsets[0]:offsets[-1]], np.float32), voxel_size)
    kept = idx[ok]
    return sum(int(kept[:, a].max() - kept[:, a].min()).bit_length() for a in range(3)) + 1


def voxel_check(cd, pts_dev, off_dev, cols_dev, exp_in, vs, mp, what):
    """voxel_downsample_batched on the device arrays against voxel_ref of exp_in = (points, colours, offsets)."""
    vp, vc, vk, vo, vd = cd.voxel_downsample_batched(pts_dev, off_dev, vs, colors=cols_dev, min_points=mp)
    torch.cuda.synchronize()
    e = pref.voxel_ref(*exp_in, vs, mp)
    tot = int(e[3][-1])
    assert_equal(vo, e[3], f"{what}: offsets")
    assert_equal(vd, e[4], f"{what}: dropped")
    assert_equal(vk[:tot], e[2], f"{what}: counts")
    assert_bitwise(vp[:tot], e[0], f"{what}: centroids")
    if cols_dev is not None:
        assert_equal(vc[:tot], e[1], f"{what}: colours")
    return e


@pytest.mark.parametrize("vs,mp,colours", sc.VOXEL_BATCH_RUNS)
def test_voxel_c2_batch(cd, c2_batch, vs, mp, colours):
    """Chained as tools/points_throughput.py does: the padded output of reproject_to_3d_batched, whose rows past
    offsets[n] were never written, goes straight to voxel_downsample_batched."""
    d, img, conf, Q, exp = c2_batch
    p, c, _, o, _ = cd.reproject_to_3d_batched(dev(d), Q, image=dev(img), confidence=dev(conf),
                                               min_confidence=MIN_CONF, indices=False)
    assert p.shape[0] == d.size                                   # the capacity is n*H*W, the tail uninitialised
    pts, cols, off = exp[0], exp[1], exp[3]
    if vs < 0.01:
        assert key_bits(pts, off, vs) >= sc.VOXEL_WIDE_KEY_BITS, "the fine voxel size no longer needs every pass"
    e = voxel_check(cd, p, o, c if colours else None, (pts, cols if colours else None, off), vs, mp, f"{vs} m")
    assert_equal(o, off, "offsets of the reprojection")
    if mp > 1 or vs < 0.01:
        assert e[4].min() > 0, "the drop path is not exercised"


def test_voxel_scan_edge_clamped_offsets(cd):
    cap = sc.VOXEL_SCAN_EDGE_CAP
    rng = np.random.default_rng(77)
    pts = rng.uniform(-20.0, 20.0, (cap, 3)).astype(np.float32)
    pts[::1001, 1] = np.nan                                       # dropped: NaN coordinate
    pts[5::1003, 2] = np.float32(2 ** 21)                         # dropped: index past 2^20 at 0.5 m
    cols = rng.integers(0, 256, (cap, 3), dtype=np.uint8)
    off = np.asarray(sc.VOXEL_SCAN_EDGE_OFFSETS, np.int64)
    clamped = pref.clamp_offsets(off, cap)
    assert clamped[0] > 0 and clamped[-1] == cap and np.any(np.diff(clamped) == 0)
    e = voxel_check(cd, dev(pts), dev(off.astype(np.int32)), dev(cols), (pts, cols, clamped), 0.5, 1, "scan edge")
    assert e[3][-1] > 100_000 and e[4].max() > 0


def test_voxel_one_huge_voxel(cd):
    """One voxel of 1.05 M points (> 16 k chunks of 64), interleaved with a few small voxels, and a second map."""
    rng = np.random.default_rng(5)
    big = rng.random((sc.VOXEL_BIG_POINTS, 3), dtype=np.float32)                     # voxel (0, 0, 0) at 1 m
    small = (rng.integers(-3, 3, (sc.VOXEL_BIG_OTHERS, 1)) * np.array([[1, 2, -1]]) +
             rng.random((sc.VOXEL_BIG_OTHERS, 3))).astype(np.float32)
    small[np.all(np.floor(small) == 0, axis=1)] += np.float32(7.0)                    # keep them out of the big voxel
    m0 = np.concatenate([big, small])[rng.permutation(sc.VOXEL_BIG_POINTS + sc.VOXEL_BIG_OTHERS)]
    m1 = rng.uniform(-2.0, 2.0, (500, 3)).astype(np.float32)
    pts = np.concatenate([m0, m1])
    cols = rng.integers(0, 256, (len(pts), 3), dtype=np.uint8)
    off = np.array([0, len(m0), len(pts)], np.int64)
    e = voxel_check(cd, dev(pts), dev(off.astype(np.int32)), dev(cols), (pts, cols, off), 1.0, 1, "huge voxel")
    assert e[2].max() == sc.VOXEL_BIG_POINTS and e[3][1] <= 20


# ---- 5 - 6. TSDF -------------------------------------------------------------------------------------------------------

TSDF_VS = 0.03
TSDF_ORIGIN = (-7.68, -0.555, 10.0)                 # 15.36 x 1.11 x 2.1 m, 10 m in front of the cameras


def tsdf_maps(rng, n, H, W):
    """Disparities of a bumpy surface 10.6 .. 11.6 m away (f*B = 389.6), with invalid, NaN and outlier pixels."""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.empty((n, H, W), np.float32)
    for f in range(n):
        z = 11.1 + 0.5 * np.sin(u / 53.0 + f) * np.cos(v / 31.0) + rng.normal(0, 0.005, (H, W))
        d[f] = (F * B / z).astype(np.float32)
    r = rng.random((n, H, W))
    d[r < 0.05] = -1.0
    d[(r >= 0.05) & (r < 0.06)] = np.nan
    out = (r >= 0.06) & (r < 0.07)
    d[out] = rng.uniform(1.0, 100.0, int(out.sum()))
    return d


def tsdf_poses(rng, n):
    return np.stack([tref.look_at(rng.uniform(-0.2, 0.2, 3), np.array([0.0, 0.0, 11.0]) + rng.uniform(-0.3, 0.3, 3))
                     for _ in range(n)])


def voxel_rows_of_points(state, nx, min_weight):
    """(row, i) of every extracted point, in output order: row = k*ny + j, i the x voxel."""
    vi, _ = np.nonzero(tref.crossings(state["tsdf"], state["weight"], min_weight))
    return vi // nx, vi % nx


def test_tsdf_c2_maps_nx512(cd):
    import cuda_depth._native as native
    dims = sc.TSDF_MAPS_DIMS
    nx, ny, nz = dims
    n8, n1 = sc.TSDF_MAPS_N
    H, W = sc.C2_H, sc.C2_W
    rng = np.random.default_rng(512)
    Q = q_c2(cd)
    d = tsdf_maps(rng, n8 + n1, H, W)
    img = rng.integers(0, 256, (n8 + n1, 3, H, W), dtype=np.uint8)
    conf = rng.random((n8 + n1, H, W), dtype=np.float32)
    conf.reshape(-1)[::13] = np.nan
    conf.reshape(-1)[::11] = 0.0
    c2w = tsdf_poses(rng, n8 + n1)
    vol = cd.TSDFVolume(dims, TSDF_VS, TSDF_ORIGIN, color=True)
    state = tref.empty_state(dims)
    kw = dict(min_confidence=0.1)
    vol.integrate(dev(d[:n8]), Q, c2w[:n8], image=dev(img[:n8]), confidence=dev(conf[:n8]), **kw)
    vol.integrate(dev(d[n8]), Q, c2w[n8], image=dev(img[n8]), confidence=dev(conf[n8]), **kw)   # one [H, W] map
    for sl in (slice(0, n8), slice(n8, n8 + n1)):
        tref.integrate_ref(state, dims, TSDF_ORIGIN, TSDF_VS, vol.truncation, vol.max_weight, d[sl], Q,
                           tref.projection(Q), tref.world_to_camera(c2w[sl]), image=img[sl], confidence=conf[sl], **kw)
    torch.cuda.synchronize()
    assert_bitwise(vol.tsdf, state["tsdf"], "tsdf")
    assert_bitwise(vol.weight, state["weight"], "weight")
    assert_equal(vol.color, state["color"], "color")
    assert (state["weight"] > 0).mean() >= 0.10, "the volume is barely measured"

    ep, en, ec = tref.extract_ref(state, dims, TSDF_ORIGIN, TSDF_VS, 1.0)
    rows, xs = voxel_rows_of_points(state, nx, 1.0)
    assert len(ep) > 10_000 and (xs >= 256).sum() > 1_000, "too few crossings in the second chunk of the rows"
    cloud = vol.extract_point_cloud()
    assert_bitwise(cloud.points, ep, "points")
    assert_bitwise(cloud.normals, en, "normals")
    assert_equal(cloud.colors, ec, "colours")

    # a capacity that ends inside the second chunk of a row: the prefix is written, nothing past it, the count is the total
    inside = np.flatnonzero((xs[1:] >= 256) & (xs[:-1] >= 256) & (rows[1:] == rows[:-1])) + 1
    assert inside.size, "no row with two crossings in its second chunk"
    cap = int(inside[inside.size // 2])                           # points of that chunk on both sides of the cut
    assert xs[cap - 1] >= 256 and xs[cap] >= 256 and rows[cap - 1] == rows[cap]
    pts = torch.full((cap + 5, 3), 7.0, device="cuda")
    nrm = torch.full((cap + 5, 3), 7.0, device="cuda")
    col = torch.full((cap + 5, 3), 7, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws_bytes = native.LIB.smx_tsdf_extract_workspace_bytes(nx, ny, nz)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    rc = native.LIB.smx_tsdf_extract_points(0, nx, ny, nz, (C.c_float * 3)(*TSDF_ORIGIN), TSDF_VS, vol.tsdf.data_ptr(),
                                            vol.weight.data_ptr(), vol.color.data_ptr(), 1.0, cap, pts.data_ptr(),
                                            nrm.data_ptr(), col.data_ptr(), count.data_ptr(), ws.data_ptr(), ws_bytes,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, native.last_error()
    torch.cuda.synchronize()
    assert int(count.item()) == len(ep)
    assert_bitwise(pts[:cap], ep[:cap], "prefix points")
    assert_bitwise(nrm[:cap], en[:cap], "prefix normals")
    assert_equal(col[:cap], ec[:cap], "prefix colours")
    assert bool((pts[cap:] == 7.0).all() and (nrm[cap:] == 7.0).all() and (col[cap:] == 7).all()), "written past cap"


@pytest.mark.parametrize("dims", sc.TSDF_STATE_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_tsdf_extract_states(cd, dims):
    """Extraction of states written directly: T uniform in (-1.2, 1.2), weights from {0, 0.5, 1, 3}, random colours."""
    nx, ny, nz = dims
    rng = np.random.default_rng(nx * 7 + ny)
    origin, vs = (-1.0, 2.0, 0.5), 0.04
    state = {"tsdf": rng.uniform(-1.2, 1.2, (nz, ny, nx)).astype(np.float32),
             "weight": rng.choice(np.array([0.0, 0.5, 1.0, 3.0], np.float32), (nz, ny, nx)),
             "color": rng.integers(0, 256, (nz, ny, nx, 4), dtype=np.uint8)}
    vol = cd.TSDFVolume(dims, vs, origin, color=True)
    vol.tsdf.copy_(dev(state["tsdf"]))
    vol.weight.copy_(dev(state["weight"]))
    vol.color.copy_(dev(state["color"]))
    ep, en, ec = tref.extract_ref(state, dims, origin, vs, 1.0)
    assert len(ep) > 0.05 * nx * ny * nz
    pts, nrm, col, count = vol.extract_point_cloud_batched(len(ep) + 3)
    torch.cuda.synchronize()
    assert int(count.item()) == len(ep)
    assert_bitwise(pts[:len(ep)], ep, "points")
    assert_bitwise(nrm[:len(ep)], en, "normals")
    assert_equal(col[:len(ep)], ec, "colours")


# ---- 7. speckle filter and fill ----------------------------------------------------------------------------------------

BLOBS = [(1, 1), (1, 2), (2, 2), (3, 4), (2, 6), (1, 12), (13, 1), (3, 5), (4, 4), (7, 7), (9, 11), (10, 10),
         (1, 100), (101, 1), (10, 11), (11, 11), (12, 12), (5, 40), (4, 25), (3, 33), (2, 50), (6, 17)]


def speckle_maps(rng, n, H, W):
    """LR-checked-like maps: vertical bands of slanted planes quantised to 1/16 px, blobs of 1 .. 200 pixels well away
    from their surroundings (a third of them across 32-pixel tile borders), a patch of per-pixel noise (regions of a
    few pixels), 8 % invalid pixels and some NaNs and infinities."""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.empty((n, H, W), np.float32)
    for m in range(n):
        edges = np.sort(rng.choice(np.arange(40, W - 40), 11, replace=False))
        band = np.searchsorted(edges, u, side="right")
        a, bu, bv = rng.uniform(5, 90, 12), rng.uniform(-0.03, 0.03, 12), rng.uniform(0.0, 0.1, 12)
        d = np.round((a[band] + bu[band] * u + bv[band] * v) * 16.0) / 16.0
        for b in range(450):
            h, w = BLOBS[rng.integers(len(BLOBS))]
            if h > H - 2 or w > W - 2:
                continue
            if b % 3 == 0:                                        # straddle a tile corner
                x0 = int(np.clip(32 * rng.integers(1, H // 32 + 1) - h // 2, 0, H - h))
                y0 = int(np.clip(32 * rng.integers(1, W // 32 + 1) - w // 2, 0, W - w))
            else:
                x0, y0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
            d[x0:x0 + h, y0:y0 + w] = d[x0, y0] + rng.choice([-1, 1]) * rng.uniform(4.0, 20.0)
        x0, y0 = int(rng.integers(0, H - 40)), int(rng.integers(0, W - 60))
        d[x0:x0 + 40, y0:y0 + 60] = rng.integers(0, 40, (40, 60)) * 0.75
        r = rng.random((H, W))
        d[r < 0.08] = -1.0
        d[(r >= 0.08) & (r < 0.085)] = np.nan
        d[(r >= 0.085) & (r < 0.086)] = np.inf
        out[m] = d
    return out


def test_speckles_and_fill_c2_batch(cd):
    n, H, W = sc.SPECKLE_N, sc.C2_H, sc.C2_W
    d = speckle_maps(np.random.default_rng(6), n, H, W)
    t = dev(d)
    for size in sc.SPECKLE_SIZES:
        got = cd.filter_speckles(t, max_speckle_size=size, max_diff=1.0)
        filled = cd.fill_invalid(got)
        torch.cuda.synchronize()
        g, gf = got.cpu().numpy(), filled.cpu().numpy()
        removed = 0
        for m in range(n):
            exp = sref.filter_speckles(d[m], size, 1.0, -1.0)
            assert_bitwise(g[m], exp, f"size {size}, map {m}: speckles")
            assert_bitwise(gf[m], sref.fill_invalid(exp, -1.0), f"size {size}, map {m}: fill")
            removed += int(((exp == -1.0) & (d[m] != -1.0)).sum())
        assert removed > 1000 * n, f"size {size}: the filter removed almost nothing"
    assert_bitwise(t, d, "input untouched")


# ---- 8. metrics --------------------------------------------------------------------------------------------------------

MAX_DISP = 192.0


def metric_maps(rng, n, H, W):
    """n (estimate, ground truth) pairs of different content: gaussian errors; heavy tails with invalid ground truth (0,
    negative, past max_disp); uniform errors on a slanted plane; scaled estimates with NaN / inf ground truth."""
    est, gt = np.empty((n, H, W), np.float32), np.empty((n, H, W), np.float32)
    v, u = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    for m in range(n):
        kind = m % 4
        if kind == 0:
            g = rng.uniform(0.5, 200.0, (H, W))
            e = g + rng.normal(0.0, 2.0, (H, W))
        elif kind == 1:
            g = rng.uniform(-20.0, 250.0, (H, W))
            g[rng.random((H, W)) < 0.2] = 0.0
            e = g + rng.laplace(0.0, 3.0, (H, W))
        elif kind == 2:
            g = 10.0 + 0.02 * u + 0.01 * v
            e = g + rng.uniform(-10.0, 10.0, (H, W))
        else:
            g = rng.uniform(1.0, 180.0, (H, W))
            e = g * 1.1 - 1.0
            r = rng.random((H, W))
            g[r < 0.05] = np.nan
            g[(r >= 0.05) & (r < 0.06)] = np.inf
        gt[m], est[m] = g, e
    return est, gt


def numpy_sums(est, gt, mask):
    """numpy_metrics' rule (tests/test_metrics.py) as the kernel's sums: count, D1, > 1, 2, 3, 5 (exact) and the float64
    sum of the float32 |e - g|."""
    e, g = est[mask], gt[mask]
    E = np.abs(e - g)
    with np.errstate(divide="ignore", invalid="ignore"):
        d1 = (E > 3) & (E / np.abs(g) > np.float32(0.05))
    counts = [E.size, int(d1.sum())] + [int((E > t).sum()) for t in (1, 2, 3, 5)]
    return counts, float(E.astype(np.float64).sum())


def test_metrics_4k_batch(cd):
    from pipeline.depth_estimation_pipeline_metrics import FusedDisparityMetrics
    n, H, W = sc.METRICS_SHAPE
    rng = np.random.default_rng(4096)
    est, gt = metric_maps(rng, n, H, W)
    with np.errstate(invalid="ignore"):
        default_masks = (gt <= np.float32(MAX_DISP)) & (gt > 0)
    given = (rng.random((n, H, W)) < 0.6) & np.isfinite(gt)
    te, tg = dev(est), dev(gt)
    for masks, arg in ((default_masks, None), (given, dev(given))):
        s = FusedDisparityMetrics.sums(te, tg, arg, MAX_DISP).cpu().numpy()
        for m in range(n):
            what = f"{'given' if arg is not None else 'default'} mask, map {m}"
            counts, asum = numpy_sums(est[m], gt[m], masks[m])
            assert s[m, :6].tolist() == [float(c) for c in counts], f"{what}: counts {s[m, :6]} != {counts}"
            assert abs(s[m, 6] - asum) <= 2e-6 * asum, f"{what}: |e - g| sum {s[m, 6]!r} vs {asum!r}"
            if arg is None:                                       # the same sums give numpy_metrics' ratios
                with np.errstate(divide="ignore", invalid="ignore"):
                    want = numpy_metrics(est[m], gt[m], MAX_DISP)
                got = [np.float32(np.float32(c) / np.float32(s[m, 0])) for c in s[m, 1:6]]
                assert np.array_equal(np.array(got, np.float32), want[:5].astype(np.float32)), what
