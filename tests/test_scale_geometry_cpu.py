"""The geometry guard of tests/test_scale_gpu.py: reads the launch constants of the point-cloud, TSDF, speckle and metrics
kernels from their defining lines in the sources and asserts that every case of tests/scale_cases.py still crosses the
size at which its kernel takes the path it is there to test.  A retuned constant that leaves a case below its threshold
fails here, by name, instead of silently shrinking what the GPU file checks."""
import os
import re

import pytest

import scale_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-depth_amd", "csrc")


def source(name: str) -> str:
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def one(pattern: str, name: str) -> int:
    """The single integer captured by `pattern` in csrc/name; fails if the defining line is missing or repeated."""
    found = re.findall(pattern, source(name), flags=re.MULTILINE)
    assert len(found) == 1, f"{name}: expected one line matching {pattern!r}, found {len(found)}"
    return int(found[0])


@pytest.fixture(scope="module")
def k():
    """The constants the cases depend on, read from the kernel sources."""
    c = {}
    c["SCAN_ITEMS"] = one(r"^constexpr int SCAN_ITEMS = (\d+);", "k_reproject.h")
    c["SCAN_THREADS"] = one(r"^constexpr int SCAN_TILE = (\d+) \* SCAN_ITEMS;", "k_reproject.h")
    c["SCAN_TILE"] = c["SCAN_THREADS"] * c["SCAN_ITEMS"]
    c["VOX_TILE"] = one(r"^constexpr int VOX_TILE = (\d+);", "k_reproject.h")
    c["VOX_BBOX_BLOCKS"] = one(r"^constexpr int VOX_BBOX_BLOCKS = (\d+);", "k_reproject.h")
    c["VOX_CHUNK"] = one(r"for \(int c0 = 0; c0 < cnt; c0 \+= (\d+)\)", "k_reproject.h")
    c["DIGIT_BITS"] = one(r"pass_skipped\(const int \*gate, int pass\) \{ return gate && pass \* (\d+) >= \*gate; \}",
                          "k_reproject.h")
    c["PASSES"] = one(r"for \(int pass = 0; pass < (\d+); \+\+pass\)", "tu_reproject.hip")
    # the single-workgroup scans: the block size in the kernel and at its launch must agree
    c["REPROJ_SCAN_THREADS"] = one(r"__launch_bounds__\((\d+)\) void k_reproj_scan\(", "k_reproject.h")
    assert one(r"k_reproj_scan, dim3\(1\), dim3\((\d+)\)", "tu_reproject.hip") == c["REPROJ_SCAN_THREADS"]
    c["TOP_SCAN_THREADS"] = one(r"__launch_bounds__\((\d+)\) void k_scan_top\(", "k_reproject.h")
    assert one(r"k_scan_top, dim3\(1\), dim3\((\d+)\)", "tu_reproject.hip") == c["TOP_SCAN_THREADS"]
    # TSDF integration: x voxels per workgroup and y rows per workgroup, in the launch and in the kernel
    c["TSDF_X"] = one(r"k_tsdf_integrate, dim3\(\(unsigned\)\(\(nx \+ \d+\) / (\d+)\)", "tu_tsdf.hip")
    c["TSDF_Y"] = one(r"\(unsigned\)\(\(ny \+ \d+\) / (\d+)\), \(unsigned\)nz\)", "tu_tsdf.hip")
    assert one(r"const int i = blockIdx\.x \* (\d+) \+", "k_tsdf.h") == c["TSDF_X"]
    assert one(r"const int j = blockIdx\.y \* (\d+) \+", "k_tsdf.h") == c["TSDF_Y"]
    c["TSDF_CHUNK"] = one(r"for \(int x0 = 0; x0 < a\.nx; x0 \+= (\d+)\)", "k_tsdf.h")
    # speckle grid-stride kernels
    c["SPK_THREADS"] = one(r"^constexpr int SPK_THREADS = (\d+);", "k_post.h")
    c["SPK_CAP"] = one(r"if \(blocks > (\d+)\) blocks = \d+;", "tu_post.hip")
    assert one(r"if \(blocks > \d+\) blocks = (\d+);", "tu_post.hip") == c["SPK_CAP"]
    # metrics: items per workgroup and the block cap of launch_metrics
    c["MET_PER_BLOCK"] = one(r"size_t blocks = \(pixels \+ 256 \* (\d+) - 1\) / \(256 \* \d+\);", "tu_stages.hip") * 256
    c["MET_CAP"] = one(r"if \(blocks > (\d+)\) blocks = \d+;\n    hipLaunchKernelGGL\(k_metrics", "tu_stages.hip")
    assert "const int b = blockIdx.y;" in source("k_metrics.h"), "k_metrics no longer takes the map from blockIdx.y"
    return c


def test_reprojection_scan_gives_threads_several_rows(k):
    n, H, _ = sc.REPROJ_BATCH
    T = k["REPROJ_SCAN_THREADS"]
    assert n * H > T and sc.per_thread(n * H, T) >= 4, "the 32-map batch no longer gives each scan thread many rows"
    pers = sorted(sc.per_thread(n * H, T) for n, H, _ in sc.REPROJ_EDGES)
    rows = sorted(n * H for n, H, _ in sc.REPROJ_EDGES)
    assert rows == [T, T + 1, 2 * T + 1], f"edge shapes must have n*H = T, T + 1, 2T + 1 for T = {T}, got {rows}"
    assert pers == [1, 2, 3]


def test_voxel_batch_reaches_multi_block_scans_grid_stride_and_many_tiles(k):
    n, H, W = sc.REPROJ_BATCH
    cap = n * H * W                                                 # the padded output of the reprojection
    Lc, Lf = sc.voxel_scan_lengths(n, cap, k["VOX_TILE"])
    nb_f, nb_c = sc.scan_blocks(Lf, k["SCAN_TILE"]), sc.scan_blocks(Lc, k["SCAN_TILE"])
    assert nb_f > k["TOP_SCAN_THREADS"] and sc.per_thread(nb_f, k["TOP_SCAN_THREADS"]) >= 2, "flag scan"
    assert nb_c > 1, "histogram scan"
    assert sc.voxel_bbox_blocks(cap, k["VOX_BBOX_BLOCKS"]) == k["VOX_BBOX_BLOCKS"]
    assert sc.grid_stride_trips(cap, k["VOX_BBOX_BLOCKS"], 256) >= 2, "k_vox_bbox's grid-stride loop"
    # the GPU test asserts that every map keeps at least REPROJ_MIN_KEPT of its pixels
    assert sc.cdiv(int(sc.REPROJ_MIN_KEPT * H * W), k["VOX_TILE"]) >= 32, "tiles per map"
    assert k["DIGIT_BITS"] * k["PASSES"] == 64
    assert sc.VOXEL_WIDE_KEY_BITS > k["DIGIT_BITS"] * (k["PASSES"] - 1), "the fine voxel size must need every pass"
    assert any(mp > 1 for _, mp, _ in sc.VOXEL_BATCH_RUNS)


def test_voxel_scan_edge_is_the_first_size_with_two_sums_per_thread(k):
    cap = sc.VOXEL_SCAN_EDGE_CAP
    T, tile = k["TOP_SCAN_THREADS"], k["SCAN_TILE"]
    assert sc.scan_blocks(cap, tile) == T, "cap itself must fill the top scan exactly"
    _, Lf = sc.voxel_scan_lengths(len(sc.VOXEL_SCAN_EDGE_OFFSETS) - 1, cap, k["VOX_TILE"])
    assert sc.scan_blocks(Lf, tile) == T + 1 and sc.per_thread(T + 1, T) == 2
    off = sc.VOXEL_SCAN_EDGE_OFFSETS
    assert off[0] > 0 and off[-1] > cap, "offsets the device must clamp at both ends"
    assert any(b < a for a, b in zip(off, off[1:])), "a decreasing entry"
    assert any(b == a for a, b in zip(off, off[1:])), "an empty map"


def test_big_voxel_has_many_chunks(k):
    assert sc.cdiv(sc.VOXEL_BIG_POINTS, k["VOX_CHUNK"]) > 15_000


def test_tsdf_cases_cross_their_blocks_and_chunks(k):
    nx, ny, _ = sc.TSDF_MAPS_DIMS
    gx, _, _ = sc.tsdf_integrate_grid(sc.TSDF_MAPS_DIMS, k["TSDF_X"], k["TSDF_Y"])
    assert gx >= 8 and ny % k["TSDF_Y"] != 0, "x-blocks and a partial y group"
    assert sc.cdiv(nx, k["TSDF_CHUNK"]) == 2, "two scatter chunks per row"
    assert max(sc.TSDF_MAPS_N) > 1 and min(sc.TSDF_MAPS_N) == 1
    (ax, ay, az), (bx, by, bz), (cx, cy, cz) = sc.TSDF_STATE_DIMS
    assert sc.cdiv(ax, k["TSDF_CHUNK"]) == 3 and ax % k["TSDF_CHUNK"] != 0, "three chunks, the last partial"
    T, tile = k["TOP_SCAN_THREADS"], k["SCAN_TILE"]
    nb = sc.scan_blocks(by * bz, tile)
    assert nb > T and sc.per_thread(nb, T) == 2, "extraction row scan past the top scan's width"
    assert sc.scan_blocks(cy * cz, tile) == T and cy * cz == T * tile, "the boundary from the other side"
    for dims in sc.TSDF_STATE_DIMS:
        assert max(dims) <= 4096 and dims[0] * dims[1] * dims[2] <= 2 ** 30, f"{dims}: outside the volume limits"


def test_speckle_batch_passes_the_grid_stride_cap(k):
    px = sc.SPECKLE_N * sc.C2_H * sc.C2_W
    blocks = sc.capped_blocks(px, k["SPK_THREADS"], k["SPK_CAP"])
    assert blocks == k["SPK_CAP"] and sc.grid_stride_trips(px, blocks, k["SPK_THREADS"]) >= 2
    assert max(sc.SPECKLE_SIZES) >= 100 and min(sc.SPECKLE_SIZES) < 32


def test_metrics_batch_passes_the_block_cap(k):
    n, H, W = sc.METRICS_SHAPE
    blocks = sc.capped_blocks(H * W, k["MET_PER_BLOCK"], k["MET_CAP"])
    assert n > 1 and blocks == k["MET_CAP"] and sc.grid_stride_trips(H * W, blocks, 256) > k["MET_PER_BLOCK"] // 256
