"""The geometry guard of tests/test_scale_gpu.py and tests/test_launch_caps_gpu.py: reads the launch constants of the
point-cloud, TSDF, speckle and metrics kernels, and the grid caps of the map entries' launchers, from their defining lines
in the sources and asserts that every case of tests/scale_cases.py still crosses the size at which its kernel takes the
path it is there to test.  A retuned constant that leaves a case below its threshold fails here, by name, instead of
silently shrinking what the GPU files check."""
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
    c["SCAN_ITEMS"] = one(r"^constexpr int SCAN_ITEMS = (\d+);", "smx_workspace.h")
    c["SCAN_THREADS"] = one(r"^constexpr int SCAN_TILE = (\d+) \* SCAN_ITEMS;", "smx_workspace.h")
    c["SCAN_TILE"] = c["SCAN_THREADS"] * c["SCAN_ITEMS"]
    c["VOX_TILE"] = one(r"^constexpr int VOX_TILE = (\d+);", "smx_workspace.h")
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


# ---- the map entries past their grid caps (tests/test_launch_caps_gpu.py) ----------------------------------------------

@pytest.fixture(scope="module")
def m():
    """The grid caps of the map entries' launchers and the kernel constants their loops stride by."""
    c = {}
    c["CONF_MAPS"] = one(r"const unsigned maps = \(unsigned\)\(n < (\d+) \? n : \1\);", "tu_confidence.hip")
    c["TEMP_MAPS"] = one(r"const unsigned maps = \(unsigned\)\(n < (\d+) \? n : \1\);", "tu_temporal.hip")
    c["SGM_IMAGES"] = one(r"const unsigned images = \(unsigned\)\(2 \* n < (\d+) \? 2 \* n : \1\);", "tu_sgm.hip")
    c["SGM_GROUPS"] = 1 << one(r"groups < \(\(size_t\)1 << (\d+)\) \? groups : \(\(size_t\)1 << \1\)", "tu_sgm.hip")
    c["SGM_THREADS"] = one(r"^constexpr int SGM_THREADS = (\d+);", "k_sgm.h")
    c["MED_TILES"] = 1 << one(r"tiles < \(\(size_t\)1 << (\d+)\) \? tiles : \(\(size_t\)1 << \1\)", "tu_median.hip")
    c["MED_TH"] = one(r"^constexpr int MED_TH = (\d+), MED_TW = \d+;", "k_median.h")
    c["MED_TW"] = one(r"^constexpr int MED_TH = \d+, MED_TW = (\d+);", "k_median.h")
    c["WLS_BLOCKS"] = 1 << one(r"blocks < \(\(size_t\)1 << (\d+)\) \? blocks : \(\(size_t\)1 << \1\)", "tu_wls.hip")
    c["WLS_LINES"] = one(r"^constexpr int WLS_LINES = (\d+);", "k_wls.h")
    c["WLS_COL_THREADS"] = one(r"^constexpr int WLS_COL_THREADS = (\d+);", "k_wls.h")
    c["WLS_PB"] = one(r"^constexpr int WLS_PB = (\d+);", "k_wls.h")
    c["REMAP_CHUNKS"] = one(r"if \(chunks > (\d+)\) chunks = \1;", "tu_remap.hip")
    c["REMAP_IPT"] = one(r"^constexpr int REMAP_IPT = (\d+);", "k_remap.h")
    c["LR_BLOCKS"] = one(r"if \(blocks > (\d+)\) blocks = \1;", "tu_lr.hip")
    c["LR_THREADS"] = one(r"^constexpr int LR_THREADS = (\d+);", "k_lr.h")
    c["LR_PACK_ITEMS"] = one(r"^constexpr int LR_PACK_ITEMS = (\d+);", "k_lr.h")
    c["LR_LDS_W"] = one(r"^constexpr int LR_LDS_W = (\d+);", "k_lr.h")
    c["TRACK_TRIPLES"] = one(r"const unsigned triples = \(unsigned\)\(n < (\d+) \? n : \1\);", "k_track_body.h")
    # the loops the cases are there to send on a second trip, and what the launchers divide by
    for name, text in (("k_confidence.h", "m += gridDim.y"), ("k_temporal.h", "m += gridDim.y"),
                       ("k_sgm.h", "z += gridDim.y"), ("k_sgm.h", "p += waves"), ("k_median.h", "tile += gridDim.x"),
                       ("k_wls.h", "line0 += (size_t)gridDim.x * WLS_LINES"),
                       ("k_wls.h", "line += (size_t)gridDim.x * WLS_COL_THREADS"), ("k_lr.h", "c += stride"),
                       ("k_lr.h", "i += stride"), ("k_lr.h", "it += stride"),
                       ("k_remap.h", "min((long long)p.n, (long long)(chunk + 1) * p.ipt)"),
                       ("tu_wls.hip", "grid_of((size_t)n * H, WLS_LINES)"),
                       ("tu_wls.hip", "grid_of((size_t)n * W, WLS_COL_THREADS)"),
                       ("tu_sgm.hip", "(pixels + SGM_THREADS / 64 - 1) / (SGM_THREADS / 64)"),
                       ("tu_lr.hip", "const bool lds = W <= LR_LDS_W;"),
                       ("k_track_body.h", "for (int f = blockIdx.y; f < a.n; f += gridDim.y)"),
                       ("k_track_body.h", "for (int f = blockIdx.x; f < a.n; f += gridDim.x)"),
                       ("k_track_body.h", "hipLaunchKernelGGL(accum, dim3((unsigned)g.groups, triples)"),
                       ("k_track_body.h", "hipLaunchKernelGGL(solve, dim3(triples)"),
                       ("k_track.h", "void k_track_accum(const TrackArgs a) { track_accum_body<TrackRule>(a); }"),
                       ("k_track.h", "void k_track_solve(const TrackArgs a) { track_solve_body<TrackRule>(a); }"),
                       ("tu_track.hip", "track_launch<TrackRule>(c, a, k_track_begin, k_track_accum, k_track_solve, s)")):
        assert text in source(name), f"{name} no longer holds {text!r}: restate the case's geometry in scale_cases.py"
    return c


def test_confidence_and_temporal_maps_take_a_second_trip(m):
    strides = []
    for shape, cap in ((sc.CONF_CAP_SHAPE, m["CONF_MAPS"]), (sc.TEMPORAL_CAP_SHAPE, m["TEMP_MAPS"])):
        n, H, W = shape
        grid, stride, trips = sc.map_grid_y(n, cap)
        assert grid == cap and trips >= 2, f"{shape}: n no longer passes the cap of {cap} maps"
        assert n - cap >= 2, "more than one workgroup row must take the second trip"
        strides.append(stride)
    assert sc.TEMPORAL_FRAMES >= 3 and 1 <= sc.MAP_RADIUS <= 7
    assert sc.tile_period_ok(strides), strides


def test_sgm_images_and_pixels_take_a_second_trip(m):
    n, H, W, dmin, D = sc.SGM_CAP_CASE
    grid, stride, trips, left2, right2 = sc.sgm_census_grid(n, m["SGM_IMAGES"])
    assert grid == m["SGM_IMAGES"] and trips >= 2 and left2 >= 1 and right2 >= 1, (grid, trips, left2, right2)
    sgrid, sstride, strips = sc.sgm_select_grid(n, H, W, m["SGM_THREADS"], m["SGM_GROUPS"])
    assert sgrid == m["SGM_GROUPS"] and strips >= 2, "the pixels no longer pass the cap of the selection kernels"
    assert D <= 64, "the main case runs one disparity per lane"
    wn, wH, wW, wdmin, wD = sc.SGM_CAP_WIDE_CASE
    wgrid, wstride, wtrips, _, wright2 = sc.sgm_census_grid(wn, m["SGM_IMAGES"])
    assert wgrid == m["SGM_IMAGES"] and wtrips >= 2 and wright2 >= 1
    assert wD > 128 and wdmin + wD - 1 < wW + wD, "the wide case runs four disparities per lane"
    assert sc.tile_period_ok([stride, sstride, wstride]), (stride, sstride, wstride)


def test_median_tiles_take_a_second_trip(m):
    n, H, W = sc.MEDIAN_CAP_SHAPE
    per_map, grid, stride, trips = sc.median_grid(n, H, W, m["MED_TH"], m["MED_TW"], m["MED_TILES"])
    assert per_map == 1, "one tile per map: the tile index is the map index"
    assert grid == m["MED_TILES"] and trips >= 2 and n - grid >= 2
    assert sc.tile_period_ok([stride]), stride


def test_wls_lines_take_a_second_trip(m):
    strides = []
    (n, H, W), (n2, H2, W2), (n3, H3, W3) = sc.WLS_CAP_SHAPES
    (rg, rs, rt), (cg, cs, ct) = sc.wls_grids(n, H, W, m["WLS_LINES"], m["WLS_COL_THREADS"], m["WLS_BLOCKS"])
    assert rg == m["WLS_BLOCKS"] and rt >= 2, "rows of the first shape no longer pass the rows cap"
    assert cg == m["WLS_BLOCKS"] and ct >= 2, "columns of the first shape no longer pass the columns cap"
    assert W >= 2, "the first shape couples pixels along its rows"
    strides += [rs, cs]
    (rg, rs, rt), (cg, cs, ct) = sc.wls_grids(n2, H2, W2, m["WLS_LINES"], m["WLS_COL_THREADS"], m["WLS_BLOCKS"])
    assert rg == m["WLS_BLOCKS"] and rt >= 2 and cg == m["WLS_BLOCKS"] and ct >= 2
    assert H2 >= 2, "the second shape couples pixels along its columns"
    strides += [rs, cs]
    (rg, rs, rt), _ = sc.wls_grids(n3, H3, W3, m["WLS_LINES"], m["WLS_COL_THREADS"], m["WLS_BLOCKS"])
    assert rg == m["WLS_BLOCKS"] and rt >= 2, "rows of the third shape no longer pass the rows cap"
    assert H3 > 2 * m["WLS_PB"], "the third shape's columns take several groups of loads"
    strides.append(rs)
    assert sc.WLS_CAP_ITERATIONS >= 2, "a second iteration reads what the first one's strided trips wrote"
    assert sc.tile_period_ok(strides), strides


def test_remap_takes_more_images_per_thread_and_a_partial_last_chunk(m):
    n, Hi, Wi, Ho, Wo = sc.REMAP_CAP_CASE
    ipt, chunks, last = sc.remap_chunks(n, m["REMAP_IPT"], m["REMAP_CHUNKS"])
    assert ipt > m["REMAP_IPT"], f"n = {n} no longer passes {m['REMAP_CHUNKS']} chunks of {m['REMAP_IPT']} images"
    assert 1 <= last < ipt, "the last chunk must be partial"
    assert chunks <= m["REMAP_CHUNKS"] and 2 * chunks <= 65535
    assert sc.tile_period_ok([ipt, chunks, m["REMAP_CHUNKS"]]), (ipt, chunks)
    runs = sc.REMAP_CAP_RUNS
    assert {(d, c) for d, c, _, _ in runs} >= {("u8", 1), ("f32", 3)}
    assert {b for _, _, b, _ in runs} == {"constant", "replicate"} and any(not both for _, _, _, both in runs)


def test_track_triples_take_a_second_trip_in_both_kernels(m):
    n, shape, model_shape = sc.TRACK_CAP_CASE
    (ag, astride, atrips), (sg, sstride, strips) = sc.track_triple_grids(n, m["TRACK_TRIPLES"])
    assert ag == sg == m["TRACK_TRIPLES"] and atrips >= 2 and strips >= 2, f"n = {n} no longer passes the triples cap"
    assert n - m["TRACK_TRIPLES"] >= 2, "more than one workgroup must take the second trip"
    assert sc.tile_period_ok([astride, sstride]), (astride, sstride)
    assert len(sc.TRACK_CAP_TRIPLES) == sc.TILE_PERIOD
    lost = [i for i, (_, _, misses) in enumerate(sc.TRACK_CAP_TRIPLES) if misses]
    assert lost and all(0 < i < sc.TILE_PERIOD - 1 for i in lost), "a lost triple between tracked ones: continue, then work"
    assert len(sc.TRACK_CAP_SCHEDULE) >= 2 and sum(k for _, k in sc.TRACK_CAP_SCHEDULE) >= 3
    operands = n * 4 * (shape[0] * shape[1] + 4 * model_shape[0] * model_shape[1])
    assert operands < 2 ** 31 and n * shape[0] * shape[1] <= 2 ** 30, "the call's frames and model views stay under 2 GB"


def test_lr_pack_halves_stride_and_wide_rows_leave_lds(m):
    seen_chunk_stride = False
    for n, dtype in sc.LR_PACK_CASES:
        eb = 4 if dtype == "f32" else 1
        g = sc.lr_pack_geometry(n * sc.C2_H, sc.C2_W, eb, m["LR_THREADS"], m["LR_PACK_ITEMS"], m["LR_BLOCKS"])
        assert g["blocks"] == m["LR_BLOCKS"], f"{n} {dtype}: the pack grid is below its cap"
        assert g["mirrored_trips"] >= 2, f"{n} {dtype}: the mirrored half does not stride"
        if dtype == "f32":
            assert g["chunk_trips"] >= 2 or g["element_trips"] >= 2, f"{n} {dtype}: the straight half does not stride"
        seen_chunk_stride |= g["chunk_trips"] >= 2
    assert seen_chunk_stride, "no case strides the straight half in 16-byte chunks"
    assert any(not sc.lr_pack_geometry(n * sc.C2_H, sc.C2_W, 4 if d == "f32" else 1, m["LR_THREADS"],
                                       m["LR_PACK_ITEMS"], m["LR_BLOCKS"])["vec"] for n, d in sc.LR_PACK_CASES)
    widths = [W for _, _, W, _, _ in sc.LR_WIDE_CASES]
    assert all(W > m["LR_LDS_W"] for W in widths), "a wide case fits the LDS row again"
    assert any(W % 4 == 0 for W in widths) and any(W % 4 != 0 for W in widths), "float4 rows and scalar rows"
