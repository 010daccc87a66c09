"""The production-size cases of tests/test_scale_gpu.py and the launch geometry each one must produce.

Every case below exists to push one kernel past a size at which it takes a different code path (a scan that gives each
thread several rows, a grid-stride loop that makes a second trip, a row loop that carries its base across chunks).  The
geometry functions restate the host-side launch arithmetic of the kernels (tu_reproject.hip, tu_tsdf.hip, tu_post.hip,
tu_stages.hip) with the kernel constants passed in, so that tests/test_scale_geometry_cpu.py can feed them the constants
it reads from the sources and fail loudly when a retuned constant leaves a case below its threshold.

The second half holds the cases of tests/test_launch_caps_gpu.py: the map entries (confidence, temporal filter, SGM,
weighted median, WLS, rectification, the LR pack and check, camera tracking) past the caps of their launchers' grids, with
many tiny maps tiled from TILE_PERIOD distinct ones."""
from __future__ import annotations

C2_H, C2_W = 375, 1242                        # KITTI C2 maps

# 1. reprojection: k_reproj_scan (one workgroup) over n*H rows
REPROJ_BATCH = (32, C2_H, C2_W)               # 12,000 rows
REPROJ_EDGES = [(1, 1024, 7), (5, 205, 9), (1, 2049, 3)]      # n*H = 1024, 1025, 2049: per = 1, 2, 3
REPROJ_MIN_KEPT = 0.5                         # every map of the batch keeps at least this share of its pixels

# 2. voxel downsampling of REPROJ_BATCH's padded output (cap = n*H*W): (voxel size, min_points, colours)
VOXEL_BATCH_RUNS = [(0.1, 1, True), (0.1, 3, True), (0.001, 1, True)]
VOXEL_WIDE_KEY_BITS = 57                      # the fine size's key must need all 8 radix passes of 8 bits

# 3. the flag scan's boundary: Lf = cap + 1 = 4,194,305 -> nb = 1,025 blocks, the first size with 2 sums per thread
VOXEL_SCAN_EDGE_CAP = 4_194_304
VOXEL_SCAN_EDGE_OFFSETS = [5_000, 900_000, 900_000, 2_000_000, 1_500_000, 3_800_000, VOXEL_SCAN_EDGE_CAP + 1_000]

# 4. one voxel of more than 15 k chunks of 64 points, among a few small ones
VOXEL_BIG_POINTS = 1_050_000
VOXEL_BIG_OTHERS = 2_000

# 5. TSDF integration and extraction of maps: nx = 512 (8 x-blocks of 64, two 256-wide scatter chunks), ny % 4 != 0
TSDF_MAPS_DIMS = (512, 37, 70)
TSDF_MAPS_N = (8, 1)                          # one call with 8 maps, then one with 1

# 6. TSDF extraction of states written directly
TSDF_STATE_DIMS = [(700, 64, 61),             # three chunks per row, the last one partial
                   (3, 2080, 2080),           # 4,326,400 rows: nb = 1,057, 2 sums per thread
                   (3, 2048, 2048)]           # 4,194,304 rows: nb = 1,024 exactly, 1 sum per thread

# 7. speckle filter and fill: n C2 maps past the grid-stride cap of k_spk_flatten / k_spk_finalize
SPECKLE_N = 6                                 # 2,794,500 pixels
SPECKLE_SIZES = (100, 12)

# 8. metrics: n maps of H x W, past the metrics kernel's block cap
METRICS_SHAPE = (4, 2160, 3840)

# ---- the map entries past their grid caps (tests/test_launch_caps_gpu.py) ----------------------------------------------
# Map i of every tiled case is distinct map i % TILE_PERIOD.  A grid-stride trip that lands on the wrong map, skips one or
# writes one twice changes a compared element as long as the period divides no loop stride (tile_period_ok) and the
# distinct expectations differ pairwise (asserted on the reference data by the GPU file).
TILE_PERIOD = 7

# 9. confidence and 10. temporal filter: (n, H, W) maps on grid.y, radius 1
CONF_CAP_SHAPE = (65538, 3, 5)
TEMPORAL_CAP_SHAPE = (65538, 3, 5)
TEMPORAL_FRAMES = 3
MAP_RADIUS = 1

# 11. SGM: the main case crosses the census cap (2 n images on grid.y, left and right images on second trips) and the
# cap of the right-view and selection kernels (one wave per pixel); the wide case (4 disparities per lane) crosses the
# census cap alone.  (n, H, W, min_disparity, num_disparities)
SGM_CAP_CASE = (65537, 5, 13, 1, 5)
SGM_CAP_WIDE_CASE = (32769, 1, 140, 1, 130)
SGM_CAP_OPTIONS = dict(paths=8, uniqueness=10, lr_max_diff=1.0)

# 12. weighted median: one tile per map
MEDIAN_CAP_SHAPE = (2 ** 20 + 5, 2, 3)
MEDIAN_CAP_RADIUS = 1
MEDIAN_CAP_SIGMAS = (40.0, 1.5)               # (sigma_color, sigma_space): neighbours weigh enough to move the median

# 13. WLS: rows of 2 past the rows cap (and n*W columns past the columns cap), then columns of 2 past both caps, then
# columns of 33 (several groups of loads in flight) whose single-pixel rows pass the rows cap alone
WLS_CAP_SHAPES = [(2 ** 26 + 3, 1, 2), (2 ** 26 + 3, 2, 1), (2 ** 20 * 64 // 33 + 1, 33, 1)]
WLS_CAP_ITERATIONS = 2

# 14. rectification: (n, H_in, W_in, H_out, W_out); runs are (dtype, channels, border mode, both views)
REMAP_CAP_CASE = (65541, 2, 3, 3, 2)
REMAP_CAP_RUNS = [("u8", 1, "constant", True), ("u8", 1, "replicate", True), ("f32", 3, "constant", True),
                  ("f32", 3, "replicate", True), ("u8", 1, "constant", False)]

# 15. the LR pack of an engine LR call: n C2 gray pairs, K = 2, D = 128.  n = 5: no part is 16-byte sized, both halves
# take their element loops; n = 8: the straight half of float32 frames strides in 16-byte chunks.
LR_PACK_CASES = [(5, "f32"), (5, "u8"), (8, "f32")]
LR_PACK_K, LR_PACK_D = 2, 128

# 16. the mirrored LR check on rows too wide for LDS: (n, H, W, K, D); W % 4 != 0 selects the scalar loop
LR_WIDE_CASES = [(1, 24, 4104, 2, 16), (1, 24, 4102, 2, 16)]

# 17. camera tracking: (n, frame shape, model view shape) triples on k_track_accum's grid.y and k_track_solve's grid.x;
# a schedule of two strides and three iterations, so that a lost triple's `continue` alternates with work on both loops'
# second trips, launch after launch.  Triple i is (model view, displacement, the model view misses) number i % 7.
TRACK_CAP_CASE = (65538, (11, 18), (12, 16))
TRACK_CAP_SCHEDULE = ((2, 1), (1, 2))
TRACK_CAP_MIN_INLIERS = 10                    # the 5 x 9 pixels of the stride-2 iteration hold more inliers in the twin
TRACK_CAP_TRIPLES = (("outside", 0, False), ("left", 1, False), ("outside", 2, False), ("left", 0, True),
                     ("outside", 1, False), ("left", 2, False), ("left", 0, False))


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def per_thread(items: int, threads: int) -> int:
    """Items per thread of a single-workgroup scan of `items` values over `threads` threads (k_reproj_scan,
    k_scan_top)."""
    return cdiv(items, threads)


def scan_blocks(L: int, scan_tile: int) -> int:
    """launch_scan: blocks of the three-launch scan of L values (tu_reproject.hip)."""
    return cdiv(L, scan_tile)


def voxel_scan_lengths(n: int, cap: int, vox_tile: int):
    """(Lc, Lf): the histogram array's and the flag array's scan lengths (vox_layout in smx_workspace.h)."""
    max_tiles = cdiv(cap, vox_tile) + n
    return max_tiles * 256, cap + 1


def voxel_bbox_blocks(cap: int, bbox_blocks: int) -> int:
    """k_vox_bbox's grid: one workgroup of 256 per 256 points, capped."""
    return min(cdiv(cap, 256), bbox_blocks)


def grid_stride_trips(items: int, blocks: int, threads: int) -> int:
    """Trips of the longest thread of a grid-stride loop over `items` with `blocks` x `threads`."""
    return cdiv(items, blocks * threads)


def tsdf_integrate_grid(dims, x_per_block: int, y_per_block: int):
    nx, ny, nz = dims
    return cdiv(nx, x_per_block), cdiv(ny, y_per_block), nz


def capped_blocks(items: int, per_block: int, cap: int) -> int:
    return min(cdiv(items, per_block), cap)


# ---- launch arithmetic of the map entries ------------------------------------------------------------------------------

def capped_grid(items: int, cap: int) -> int:
    """A grid dimension of one workgroup (or wave group) per item, capped: the kernel strides over the rest."""
    return min(items, cap)


def stride_trips(items: int, stride: int) -> int:
    """Trips of the first worker of a loop `for (i = id; i < items; i += stride)`."""
    return cdiv(items, stride)


def map_grid_y(n: int, cap: int):
    """(grid.y, stride, trips) of k_confidence / k_temporal: one map per blockIdx.y, m += gridDim.y."""
    g = capped_grid(n, cap)
    return g, g, stride_trips(n, g)


def sgm_census_grid(n: int, cap: int):
    """(grid.y, stride, trips, left images on a second trip, right images on a second trip) of k_sgm_census, whose
    images z < n are left frames and z >= n right frames."""
    g = capped_grid(2 * n, cap)
    second = range(g, 2 * n)
    return g, g, stride_trips(2 * n, g), sum(1 for z in second if z < n), sum(1 for z in second if z >= n)


def sgm_select_grid(n: int, H: int, W: int, threads: int, cap: int):
    """(grid.x, stride in pixels, trips) of k_sgm_right_wta / k_sgm_select: one wave per pixel, p += waves."""
    waves_per_block = threads // 64
    pixels = n * H * W
    g = capped_grid(cdiv(pixels, waves_per_block), cap)
    return g, g * waves_per_block, stride_trips(pixels, g * waves_per_block)


def median_grid(n: int, H: int, W: int, th: int, tw: int, cap: int):
    """(tiles per map, grid.x, stride, trips) of k_median: tile += gridDim.x."""
    per_map = cdiv(H, th) * cdiv(W, tw)
    g = capped_grid(n * per_map, cap)
    return per_map, g, g, stride_trips(n * per_map, g)


def wls_grids(n: int, H: int, W: int, lines: int, col_threads: int, cap: int):
    """((rows grid, stride in lines, trips), (columns grid, stride in columns, trips)) of k_wls_rows / k_wls_cols."""
    rg = capped_grid(cdiv(n * H, lines), cap)
    cg = capped_grid(cdiv(n * W, col_threads), cap)
    return (rg, rg * lines, stride_trips(n * H, rg * lines)), (cg, cg * col_threads, stride_trips(n * W, cg * col_threads))


def remap_chunks(n: int, ipt0: int, cap: int):
    """(images per thread, chunks, images of the last chunk) of launch_remap_pairs."""
    chunks = min(cdiv(n, ipt0), cap)
    ipt = cdiv(n, chunks)
    chunks = cdiv(n, ipt)
    return ipt, chunks, n - (chunks - 1) * ipt


def lr_pack_geometry(rows: int, W: int, elem_bytes: int, threads: int, items: int, cap: int):
    """launch_lr_pack on 16-byte aligned buffers: dict of blocks, stride, vec, the straight half's (16-byte chunks and)
    elements and the trips of its loops, the mirrored half's items and trips."""
    half = rows * W
    vec = (half * elem_bytes) % 16 == 0
    straight = cdiv(half * elem_bytes, 16)
    mirrored = rows * cdiv(W, items)
    blocks = min(cdiv(max(straight, mirrored), threads), cap)
    stride = blocks * threads
    chunks = half * elem_bytes // 16 if vec else 0
    tail = half - chunks * (16 // elem_bytes)
    return dict(blocks=blocks, stride=stride, vec=vec, chunk_trips=stride_trips(chunks, stride),
                element_trips=stride_trips(tail, stride), mirrored_trips=stride_trips(mirrored, stride))


def track_triple_grids(n: int, cap: int):
    """((grid.y, stride, trips) of k_track_accum: f += gridDim.y, (grid.x, stride, trips) of k_track_solve: f += gridDim.x)."""
    g = capped_grid(n, cap)
    return (g, g, stride_trips(n, g)), (g, g, stride_trips(n, g))


def tile_period_ok(strides) -> bool:
    """TILE_PERIOD divides none of the loop strides (in maps, tiles, images, lines, pixels or chunks)."""
    return all(s % TILE_PERIOD != 0 for s in strides)
