"""The production-size cases of tests/test_scale_gpu.py and the launch geometry each one must produce.

Every case below exists to push one kernel past a size at which it takes a different code path (a scan that gives each
thread several rows, a grid-stride loop that makes a second trip, a row loop that carries its base across chunks).  The
geometry functions restate the host-side launch arithmetic of the kernels (tu_reproject.hip, tu_tsdf.hip, tu_post.hip,
tu_stages.hip) with the kernel constants passed in, so that tests/test_scale_geometry_cpu.py can feed them the constants
it reads from the sources and fail loudly when a retuned constant leaves a case below its threshold."""
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
    """(Lc, Lf): the histogram array's and the flag array's scan lengths (vox_layout in tu_reproject.hip)."""
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
