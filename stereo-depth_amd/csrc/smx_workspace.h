// smx_workspace.h -- the layout of every caller-supplied workspace, written once.  A size query (smx_maps.hip) reads
// `total`, the launcher (tu_*.hip) carves its pointers from the parts with ws_at(), and neither does arithmetic of its
// own, so the two cannot disagree.  Host-only code without a HIP include: tests/workspace_layout_harness.cpp sweeps it
// on the CPU.  Every part starts on a multiple of 256 bytes (include/stereo_mi355x.h: conventions); the layouts are
// private to the library and nothing in a workspace survives a call.
#pragma once
#include <stddef.h>

namespace smx {

struct WsPart {
    size_t offset, bytes;
};

// Hands out the parts of one workspace in order, each rounded up to 256 bytes.
struct WsCursor {
    size_t at = 0;
    WsPart take(size_t bytes) {
        const WsPart p{at, bytes};
        at += (bytes + 255) & ~(size_t)255;
        return p;
    }
};

template <class T> inline T *ws_at(void *workspace, const WsPart &p) { return (T *)((char *)workspace + p.offset); }

// ---- constants the layouts share with the kernels of k_reproject.h, and SGM's pitch rule for tu_sgm.hip --------------
constexpr int SCAN_ITEMS = 16;             // exclusive scan of an int array: values per thread,
constexpr int SCAN_TILE = 256 * SCAN_ITEMS;   // ... per workgroup
constexpr int VOX_TILE = 4096;             // voxel downsampling: points per radix tile (one workgroup of 256 threads)
constexpr int VM_COUNT = 16;               // ... ints of device-side state (meta[], indexed by k_reproject.h's VM_*)

inline size_t scan_block_sums(long L) { return (size_t)((L + SCAN_TILE - 1) / SCAN_TILE); }   // ints of scan scratch

// SGM: disparities per lane of a wave, and the disparity count rounded up to it (the pitch of S)
inline int sgm_dpl(int D) { return D <= 64 ? 1 : D <= 128 ? 2 : 4; }
inline int sgm_dp(int D) { const int k = sgm_dpl(D); return (D + k - 1) / k * k; }

// ---- speckle filter and hole fill: labels int[P] | sizes int[P] | row flags int[n H], P = n H W ---------------------
struct PostLayout {
    WsPart label, size, flags;
    size_t total;
};
inline PostLayout post_layout(int n, int H, int W) {
    const size_t px = (size_t)n * H * W;
    WsCursor c;                                            // a braced list is evaluated left to right
    return PostLayout{c.take(px * sizeof(int)), c.take(px * sizeof(int)), c.take((size_t)n * H * sizeof(int)), c.at};
}

// ---- WLS: the planes U | V | E, each f32[n][H][W].  The forward sweeps write y_U over U, y_V over V and e to E; the
// back sweeps read them.
struct WlsLayout {
    WsPart U, V, E;
    size_t total;
};
inline WlsLayout wls_layout(int n, int H, int W) {
    const size_t plane = (size_t)n * H * W * sizeof(float);
    WsCursor c;
    return WlsLayout{c.take(plane), c.take(plane), c.take(plane), c.at};
}

// ---- SGM: left census u64[P] | right census u64[P] | S u16[P][Dp] | iR i16[P] ---------------------------------------
struct SgmLayout {
    int Dp;
    WsPart cen_l, cen_r, S, iR;
    size_t total;
};
inline SgmLayout sgm_layout(int n, int H, int W, int D) {
    const size_t P = (size_t)n * H * W;
    const int Dp = sgm_dp(D);
    WsCursor c;
    return SgmLayout{Dp, c.take(P * 8), c.take(P * 8), c.take(P * Dp * 2), c.take(P * 2), c.at};
}

// ---- reprojection: one part, row counts int[n H] and row offsets int[n H] back to back ------------------------------
struct ReprojectLayout {
    WsPart rows;
    size_t total;
};
inline ReprojectLayout reproject_layout(int n, int H) {
    WsCursor c;
    return ReprojectLayout{c.take(2 * (size_t)n * H * sizeof(int)), c.at};
}

// ---- voxel downsampling: two key and two value buffers of the radix sort, the tiles' histograms and their scan, the
// voxel heads' flags / positions / counts, the scan's block sums, per-map offsets and tile bases, meta[] --------------
struct VoxLayout {
    WsPart keys, vals, counts, counts_scan, flag, pos, vcnt, block_sums, off, tile_base, meta;
    size_t total;
    long max_tiles, Lc, Lf;
    int nb;
};
inline VoxLayout vox_layout(int n, int cap) {
    VoxLayout l;
    l.max_tiles = ((long)cap + VOX_TILE - 1) / VOX_TILE + n;
    l.Lc = l.max_tiles * 256;
    l.Lf = (long)cap + 1;
    l.nb = (int)(((l.Lc > l.Lf ? l.Lc : l.Lf) + SCAN_TILE - 1) / SCAN_TILE);
    WsCursor c;
    l.keys = c.take(2 * (size_t)cap * sizeof(unsigned long long));
    l.vals = c.take(2 * (size_t)cap * sizeof(int));
    l.counts = c.take((size_t)l.Lc * sizeof(int));
    l.counts_scan = c.take((size_t)l.Lc * sizeof(int));
    l.flag = c.take((size_t)l.Lf * sizeof(int));
    l.pos = c.take((size_t)l.Lf * sizeof(int));
    l.vcnt = c.take((size_t)l.Lf * sizeof(int));
    l.block_sums = c.take((size_t)l.nb * sizeof(int));
    l.off = c.take(((size_t)n + 1) * sizeof(int));
    l.tile_base = c.take(((size_t)n + 1) * sizeof(int));
    l.meta = c.take(VM_COUNT * sizeof(int));
    l.total = c.at;
    return l;
}

// ---- projection of point clouds: one 64-bit key per output pixel | the clamped offsets int[n + 1] -----------------------
struct ProjectLayout {
    WsPart keys, off;
    size_t total;
};
inline ProjectLayout project_layout(int n, int H, int W) {
    WsCursor c;
    return ProjectLayout{c.take((size_t)n * H * W * sizeof(unsigned long long)), c.take(((size_t)n + 1) * sizeof(int)), c.at};
}

// ---- TSDF integrate: measurements float2[P] | colour words u32[P] ---------------------------------------------------
struct TsdfIntegrateLayout {
    WsPart meas, pcol;
    size_t total;
};
inline TsdfIntegrateLayout tsdf_integrate_layout(int n, int H, int W) {
    const size_t px = (size_t)n * H * W;
    WsCursor c;
    return TsdfIntegrateLayout{c.take(px * 2 * sizeof(float)), c.take(px * sizeof(unsigned)), c.at};
}

// ---- TSDF extract points: counts int[rows] | offsets int[rows] | the scan's block sums, rows = ny nz -----------------
struct TsdfExtractLayout {
    WsPart row_count, row_offset, block_sums;
    size_t total;
};
inline TsdfExtractLayout tsdf_extract_layout(int ny, int nz) {
    const long rows = (long)ny * nz;
    WsCursor c;
    return TsdfExtractLayout{c.take((size_t)rows * sizeof(int)), c.take((size_t)rows * sizeof(int)),
                             c.take(scan_block_sums(rows) * sizeof(int)), c.at};
}

// ---- TSDF extract triangles: one byte per voxel | one word per 64-voxel chunk of a row | three counts and three
// offsets per row | the scan's block sums ------------------------------------------------------------------------------
struct MeshLayout {
    int nch;
    WsPart flags, chunk_first, counts, offsets, block_sums;
    size_t total;
};
inline MeshLayout mesh_layout(int nx, int ny, int nz) {
    const size_t rows = (size_t)ny * nz;
    const int nch = (nx + 63) / 64;
    WsCursor c;
    return MeshLayout{nch, c.take(rows * nx), c.take(rows * nch * sizeof(unsigned)), c.take(3 * rows * sizeof(int)),
                      c.take(3 * rows * sizeof(int)), c.take(scan_block_sums(3 * (long)rows) * sizeof(int)), c.at};
}

// ---- TSDF ray cast: two bytes per brick of 8 x 8 x 8 voxels, flags u8[bz][by][bx] | occ u8[bz][by][bx], b_a = ceil(n_a / 8)
struct RaycastLayout {
    int bx, by, bz;
    WsPart flags, occ;
    size_t total;
};
inline RaycastLayout raycast_layout(int nx, int ny, int nz) {
    const int bx = (nx + 7) / 8, by = (ny + 7) / 8, bz = (nz + 7) / 8;
    WsCursor c;
    return RaycastLayout{bx, by, bz, c.take((size_t)bx * by * bz), c.take((size_t)bx * by * bz), c.at};
}

// ---- camera tracking: one state record of 32 words per triple | the sums of every group of four tiles of the selected
// grid, double[n][groups at stride 1][TRK_SLOTS].  The constants are shared with k_track_body.h and fix the order of the sums.
#ifndef SMX_TRK_ROWS                           // tuning experiments only (build.py: SMX_EXTRA_FLAGS): another value sums in
#define SMX_TRK_ROWS 4                         // another order than the header states
#endif
constexpr int TRK_COLS = 64, TRK_ROWS = SMX_TRK_ROWS;   // a tile of the selected grid: one wave, one lane per column
constexpr int TRK_WAVES = 4;                   // tiles per workgroup, consecutive in row-major order
constexpr int TRK_TERMS = 30;                  // the sums of the header ...
constexpr int TRK_SLOTS = 32;                  // ... then the accepted pixels, and one unused slot
constexpr int TRK_MAX_TILES = 32768;           // of a frame at stride 1 (the combine kernel's stack: k_track_body.h)
struct TrackGrid {
    int ws, hs, tx, ty, tiles, groups;         // selected columns and rows; tiles across, down, in all; groups of 4 tiles
};
inline TrackGrid track_grid(int H, int W, int stride) {
    TrackGrid g;
    g.ws = (W + stride - 1) / stride, g.hs = (H + stride - 1) / stride;
    g.tx = (g.ws + TRK_COLS - 1) / TRK_COLS, g.ty = (g.hs + TRK_ROWS - 1) / TRK_ROWS;
    g.tiles = g.tx * g.ty, g.groups = (g.tiles + TRK_WAVES - 1) / TRK_WAVES;
    return g;
}
struct TrackLayout {
    int groups;                                // per triple, at stride 1 (no stride has more)
    WsPart state, partial;
    size_t total;
};
inline TrackLayout track_layout(int n, int H, int W, int slots = TRK_SLOTS) {
    const int groups = track_grid(H, W, 1).groups;
    WsCursor c;
    return TrackLayout{groups, c.take((size_t)n * 32 * sizeof(int)), c.take((size_t)n * groups * slots * sizeof(double)),
                       c.at};
}

// ---- camera tracking with the photometric term: the same state record | the sums of every group of four tiles,
// double[n][groups at stride 1][TRKP_SLOTS].  The grid is track_grid's; the slots are the geometric rule's 0..30 as they
// are, then the three photometric sums (k_track_photo_rule.h).
constexpr int TRKP_TERMS = TRK_TERMS + 3;      // the sums of the header: thirty of the joint system, three photometric
constexpr int TRKP_SLOTS = TRK_TERMS + 4;      // the thirty, the accepted pixels, the three
inline TrackLayout track_photo_layout(int n, int H, int W) { return track_layout(n, H, W, TRKP_SLOTS); }

// ---- intensity pyramids (not a workspace: the caller's buffer): level 0 [n][H][W] | level 1 [n][H_1][W_1] | ..., float32,
// a level's dimension ceil(d / 2) of the one before it, which is the selected grid of stride 2^level.
constexpr int PYR_MAX_LEVELS = 8;
struct PyramidLevel {
    size_t offset;                             // in floats
    int H, W;
};
// level == levels gives the pyramid's size
inline PyramidLevel pyramid_level(int n, int H, int W, int level) {
    PyramidLevel l{0, H, W};
    for (int k = 0; k < level; ++k) {
        l.offset += (size_t)n * l.H * l.W;
        l.H = (l.H + 1) / 2, l.W = (l.W + 1) / 2;
    }
    return l;
}

}  // namespace smx
