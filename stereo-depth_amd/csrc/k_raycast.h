// k_raycast.h -- views of a TSDF volume by ray casting (smx_tsdf_raycast).  The rule, bit for bit, is in
// include/stereo_mi355x.h; tests/raycast_ref.py restates it in NumPy, without the skips.
//
//   k_raycast_bricks  one byte per brick of 8 x 8 x 8 voxels: RC_ANY iff a voxel of the brick has weight >= min_weight,
//                     RC_FREE iff all of them have, with tsdf == 1.0f exactly (measured free space).  One workgroup per
//                     (brick row y, brick row z): a thread keeps one x and walks the 64 voxel rows of the brick row, so
//                     every load is a coalesced row segment; ballots join the 8 lanes of a brick and the first of them
//                     stores the byte.  No atomics, no LDS.
//   k_raycast_free    a brick keeps RC_FREE only if its upper neighbours are free too: then every cell whose first
//                     corner lies in the brick has eight measured corners of tsdf 1.
//   k_raycast_march   one thread per pixel, RC_TW x RC_TH pixels per wave (neighbouring rays share voxel rows), the view
//                     in blockIdx.z so the pose is wave-uniform.  A sample outside the box, or whose first corner lies
//                     in an empty brick, is invalid without a load from the volume; one whose first corner lies in a
//                     free brick is valid with T = 1 exactly (every lerp is 1 + (1 - 1)*t), again without a load.  In
//                     all three cases the ray then tries to jump.
//
// Why a jump is exact: every step from the sample index m to floorf(g_a) is a monotone float32 function (a rounded
// product with a factor of fixed sign, rounded sums with a constant, a division by s > 0, floorf), so along one ray
// f_a(m) is monotone in m on each axis.  If samples m and m + k have their first corner in the same brick, or lie beyond
// the same face of the box, so do all samples between them, and all of them are invalid (or, in a free brick, all valid
// with T = 1: none of them ends the ray, and the last leaves "valid, T = 1" behind).  The length k of a jump is
// only an estimate in float arithmetic; sample m + k is then evaluated by the rule and the jump is taken iff it
// confirms.  A sample beyond a face that the ray moves away from (dw_a >= 0 past the upper face, dw_a <= 0 before the
// lower) ends the ray: every later sample is beyond that face too.
#pragma once
#include "k_raycast_rule.h"

#ifndef SMX_RAYCAST_TILE_W
#define SMX_RAYCAST_TILE_W 8           // pixels of a wave along x: 8 (8 x 8 tiles) or 64 (64 x 1); DESIGN.md has both times
#endif

namespace smx {

constexpr int RC_TW = SMX_RAYCAST_TILE_W, RC_TH = 64 / RC_TW;   // a wave's pixel tile
constexpr int RC_BW = RC_TW == 8 ? 4 : 1, RC_BH = 4 / RC_BW;    // a workgroup's 4 waves: 32 x 8 or 64 x 4 pixels
static_assert(RC_TW == 8 || RC_TW == 64, "SMX_RAYCAST_TILE_W must be 8 or 64");

// grid (by, bz), 256 threads: flags[brick] = RC_ANY | RC_FREE of the brick's own voxels
__global__ __launch_bounds__(256) void k_raycast_bricks(const RaycastArgs a) {
    const int bj = blockIdx.x, bk = blockIdx.y;
    const int y0 = bj * 8, z0 = bk * 8;
    const int xend = a.bx * 8;                                       // whole waves reach the ballots
    for (int x = threadIdx.x; x < xend; x += 256) {
        bool any = false, all = true;                                 // a column past the volume has no voxel: free
        if (x < a.nx) {
#pragma unroll
            for (int dz = 0; dz < 8; ++dz)
#pragma unroll
                for (int dy = 0; dy < 8; ++dy) {                      // rows past the volume repeat its last row
                    const int y = min(y0 + dy, a.ny - 1), z = min(z0 + dz, a.nz - 1);
                    const bool ok = a.weight[voxel_index(z, y, x, a.ny, a.nx)] >= a.min_weight;
                    any |= ok, all &= ok;
                }
            if (all) {                                                // the tsdf is read only under measured columns
#pragma unroll
                for (int dz = 0; dz < 8; ++dz)
#pragma unroll
                    for (int dy = 0; dy < 8; ++dy) {
                        const int y = min(y0 + dy, a.ny - 1), z = min(z0 + dz, a.nz - 1);
                        all &= a.tsdf[voxel_index(z, y, x, a.ny, a.nx)] == 1.0f;
                    }
            }
        }
        const unsigned long long b_any = __ballot(any), b_all = __ballot(all);
        const int lane = threadIdx.x & 63;
        if ((lane & 7) == 0)
            a.flags[((size_t)bk * a.by + bj) * a.bx + (x >> 3)] =
                (uint8_t)((((b_any >> lane) & 0xffull) != 0 ? RC_ANY : 0) | (((b_all >> lane) & 0xffull) == 0xffull ? RC_FREE : 0));
    }
}

// one thread per brick: occ[brick] = its RC_ANY, and RC_FREE iff the brick and its existing upper neighbours (the voxels a
// cell with its first corner in the brick can touch) are all free
__global__ __launch_bounds__(256) void k_raycast_free(const RaycastArgs a) {
    const int total = a.bx * a.by * a.bz;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= total) return;
    const int i = b % a.bx, j = (b / a.bx) % a.by, k = b / (a.bx * a.by);
    unsigned fl = a.flags[b];
    unsigned free = fl & RC_FREE;
#pragma unroll
    for (int c = 1; c < 8; ++c) {
        const int ni = i + (c & 1), nj = j + ((c >> 1) & 1), nk = k + (c >> 2);
        if (ni < a.bx && nj < a.by && nk < a.bz) free &= a.flags[((size_t)nk * a.by + nj) * a.bx + ni];
    }
    a.occ[b] = (uint8_t)((fl & RC_ANY) | (free & RC_FREE));
}

// grid (ceil(W / (RC_TW*RC_BW)), ceil(H / (RC_TH*RC_BH)), min(n, 65535)), 256 threads; a grid-stride loop over the views
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_raycast_march(const RaycastArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int px = (blockIdx.x * RC_BW + (wv % RC_BW)) * RC_TW + (lane % RC_TW);
    const int py = (blockIdx.y * RC_BH + (wv / RC_BW)) * RC_TH + (lane / RC_TW);
    if (px >= a.W || py >= a.H) return;
    for (int view = blockIdx.z; view < a.n; view += gridDim.z) rc_pixel(a, px, py, view);
}

}  // namespace smx
