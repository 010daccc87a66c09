// tu_tsdf_merge.hip -- one volume's state merged into another in place (k_tsdf_merge.h): one launch over the rows of the
// overlap of the source's region with the destination grid, none where they do not meet.
#include "k_tsdf_merge.h"
#include "smx_launch.h"

namespace smx {

void launch_tsdf_merge(int nx, int ny, int nz, float *tsdf, float *weight, uint8_t *color, int sx, int sy, int sz,
                       const float *src_tsdf, const float *src_weight, const uint8_t *src_color, int x0, int y0, int z0,
                       int rx, int ry, int rz, int cx, int cy, int cz, int mode, float max_weight, hipStream_t s) {
    (void)sz;
    // the region in destination voxels, clipped to the grid: |x0| <= 8192 and dims <= 4096 keep every sum in an int
    const int n[3] = {nx, ny, nz}, o[3] = {x0, y0, z0}, r[3] = {rx, ry, rz}, c[3] = {cx, cy, cz};
    int lo[3], len[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = o[a] + r[a] > 0 ? o[a] + r[a] : 0;
        const int hi = o[a] + r[a] + c[a] < n[a] ? o[a] + r[a] + c[a] : n[a];
        if (hi <= lo[a]) return;                                      // no pair: nothing is launched
        len[a] = hi - lo[a];
    }
    TsdfMergeArgs a;
    a.nx = nx, a.ny = ny, a.sx = sx, a.sy = sy;
    a.dx = lo[0], a.dy = lo[1], a.dz = lo[2];
    a.ox = len[0], a.oy = len[1], a.oz = len[2];
    a.x0 = x0, a.y0 = y0, a.z0 = z0;
    a.mode = mode, a.max_weight = max_weight;
    a.dst[0] = (unsigned *)tsdf, a.dst[1] = (unsigned *)weight, a.dst[2] = (unsigned *)color;
    a.src[0] = (const unsigned *)src_tsdf, a.src[1] = (const unsigned *)src_weight, a.src[2] = (const unsigned *)src_color;
    const long rows = (long)a.oy * a.oz;                              // <= 2^24: a wave per row, at most 2^22 workgroups
    hipLaunchKernelGGL(k_tsdf_merge, dim3((unsigned)((rows + MRG_WAVES - 1) / MRG_WAVES)), dim3(64 * MRG_WAVES), 0, s, a);
}

}  // namespace smx
