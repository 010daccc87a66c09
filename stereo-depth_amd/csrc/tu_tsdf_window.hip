// tu_tsdf_window.hip -- the windowed copy of a TSDF volume's state (k_tsdf_window.h): one launch for the three arrays.
#include "k_tsdf_window.h"
#include "smx_launch.h"

namespace smx {

void launch_tsdf_window(int nx, int ny, int nz, const float *tsdf, const float *weight, const uint8_t *color, int x0,
                        int y0, int z0, int bx, int by, int bz, float *tsdf_out, float *weight_out, uint8_t *color_out,
                        hipStream_t s) {
    TsdfWindowArgs a;
    a.nx = nx, a.ny = ny, a.nz = nz;
    a.x0 = x0, a.y0 = y0, a.z0 = z0;
    a.bx = bx, a.by = by, a.bz = bz;
    a.src[0] = (const unsigned *)tsdf, a.src[1] = (const unsigned *)weight, a.src[2] = (const unsigned *)color;
    a.dst[0] = (unsigned *)tsdf_out, a.dst[1] = (unsigned *)weight_out, a.dst[2] = (unsigned *)color_out;
    const long rows = (long)by * bz;                                  // <= 2^24: a wave per row, at most 2^22 workgroups
    hipLaunchKernelGGL(k_tsdf_window, dim3((unsigned)((rows + WIN_WAVES - 1) / WIN_WAVES)), dim3(64 * WIN_WAVES), 0, s, a);
}

}  // namespace smx
