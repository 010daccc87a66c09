// tu_pyramid.hip -- intensity pyramids (k_pyramid.h): one launch for level 0, then one per level, each reading the level
// before it from the pyramid itself.
#include "k_pyramid.h"

namespace smx {

void launch_intensity_pyramid(int n, int H, int W, int levels, const float *plane, const float *mask_depth, float *pyramid,
                              hipStream_t s) {
    const size_t total = (size_t)n * H * W, blocks = (total + 255) / 256;
    hipLaunchKernelGGL(k_pyramid_base, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, plane, mask_depth,
                       pyramid, total);
    for (int l = 1; l < levels; ++l) {
        const PyramidLevel from = pyramid_level(n, H, W, l - 1), to = pyramid_level(n, H, W, l);
        hipLaunchKernelGGL(k_pyramid_reduce,
                           dim3((unsigned)((to.W + PYR_TW - 1) / PYR_TW), (unsigned)((to.H + PYR_TH - 1) / PYR_TH),
                                (unsigned)(n < 65535 ? n : 65535)),
                           dim3(256), 0, s, pyramid + from.offset, pyramid + to.offset, n, from.H, from.W, to.H, to.W);
    }
}

}  // namespace smx
