// tu_confidence.hip -- per-pixel confidence of a disparity map (k_confidence.h).
#include "k_confidence.h"
#include "smx_launch.h"

namespace smx {

void launch_confidence(int n, int H, int W, const float *left, const float *right, const float *guide, int radius,
                       float lr_scale, float texture_scale, float invalid, float *out, hipStream_t s) {
    ConfArgs a;
    a.left = left, a.right = right, a.guide = guide, a.out = out;
    a.n = n, a.H = H, a.W = W;
    a.radius = guide ? radius : 0;
    a.tiles_x = (W + CONF_TW - 1) / CONF_TW;
    a.lr_scale = lr_scale, a.texture_scale = texture_scale, a.invalid = invalid;
    const int tiles_y = (H + CONF_TH - 1) / CONF_TH;
    const unsigned maps = (unsigned)(n < 65535 ? n : 65535);                       // grid-stride beyond
    const size_t lds = guide ? conf_lds_floats(radius) * sizeof(float) : 0;
    hipLaunchKernelGGL(k_confidence, dim3((unsigned)(a.tiles_x * tiles_y), maps), dim3(CONF_THREADS), lds, s, a);
}

}  // namespace smx
