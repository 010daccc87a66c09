// tu_temporal.hip -- motion-gated temporal filter of disparity-map streams (k_temporal.h).
#include "k_temporal.h"
#include "smx_launch.h"

namespace smx {

void launch_temporal(int n, int H, int W, const float *disp, const float *conf, const float *guide,
                     const float *prev_guide, float *state_disp, float *state_weight, float *guide_out, float *out,
                     int radius, float threshold, float decay, float max_diff, float max_weight, float min_weight,
                     float invalid, hipStream_t s) {
    TemporalArgs a;
    a.disp = disp, a.conf = conf, a.guide = guide, a.prev = prev_guide;
    a.state_disp = state_disp, a.state_weight = state_weight, a.guide_out = guide_out, a.out = out;
    a.n = n, a.H = H, a.W = W, a.radius = radius;
    a.tiles_x = (W + TEMP_TW - 1) / TEMP_TW;
    a.threshold = threshold, a.decay = decay, a.max_diff = max_diff, a.max_weight = max_weight;
    a.min_weight = min_weight, a.invalid = invalid;
    const int tiles_y = (H + TEMP_TH - 1) / TEMP_TH;
    const unsigned maps = (unsigned)(n < 65535 ? n : 65535);                       // grid-stride beyond
    const size_t lds = temporal_lds_floats(radius) * sizeof(float);
    hipLaunchKernelGGL(k_temporal, dim3((unsigned)(a.tiles_x * tiles_y), maps), dim3(TEMP_THREADS), lds, s, a);
}

}  // namespace smx
