// tu_synthesis.hip -- right-view synthesis head (k_synthesis.h): the rescaled view and its training form.
#include "k_synthesis.h"
#include "smx_launch.h"

namespace smx {

template <bool RESCALE>
static void launch_head(int n, int C, bool f32, int D, int h, int w, int S, const float *prob, const void *left, float *out,
                        hipStream_t s) {
    SynArgs a;
    a.prob = prob, a.left = left, a.out = out;
    a.n = n, a.D = D, a.h = h, a.w = w, a.S = S, a.H = h * S, a.W = w * S;
    a.tiles_x = (a.W + SYN_TW - 1) / SYN_TW;
    a.dc = synthesis_chunk(C, D, S, h, w);
    const int tiles_y = (a.H + SYN_TH - 1) / SYN_TH;
    const dim3 grid((unsigned)(a.tiles_x * tiles_y), (unsigned)(n < 65535 ? n : 65535));         // grid-stride beyond
    const size_t lds = syn_lds_floats(C, a.dc, S, h, w) * sizeof(float);
    if (C == 3) {
        if (f32) hipLaunchKernelGGL((k_synthesis<3, true, RESCALE>), grid, dim3(SYN_THREADS), lds, s, a);
        else hipLaunchKernelGGL((k_synthesis<3, false, RESCALE>), grid, dim3(SYN_THREADS), lds, s, a);
    } else {
        if (f32) hipLaunchKernelGGL((k_synthesis<1, true, RESCALE>), grid, dim3(SYN_THREADS), lds, s, a);
        else hipLaunchKernelGGL((k_synthesis<1, false, RESCALE>), grid, dim3(SYN_THREADS), lds, s, a);
    }
}

void launch_synthesis(int n, int C, bool f32, int D, int h, int w, int S, const float *prob, const void *left, float *out,
                      hipStream_t s) {
    launch_head<true>(n, C, f32, D, h, w, S, prob, left, out, s);
}

void launch_synthesis_view(int n, int C, bool f32, int D, int h, int w, int S, const float *prob, const void *left,
                           float *view, hipStream_t s) {
    launch_head<false>(n, C, f32, D, h, w, S, prob, left, view, s);
}

}  // namespace smx
