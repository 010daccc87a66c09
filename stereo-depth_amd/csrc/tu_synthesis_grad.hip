// tu_synthesis_grad.hip -- backward of the right-view synthesis head (k_synthesis_grad.h).
#include "k_synthesis_grad.h"
#include "smx_launch.h"

namespace smx {

template <int NT, int U, int SC>
static void launch_grad(const SynGradArgs &a, int C, bool f32, dim3 grid, int threads, size_t lds, hipStream_t s) {
    if (C == 3) {
        if (f32) hipLaunchKernelGGL((k_synthesis_grad<3, true, NT, U, SC>), grid, dim3(threads), lds, s, a);
        else hipLaunchKernelGGL((k_synthesis_grad<3, false, NT, U, SC>), grid, dim3(threads), lds, s, a);
    } else {
        if (f32) hipLaunchKernelGGL((k_synthesis_grad<1, true, NT, U, SC>), grid, dim3(threads), lds, s, a);
        else hipLaunchKernelGGL((k_synthesis_grad<1, false, NT, U, SC>), grid, dim3(threads), lds, s, a);
    }
}

void launch_synthesis_grad(int n, int C, bool f32, int D, int h, int w, int S, const float *grad_view, const void *left,
                           float *grad_prob, hipStream_t s) {
    const SynGradShape sh = syn_grad_shape(S);
    const int rows = 1 << sh.rows_log2, tj = 1 << sh.tj_log2;
    SynGradArgs a;
    a.g = grad_view, a.left = left, a.out = grad_prob;
    a.n = n, a.D = D, a.h = h, a.w = w, a.S = S, a.H = h * S, a.W = w * S;
    a.rows_log2 = sh.rows_log2, a.tj_log2 = sh.tj_log2;
    a.ti = rows / S - 1;
    a.tiles_j = (w + tj - 1) / tj;
    a.dc = synthesis_grad_chunk(C, D, S);
    a.rs = syg_row_floats(S, tj, sh.NT, a.dc);
    const int tiles_i = (h + a.ti - 1) / a.ti;                 // at most 1058 x 4096 tiles (S = 1)
    const dim3 grid((unsigned)(tiles_i * a.tiles_j), (unsigned)(n < 65535 ? n : 65535));          // grid-stride beyond
    const size_t lds = syg_lds_floats(C, S, rows, tj, sh.NT, sh.U, a.dc) * sizeof(float);
    if (S == 4) launch_grad<10, 4, 4>(a, C, f32, grid, rows * tj, lds, s);                         // the reference's scale
    else if (sh.NT == 10) launch_grad<10, 4, 0>(a, C, f32, grid, rows * tj, lds, s);
    else if (sh.NT == 20) launch_grad<20, 2, 0>(a, C, f32, grid, rows * tj, lds, s);
    else launch_grad<40, 1, 0>(a, C, f32, grid, rows * tj, lds, s);
}

}  // namespace smx
