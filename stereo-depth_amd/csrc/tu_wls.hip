// tu_wls.hip -- image-guided weighted least squares filter (k_wls.h).
#include <string.h>

#include "k_wls.h"
#include "smx_launch.h"
#include "smx_workspace.h"

namespace smx {

namespace {

unsigned grid_of(size_t lines, int per_block) {
    const size_t blocks = (lines + per_block - 1) / per_block;
    return (unsigned)(blocks < ((size_t)1 << 20) ? blocks : ((size_t)1 << 20));      // grid-stride beyond
}

}  // namespace

void launch_wls(int n, int H, int W, const float *in, const float *conf, const float *guide, float *out, int iterations,
                const float *lambdas, const float *range, float min_weight, float invalid, void *workspace,
                hipStream_t s) {
    WlsTable tab;
    memcpy(tab.range, range, sizeof tab.range);
    const WlsLayout l = wls_layout(n, H, W);
    WlsArgs a;
    a.in = in, a.conf = conf, a.guide = guide;
    a.U = ws_at<float>(workspace, l.U), a.V = ws_at<float>(workspace, l.V), a.E = ws_at<float>(workspace, l.E);
    a.out = out;
    a.n = n, a.H = H, a.W = W;
    a.min_weight = min_weight, a.invalid = invalid;
    const unsigned rows_grid = grid_of((size_t)n * H, WLS_LINES);
    const unsigned cols_grid = grid_of((size_t)n * W, WLS_COL_THREADS);
    for (int t = 0; t < iterations; ++t) {
        a.lambda = lambdas[t];
        a.first = t == 0;
        a.last = t == iterations - 1;
        hipLaunchKernelGGL(k_wls_rows, dim3(rows_grid), dim3(WLS_ROW_THREADS), 0, s, a, tab);
        hipLaunchKernelGGL(k_wls_cols, dim3(cols_grid), dim3(WLS_COL_THREADS), 0, s, a, tab);
    }
}

}  // namespace smx
