// tu_wls.hip -- image-guided weighted least squares filter (k_wls.h).
#include <string.h>

#include "k_wls.h"
#include "smx_launch.h"

namespace smx {

namespace {

constexpr size_t WLS_ALIGN = 256;
size_t wls_plane_bytes(int n, int H, int W) {
    return ((size_t)n * H * W * sizeof(float) + WLS_ALIGN - 1) / WLS_ALIGN * WLS_ALIGN;
}

unsigned grid_of(size_t lines, int per_block) {
    const size_t blocks = (lines + per_block - 1) / per_block;
    return (unsigned)(blocks < ((size_t)1 << 20) ? blocks : ((size_t)1 << 20));      // grid-stride beyond
}

}  // namespace

// Workspace layout (include/stereo_mi355x.h: smx_wls_workspace_bytes): the planes U | V | E, each [n][H][W] f32
// rounded up to 256 bytes.  The forward sweeps write y_U over U, y_V over V and e to E; the back sweeps read them.
size_t wls_workspace_bytes(int n, int H, int W) { return 3 * wls_plane_bytes(n, H, W); }

void launch_wls(int n, int H, int W, const float *in, const float *conf, const float *guide, float *out, int iterations,
                const float *lambdas, const float *range, float min_weight, float invalid, void *workspace,
                hipStream_t s) {
    WlsTable tab;
    memcpy(tab.range, range, sizeof tab.range);
    const size_t plane = wls_plane_bytes(n, H, W);
    char *ws = (char *)workspace;
    WlsArgs a;
    a.in = in, a.conf = conf, a.guide = guide;
    a.U = (float *)ws, a.V = (float *)(ws + plane), a.E = (float *)(ws + 2 * plane);
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
