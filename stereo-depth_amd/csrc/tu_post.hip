// tu_post.hip -- disparity post-processing kernels (k_post.h): speckle filter and hole fill.
#include "k_post.h"
#include "smx_launch.h"
#include "smx_workspace.h"

namespace smx {

namespace {

unsigned stride_blocks(size_t items) {                     // grid-stride kernels: enough blocks, capped
    size_t blocks = (items + SPK_THREADS - 1) / SPK_THREADS;
    if (blocks > 8192) blocks = 8192;
    return (unsigned)blocks;
}

}  // namespace

void launch_filter_speckles(int n, int H, int W, const float *in, float *out, int max_size, float max_diff, float invalid,
                            void *workspace, hipStream_t s) {
    const size_t px = (size_t)n * H * W;
    const PostLayout l = post_layout(n, H, W);
    int *label = ws_at<int>(workspace, l.label), *size = ws_at<int>(workspace, l.size);
    const unsigned fin = stride_blocks(px);
    if (max_size == 0) {                                   // nothing is ever that small: a copy
        hipLaunchKernelGGL((k_spk_finalize<true>), dim3(fin), dim3(SPK_THREADS), 0, s, in, out, label, size, H, W, n,
                           max_size, invalid);
        return;
    }
    const unsigned tiles = (unsigned)((size_t)n * ((H + SPK_T - 1) / SPK_T) * ((W + SPK_T - 1) / SPK_T));
    hipLaunchKernelGGL(k_spk_local, dim3(tiles), dim3(SPK_THREADS), 0, s, in, label, size, H, W, max_diff, invalid);
    hipLaunchKernelGGL(k_spk_merge, dim3(tiles), dim3(2 * SPK_T), 0, s, in, label, H, W, max_diff, invalid);
    hipLaunchKernelGGL(k_spk_flatten, dim3(fin), dim3(SPK_THREADS), 0, s, label, H, W, n);
    hipLaunchKernelGGL(k_spk_count, dim3(tiles), dim3(SPK_THREADS), 0, s, (const int *)label, size, H, W);
    hipLaunchKernelGGL((k_spk_finalize<false>), dim3(fin), dim3(SPK_THREADS), 0, s, in, out, (const int *)label,
                       (const int *)size, H, W, n, max_size, invalid);
}

void launch_fill_invalid(int n, int H, int W, const float *in, float *out, float invalid, void *workspace, hipStream_t s) {
    int *flags = ws_at<int>(workspace, post_layout(n, H, W).flags);
    const dim3 rows((unsigned)((size_t)n * H));
    if (W <= FILL_LDS_W)
        hipLaunchKernelGGL((k_fill_rows<true>), rows, dim3(FILL_THREADS), 0, s, in, out, flags, W, invalid);
    else
        hipLaunchKernelGGL((k_fill_rows<false>), rows, dim3(FILL_THREADS), 0, s, in, out, flags, W, invalid);
    hipLaunchKernelGGL(k_fill_cols, rows, dim3(FILL_THREADS), 0, s, out, (const int *)flags, H, W);
}

}  // namespace smx
