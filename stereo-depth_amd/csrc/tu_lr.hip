// tu_lr.hip -- the left-right consistency check's two kernels (k_lr.h): input pack / mirror and the check.
#include "k_lr.h"
#include "smx_launch.h"

namespace smx {

void launch_lr_pack(int elem_bytes, const void *l, const void *r, void *pl, void *pr, long rows, int W, hipStream_t s) {
    const size_t half = (size_t)rows * W;
    const uintptr_t a = (uintptr_t)l | (uintptr_t)r | (uintptr_t)pl | (uintptr_t)pr | (uintptr_t)(half * elem_bytes);
    const int vec = (a & 15u) == 0 ? 1 : 0;
    // enough work items for the widest of the four parts (straight: 16-byte chunks; mirrored: 4 elements per thread),
    // capped: the kernels stride over the rest
    const size_t straight = (half * elem_bytes + 15) / 16;
    const size_t mirrored = (size_t)rows * ((W + LR_PACK_ITEMS - 1) / LR_PACK_ITEMS);
    const size_t items = straight > mirrored ? straight : mirrored;
    size_t blocks = (items + LR_THREADS - 1) / LR_THREADS;
    if (blocks > 2048) blocks = 2048;
    const dim3 grid((unsigned)blocks, 4);
    if (elem_bytes == 4)
        hipLaunchKernelGGL(k_lr_pack<float>, grid, dim3(LR_THREADS), 0, s, (const float *)l, (const float *)r, (float *)pl,
                           (float *)pr, rows, W, vec);
    else
        hipLaunchKernelGGL(k_lr_pack<uint8_t>, grid, dim3(LR_THREADS), 0, s, (const uint8_t *)l, (const uint8_t *)r,
                           (uint8_t *)pl, (uint8_t *)pr, rows, W, vec);
}

void launch_lr_check(bool mirrored, const float *left, const float *right, float *out, float *right_out, int n, int H, int W,
                     float max_diff, float invalid, hipStream_t s) {
    const uintptr_t a = (uintptr_t)left | (uintptr_t)out;
    const int vec = ((W & 3) == 0 && (a & 15u) == 0) ? 1 : 0;
    const dim3 grid((unsigned)((size_t)n * H)), block(LR_THREADS);
    const bool lds = W <= LR_LDS_W;
#define SMX_LR_CHECK(M, S) hipLaunchKernelGGL((k_lr_check<M, S>), grid, block, 0, s, left, right, out, right_out, W, max_diff, invalid, vec)
    if (mirrored) {
        if (lds) SMX_LR_CHECK(true, true);
        else SMX_LR_CHECK(true, false);
    } else {
        if (lds) SMX_LR_CHECK(false, true);
        else SMX_LR_CHECK(false, false);
    }
#undef SMX_LR_CHECK
}

}  // namespace smx
