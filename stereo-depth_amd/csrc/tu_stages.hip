// tu_stages.hip -- the kernels around the aggregation: steps 1-2 (k_prologue.h), step 6 (k_refine.h), steps 7-9
// (k_fill.h) and the "next"-row kernels (device metrics, disparity -> points).
#include "k_fill.h"
#include "k_metrics.h"
#include "k_points.h"
#include "k_prologue.h"
#include "k_refine.h"
#include "smx_launch.h"

namespace smx {

namespace {
__global__ void k_flag_to_bool(const int *flag, int epoch, int *out) { *out = (*flag == epoch) ? 1 : 0; }

template <int MODE>
void prologue_t(int kernel, const PrologueArgs &a, int n, hipStream_t s) {
    const dim3 block(64, 4), grid((a.w + 63) / 64, (a.h + 3) / 4, n);
    switch (kernel) {
        case PROLOGUE_K2: {   // two pooled pixels per thread, 16-byte loads (gray entries, K = 2, even width)
            constexpr int M2 = (MODE == IN_GRAY_U8) ? IN_GRAY_U8 : IN_GRAY_F32;
            hipLaunchKernelGGL((k_prologue_k2<M2>), dim3((a.w + 127) / 128, grid.y, n), block, 0, s, a.left, a.right, a.gray_l, a.gray_r,
                               a.down_l, a.down_r, a.flags, a.g8_l, a.g8_r, a.flags2, a.H, a.W, a.h, a.w,
                               a.pitch8, a.padl, a.padr, a.epoch, a.gpitch, a.gpadl, a.units_l, a.units_r, a.upitch);
            return;
        }
        case PROLOGUE_K4:     // one pooled pixel = a 4 x 4 block read with four 16-byte loads per image and plane (K = 4, W a multiple of 4)
            hipLaunchKernelGGL((k_prologue_k4<MODE>), grid, block, 0, s, a.left, a.right, a.gray_l, a.gray_r, a.down_l,
                               a.down_r, a.flags, a.g8_l, a.g8_r, a.flags2, a.H, a.W, a.h, a.w,
                               a.pitch8, a.padl, a.padr, a.epoch, a.gpitch, a.gpadl, a.fp_conv, a.units_l, a.units_r, a.upitch);
            return;
        default:
            hipLaunchKernelGGL((k_prologue<MODE>), grid, block, 0, s, a.left, a.right, a.gray_l, a.gray_r, a.down_l,
                               a.down_r, a.flags, a.g8_l, a.g8_r, a.flags2, a.H, a.W, a.K, a.h, a.w,
                               a.grid_capable, a.pitch8, a.padl, a.padr, a.epoch, a.gpitch, a.gpadl, a.fp_conv, a.units_l, a.units_r, a.upitch);
    }
}
}  // namespace

// The three launchers below are tables from launch spec (smx_common.h; filled by plan_range, smx_plan.h) to instantiation.
void launch_prologue(const PrologueLaunch &x, const PrologueArgs &a, int n, hipStream_t s) {
    switch (x.in_mode) {
        case IN_GRAY_F32: prologue_t<IN_GRAY_F32>(x.kernel, a, n, s); break;
        case IN_RGB_F32: prologue_t<IN_RGB_F32>(x.kernel, a, n, s); break;
        case IN_RGB_U8: prologue_t<IN_RGB_U8>(x.kernel, a, n, s); break;
        default: prologue_t<IN_GRAY_U8>(x.kernel, a, n, s); break;
    }
}

void launch_refine(const RefineLaunch &x, const RefineParams &rp, int n, hipStream_t s) {
    const dim3 block(64, 4);
    const dim3 grid((rp.w + 63) / 64, (rp.h + 3) / 4, n);                       // one 64x4 tile of pooled pixels per workgroup
    const dim3 vgrid(grid.x, (rp.h + 4 * RV - 1) / (4 * RV), n);                // ... 64 x 4RV
    switch (x.kind) {
        case REFINE_FLOAT: {
            const dim3 fgrid(grid.x * grid.y, 1, n);
            if (x.apron) {                               // engine-owned gray with cyclic aprons: no border variant
                switch (x.kt) {
                    case 1: hipLaunchKernelGGL((k_refine<1, 5, true>), fgrid, block, 0, s, rp); return;
                    case 2: hipLaunchKernelGGL((k_refine<2, 5, true>), fgrid, block, 0, s, rp); return;
                    case 4: hipLaunchKernelGGL((k_refine<4, 5, true>), fgrid, block, 0, s, rp); return;
                    default: break;
                }
            }
            switch (x.kt) {
                case 1: hipLaunchKernelGGL((k_refine<1, 5, false>), fgrid, block, 0, s, rp); break;
                case 2: hipLaunchKernelGGL((k_refine<2, 5, false>), fgrid, block, 0, s, rp); break;
                case 4: hipLaunchKernelGGL((k_refine<4, 5, false>), fgrid, block, 0, s, rp); break;
                default: hipLaunchKernelGGL((k_refine<0, 0, false>), fgrid, block, 0, s, rp); break;
            }
            return;
        }
// the integer kernels come in two instantiations: SX = the SAD parabola is exact for this engine's disparities (k_refine.h
// refine_finish_int), the usual case, and the general one
#define SMX_LAUNCH_INT(KERNEL, GRID)                                                                            \
    switch (x.kt * 2 + (x.sad_exact ? 1 : 0)) {                                                                 \
        case 3: hipLaunchKernelGGL((KERNEL<1, true>), GRID, block, 0, s, rp); break;                            \
        case 2: hipLaunchKernelGGL((KERNEL<1, false>), GRID, block, 0, s, rp); break;                           \
        case 5: hipLaunchKernelGGL((KERNEL<2, true>), GRID, block, 0, s, rp); break;                            \
        case 4: hipLaunchKernelGGL((KERNEL<2, false>), GRID, block, 0, s, rp); break;                           \
        case 9: hipLaunchKernelGGL((KERNEL<4, true>), GRID, block, 0, s, rp); break;                            \
        default: hipLaunchKernelGGL((KERNEL<4, false>), GRID, block, 0, s, rp); break;                          \
    }
        case REFINE_INT: SMX_LAUNCH_INT(k_refine_int, grid) return;
        case REFINE_INT_V: SMX_LAUNCH_INT(k_refine_int_v, vgrid) return;
        case REFINE_AUTO: SMX_LAUNCH_INT(k_refine_auto, grid) return;
        default: SMX_LAUNCH_INT(k_refine_auto_v, vgrid) return;
#undef SMX_LAUNCH_INT
    }
}

// FillLaunch::px: output pixels per thread and row of k_fill4 (K = 2 / 4).  8 is the fastest shape on its own (0.065 ms per 64 C2
// pairs, 42 registers); 4 needs 28 registers, which is what fits beside three workgroups of the aggregation kernel
// (3 x 160 of a SIMD's 512 registers): on the stream lanes the fill of one half then runs INSIDE the other half's
// aggregation kernel instead of waiting for it to drain -- 84.4 k against 82.1 k pairs/s (profiles/r03_coresidency.txt).
void launch_fill(const FillLaunch &x, const FillParams &fp, int n, hipStream_t s) {
    const dim3 grid((fp.W + 255) / 256, fp.H, n);
    const dim3 grid8((fp.W + 256 * 8 - 1) / (256 * 8), fp.h, n), grid4((fp.W + 256 * 4 - 1) / (256 * 4), fp.h, n);
    switch (x.kernel) {
        case FILL_4:
            switch (x.K * 10 + x.px) {
                case 14: case 18: hipLaunchKernelGGL((k_fill4<1, 4>), grid4, dim3(256), 0, s, fp); break;
                case 24: hipLaunchKernelGGL((k_fill4<2, 4>), grid4, dim3(256), 0, s, fp); break;
                case 28: hipLaunchKernelGGL((k_fill4<2, 8>), grid8, dim3(256), 0, s, fp); break;
                case 44: hipLaunchKernelGGL((k_fill4<4, 4>), grid4, dim3(256), 0, s, fp); break;
                default: hipLaunchKernelGGL((k_fill4<4, 8>), grid8, dim3(256), 0, s, fp); break;
            }
            break;
        case FILL_POW2: hipLaunchKernelGGL(k_fill<true>, grid, dim3(256), 0, s, fp); break;
        default: hipLaunchKernelGGL(k_fill<false>, grid, dim3(256), 0, s, fp); break;
    }
}

void launch_flag_to_bool(const int *flag, int epoch, int *out, hipStream_t s) {
    hipLaunchKernelGGL(k_flag_to_bool, dim3(1), dim3(1), 0, s, flag, epoch, out);
}

void launch_metrics(int n, const float *est, const float *gt, const uint8_t *mask, size_t pixels, float max_disparity,
                    const float thresholds[4], double *out_sums, hipStream_t s) {
    MetricsParams mp{};
    mp.est = est; mp.gt = gt; mp.mask = mask; mp.out = out_sums; mp.pixels = pixels;
    mp.max_disp = max_disparity;
    for (int k = 0; k < 4; ++k) mp.thr[k] = thresholds[k];
    size_t blocks = (pixels + 256 * 8 - 1) / (256 * 8);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_metrics, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, s, mp);
}

void launch_points(const float *disp, int H, int W, float bf, float invalid, float *depth, float *points, int *count_dev,
                   int *workspace, hipStream_t s) {
    int *row_count = workspace, *row_offset = workspace + H;
    hipLaunchKernelGGL(k_depth_count, dim3(H), dim3(256), 0, s, disp, depth, row_count, W, bf, invalid);
    hipLaunchKernelGGL(k_row_scan, dim3(1), dim3(1024), 0, s, row_count, row_offset, count_dev, H);
    hipLaunchKernelGGL(k_points_scatter, dim3(H), dim3(256), 0, s, disp, row_offset, points, W, bf, invalid);
}

}  // namespace smx
