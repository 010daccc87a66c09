// tu_sgm.hip -- semi-global matching (k_sgm.h).
#include "k_sgm.h"
#include "smx_launch.h"
#include "smx_workspace.h"

namespace smx {

namespace {

template <int DPL>
void launch_dpl(const SgmPathArgs &base, int paths, const SgmSelectArgs &sel, hipStream_t s) {
    const int axes = paths == 8 ? 4 : 2;
    for (int ax = 0; ax < axes; ++ax) {
        SgmPathArgs a = base;
        a.axis = ax;
        a.lines = ax == SGM_HORIZONTAL ? a.H : ax == SGM_VERTICAL ? a.W : a.H + a.W - 1;
        a.init = ax == 0;
        const size_t waves = (size_t)a.n * a.lines;
        const unsigned grid = (unsigned)((waves + SGM_THREADS / 64 - 1) / (SGM_THREADS / 64));
        hipLaunchKernelGGL((k_sgm_paths<DPL>), dim3(grid), dim3(SGM_THREADS), 0, s, a);
    }
    const size_t pixels = (size_t)sel.n * sel.H * sel.W;
    const size_t groups = (pixels + SGM_THREADS / 64 - 1) / (SGM_THREADS / 64);
    const unsigned grid = (unsigned)(groups < ((size_t)1 << 20) ? groups : ((size_t)1 << 20));   // grid-stride beyond
    if (sel.lr || sel.right_out) hipLaunchKernelGGL((k_sgm_right_wta<DPL>), dim3(grid), dim3(SGM_THREADS), 0, s, sel);
    hipLaunchKernelGGL((k_sgm_select<DPL>), dim3(grid), dim3(SGM_THREADS), 0, s, sel);
}

}  // namespace

void launch_sgm(int n, int C, bool f32, int H, int W, const void *left, const void *right, int dmin, int D, int paths,
                int P1, int P2, int uniqueness, float lr_max_diff, bool subpixel, float invalid, float *out,
                float *gray_out, float *right_out, void *workspace, hipStream_t s) {
    const SgmLayout l = sgm_layout(n, H, W, D);
    uint64_t *cen_l = ws_at<uint64_t>(workspace, l.cen_l), *cen_r = ws_at<uint64_t>(workspace, l.cen_r);
    uint16_t *S = ws_at<uint16_t>(workspace, l.S);
    int16_t *iR = ws_at<int16_t>(workspace, l.iR);
    const int tiles_x = (W + SGM_TW - 1) / SGM_TW, tiles_y = (H + SGM_TH - 1) / SGM_TH;
    const unsigned images = (unsigned)(2 * n < 65535 ? 2 * n : 65535);            // grid-stride beyond
    hipLaunchKernelGGL(k_sgm_census, dim3(tiles_x * tiles_y, images), dim3(SGM_THREADS), 0, s, left, right, C, (int)f32,
                       n, H, W, tiles_x, cen_l, cen_r, gray_out);
    SgmPathArgs a;
    a.cen_l = cen_l;
    a.cen_r = cen_r;
    a.S = S;
    a.n = n, a.H = H, a.W = W, a.dmin = dmin, a.D = D, a.Dp = l.Dp, a.P1 = P1, a.P2 = P2;
    a.axis = 0, a.lines = 0, a.init = 1;
    SgmSelectArgs sel;
    sel.S = S;
    sel.iR = iR;
    sel.out = out;
    sel.right_out = right_out;
    sel.n = n, sel.H = H, sel.W = W, sel.dmin = dmin, sel.D = D, sel.Dp = a.Dp;
    sel.uniqueness = uniqueness, sel.lr = lr_max_diff >= 0.0f, sel.subpixel = subpixel;
    sel.lr_max_diff = lr_max_diff, sel.invalid = invalid;
    switch (sgm_dpl(D)) {
    case 1: launch_dpl<1>(a, paths, sel, s); break;
    case 2: launch_dpl<2>(a, paths, sel, s); break;
    default: launch_dpl<4>(a, paths, sel, s); break;
    }
}

}  // namespace smx
