// What the synthesis head's host code chooses for a case (k_synthesis_grad.h: syn_grad_shape, synthesis_grad_chunk,
// syg_row_floats, syg_lds_floats; k_synthesis.h: synthesis_chunk, syn_lds_floats; the tile counts as
// launch_synthesis_grad and launch_head compute them), compiled for the host like the plan harnesses: the headers' own
// lines, no HIP runtime.  tests/test_synthesis_paths_cpu.py compares every line with tests/synthesis_paths.py.
//
//   synthesis_paths_harness < cases       one "C D h w S" per line in, one line per case out:
//       grad rows_log2 tj_log2 NT U ti tiles_i tiles_j dc rs lds threads  head dc lds tiles_x tiles_y
//   and a last line "limits <SYG_LDS_FLOATS> <SYN_LDS_FLOATS> cases <n>"
#include <cstdio>

#include "k_synthesis_grad.h"

using namespace smx;

int main() {
    int C, D, h, w, S, cases = 0;
    while (scanf("%d %d %d %d %d", &C, &D, &h, &w, &S) == 5) {
        const SynGradShape sh = syn_grad_shape(S);
        const int rows = 1 << sh.rows_log2, tj = 1 << sh.tj_log2;
        const int ti = rows / S - 1;
        const int tiles_j = (w + tj - 1) / tj, tiles_i = (h + ti - 1) / ti;
        const int dc = synthesis_grad_chunk(C, D, S);
        const int rs = syg_row_floats(S, tj, sh.NT, dc);
        const int lds = syg_lds_floats(C, S, rows, tj, sh.NT, sh.U, dc);
        const int H = h * S, W = w * S;
        const int fdc = synthesis_chunk(C, D, S, h, w);
        const int flds = syn_lds_floats(C, fdc, S, h, w);
        const int tiles_x = (W + SYN_TW - 1) / SYN_TW, tiles_y = (H + SYN_TH - 1) / SYN_TH;
        printf("grad %d %d %d %d %d %d %d %d %d %d %d  head %d %d %d %d\n", sh.rows_log2, sh.tj_log2, sh.NT, sh.U, ti, tiles_i,
               tiles_j, dc, rs, lds, rows * tj, fdc, flds, tiles_x, tiles_y);
        ++cases;
    }
    printf("limits %d %d cases %d\n", SYG_LDS_FLOATS, SYN_LDS_FLOATS, cases);
    return 0;
}
